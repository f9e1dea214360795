"""dabx_eti_frames_device: the device's ETI(NI) frame assembly (csrc/eti_core.h, one wavefront per frame, the kernel body of the delivery's
ETI stage) on crafted bytes, against the host's dabx_eti_frame and the oracle's ora_eti_frame (oracle/eti.c): every byte and every `used`
value equal.  The layouts are the smallest at which the lane slicing, the combination of the lanes' CRC shares or the copy can go wrong."""
import numpy as np
import pytest

import oracle_lib as ol
from dabstar_amd import lib as dx

pytestmark = pytest.mark.gpu


def D(i, cu, kbps, level, short=0):
    return dx.SubchDesc(i, cu, max(1, kbps * 3 // 4), kbps, level, short, 1, 0)


LAYOUTS = {
    # the MST is the 96 FIC bytes alone: 40 of the 64 lanes have nothing in the only round
    "none": [],
    "1x8": [D(5, 0, 8, 2)],
    "18x64": [D(i, 48 * i, 64, 2) for i in range(18)],
    # the header CRC runs over 4 + 4 * 64 + 2 = 262 bytes, every lane holds an STC word
    "64x8": [D(i, 6 * i, 8, 2) for i in range(64)],
    # short form levels 1-5, long form levels 0-7, start addresses above 255 (SAD's high bits) and a sub-channel size above 255 words (STL's)
    "mixed": [D(1, 0, 32, 1, 1), D(2, 24, 48, 2, 1), D(3, 260, 64, 3, 1), D(4, 310, 32, 4, 1), D(5, 863, 48, 5, 1)] +
             [D(10 + l, 300 + 60 * l, 8 * (l + 1), l) for l in range(7)] + [D(63, 768, 704, 7)],
    # 116 + 4 * 7 + 3 * 2000 = 6144: the frame is full, no padding byte, the EOF and TIST words are the frame's last
    "full": [D(i, 100 * i, 288, 2) for i in range(6)] + [D(6, 700, 272, 2)],
}
TOO_BIG = [D(i, 100 * i, 288, 2) for i in range(6)] + [D(6, 700, 280, 2)]
# (hi, lo, minor): nothing moves | lo wraps to 0, hi moves to 4 | the clamp at 20 | the fields' maxima | an even and an odd lo (the two FSYNCs)
COUNTERS = [(0, 0, 0), (3, 249, 1), (19, 249, 3), (31, 255, 3), (5, 100, 0), (5, 101, 0), (7, 248, 2), (0, 1, 3)]


def payload(kind, shape, rng):
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "ones":
        return np.full(shape, 0xFF, np.uint8)
    return rng.integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_device_frames_equal_the_hosts_and_the_oracles(name):
    subch = LAYOUTS[name]
    row = sum(3 * c.kbps for c in subch)
    rng = np.random.default_rng(len(name) + row)
    for kind in ("zero", "ones", "random"):       # (a message of zeros shows a wrong handling of the CRC's initial value)
        for n in (1, 2, 65):                      # more than one block, an odd count
            ctr = [COUNTERS[(i + n) % len(COUNTERS)] for i in range(n)]
            fic, msc = payload(kind, (n, 96), rng), payload(kind, (n, row), rng)
            out, used = dx.eti_frames_device([c[0] for c in ctr], [c[1] for c in ctr], [c[2] for c in ctr], subch, fic, msc)
            assert out.shape == (n, 6144) and used.shape == (n,)
            for f in range(n):
                parts, o = [], 0
                for c in subch:
                    parts.append(msc[f, o:o + 3 * c.kbps]); o += 3 * c.kbps
                want, w_used = dx.eti_frame(*ctr[f], subch, fic[f], parts)
                ora, o_used = ol.ora_eti_frame(*ctr[f], subch, fic[f], parts)
                assert w_used == o_used == used[f] == 12 + 4 * len(subch) + 96 + row + 8, (kind, n, f)
                assert np.array_equal(want, ora), (kind, n, f)
                bad = np.flatnonzero(out[f] != want)
                assert bad.size == 0, (kind, n, f, ctr[f], bad[:8], out[f][bad[:8]], want[bad[:8]])
    if name == "full":
        assert used[0] == 6144 and (out[:, -6:] == 0xFF).all()      # EOF CRC, RFU, TIST: the last 8 bytes
    elif name == "none":
        assert used[0] == 116 and (out[:, 116:] == 0x55).all()


def test_what_the_host_refuses_the_device_refuses():
    fic = np.zeros((1, 96), np.uint8)

    def refused(subch, hi=0, lo=0, minor=0):
        msc = np.zeros((1, sum(3 * c.kbps for c in subch)), np.uint8)
        with pytest.raises(dx.DabxError, match="libdabx error -2"):
            dx.eti_frames_device([hi], [lo], [minor], subch, fic, msc)
        return True

    # 8 kbit/s more than the full frame: both sides, DABX_E_ARG
    msc = [np.zeros(3 * c.kbps, np.uint8) for c in TOO_BIG]
    with pytest.raises(dx.DabxError):
        dx.eti_frame(0, 0, 0, TOO_BIG, fic[0], msc)
    assert refused(TOO_BIG)                       # (the oracle's assembly has no such check: it is not asked)
    E_ARG = -2
    L = dx.load()
    for subch in ([D(64, 0, 8, 2)], [D(1, 864, 8, 2)], [D(1, 0, 8, 8)], [D(1, 0, 8, 0, 1)], [D(1, 0, 8, 6, 1)], [D(1, 0, 1024, 2)]):
        with pytest.raises(dx.DabxError):
            dx.eti_frame(0, 0, 0, subch, fic[0], [np.zeros(3 * subch[0].kbps, np.uint8)])
        assert refused(subch)
    assert refused([], minor=4) and refused([], hi=-1) and refused([], lo=-1)
    # ... and a rate that is no multiple of 8, which the host form takes (no sub-channel of the standard has one: the device copies dwords)
    odd = [D(1, 0, 12, 2)]
    assert dx.eti_frame(0, 0, 0, odd, fic[0], [np.zeros(36, np.uint8)])[1] == 116 + 4 + 36
    assert refused(odd)
    arr = (dx.SubchDesc * 1)(D(1, 0, 8, 2))
    one = np.zeros(1, np.int32)
    assert L.dabx_eti_frames_device(0, dx._p(one), dx._p(one), dx._p(one), arr, 0, dx._p(fic), None, dx._p(np.zeros(6144, np.uint8)), dx._p(one)) == E_ARG
