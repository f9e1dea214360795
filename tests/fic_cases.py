"""Shared by test_fic_cases.py (no device) and test_gpu_fic_stage.py: adversarial soft-bit classes per 2304-bit FIC block, crafted FIBs
carried by clean coded blocks, the per-stream schedules, the model of the CIF-counter rule and the oracle run that gives every expected
value (oracle/fic.c through ora_fic_process_block, under each of its three Viterbi arithmetics)."""
import ctypes as C
import functools
import os
import sys

import numpy as np

import msc_cases as mc
import oracle_lib as ol

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

FIC_IN, FIC_OUT, K2 = 2304, 768, 3072
N_STREAMS, N_STEPS = 6, 24
ABSENT = {4: (5, 6, 13), 5: (0, 13, 22)}          # stream -> engine steps in which it has no frame (present = 0): 21 frames are left
CARRIER_EVERY = 3                                  # frames 0, 3, 6 ... of a stream are carrier frames: 4 clean coded blocks = 12 crafted FIBs


class OraFic(C.Structure):
    """ora_fic of oracle/dab_oracle.h (test_fic_cases.py checks the layout against ora_fic_map / ora_prbs)."""
    _fields_ = [("map", C.c_int32 * 3096), ("punct", C.c_uint8 * 3096), ("prbs", C.c_uint8 * 768), ("vit_in", C.c_int16 * 3096),
                ("soft", C.c_int16 * FIC_IN), ("fib_bits", C.c_uint8 * 3072), ("fic_valid", C.c_uint8 * 4), ("fib_crc", C.c_uint8 * 12),
                ("index", C.c_int), ("fic_idx", C.c_int), ("fic_block", C.c_int), ("fic_errors", C.c_int), ("fic_bits", C.c_int),
                ("success_ratio", C.c_int), ("cif_count", C.c_int), ("cif_hi", C.c_int), ("cif_lo", C.c_int)]


# ---- the model: ONE function for the CIF-counter rule --------------------------------------------------------------------------------
def model_fig00(fib):
    """(CIFCountHi, CIFCountLo) of the last FIG 0/0 the walk meets in one FIB of 32 bytes whose CRC is good, or None.  The reference's
    walk (fib_decoder.cpp:74-100, fib_decoder_fig0.cpp:95-101: no length check anywhere) wherever the bytes it reads lie inside the
    FIB's own 32 bytes; a FIG 0/0 header at byte 27 or later is ignored (there the reference reads its neighbour's bits)."""
    out, p = None, 0
    while p < 30:
        typ, ln = int(fib[p]) >> 5, int(fib[p]) & 0x1F
        if typ == 7 and ln == 0x1F:
            break
        if typ == 0 and p + 5 < 32 and (int(fib[p + 1]) & 0x1F) == 0:
            out = (int(fib[p + 4]) & 0x1F, int(fib[p + 5]))
        p += ln + 1
    return out


def reaches_late_fig00(fib):
    """Whether the walk meets a FIG 0/0 header at byte 27, 28 or 29: the cases on which the model and oracle/fic.c may differ."""
    p = 0
    while p < 30:
        typ, ln = int(fib[p]) >> 5, int(fib[p]) & 0x1F
        if typ == 7 and ln == 0x1F:
            break
        if typ == 0 and p >= 27 and (int(fib[p + 1]) & 0x1F) == 0:
            return True
        p += ln + 1
    return False


def model_track(cif, fibs, crc):
    """The counter after the FIBs of one launch, in FIB order: the last good FIB that carries a FIG 0/0 sets it."""
    for fib, ok in zip(fibs, crc):
        if ok:
            m = model_fig00(fib)
            if m is not None:
                cif = m[0] * 250 + m[1]
    return cif


# ---- FIBs ----------------------------------------------------------------------------------------------------------------------------
def make_fib(data, pad=True, good=True, fill=0x00):
    """30 data bytes (shorter: end marker + fill bytes when pad, zeros alone otherwise) + CRC; good = False flips one CRC bit."""
    data = bytes(data)
    assert len(data) <= 30
    if len(data) < 30:
        data += (b"\xFF" + bytes([fill]) * (29 - len(data))) if pad else bytes(30 - len(data))
    c = ds.crc16(data) ^ (0 if good else 0x0100)
    return np.frombuffer(data + bytes([c >> 8, c & 0xFF]), np.uint8).copy()


def crc_good(fib):
    return ds.crc16(bytes(fib[:30])) == (int(fib[30]) << 8 | int(fib[31]))


def fig00(hi, lo, length=5, second=0x00):
    return bytes([length & 0x1F, second, 0x10, 0xF2, hi & 0x1F, lo & 0xFF])


FILLER = make_fib(b"")                              # end marker first: no FIG at all


def _skip(n, typ=2):
    """One FIG of type typ that takes n bytes in all (header + n - 1 bytes that are no headers to anybody)."""
    assert 1 <= n <= 32
    return bytes([(typ << 5) | (n - 1)]) + bytes([0xA5] * (n - 1))


def _late(p):
    """FIG 0/0 header at byte p >= 27; for p = 29 the extension lies in the first CRC byte, so the filler is searched until that byte's low
    five bits are 0 (the reference then sees a FIG 0/0 there)."""
    for k in range(256):
        front = bytes([(3 << 5) | (p - 1), k] + [0xA5] * (p - 2))       # one FIG of type 3 that takes bytes 0 .. p - 1
        data = front + fig00(7, 77)[:30 - p]
        f = make_fib(data)
        if p + 1 < 30 or (int(f[30]) & 0x1F) == 0:
            return f
    raise AssertionError(p)


def crafted_singles():
    """[(name, fib32)]: every one with a good CRC and, where it carries a counter, a counter no other case carries."""
    n = [0]

    def c():                                        # a fresh (hi, lo): hi 0..19, lo over the whole byte
        n[0] += 1
        return (n[0] * 7) % 20, (n[0] * 37 + 11) % 256
    out = [("fig00_first", make_fib(fig00(*c())))]
    out.append(("behind_fig0_1", make_fib(bytes([0x04, 0x01, 0x04, 0x00, 0x10]) + fig00(*c()))))
    out.append(("behind_fig0_2", make_fib(bytes([0x06, 0x02, 0x10, 0x01, 0x01, 0x3F, 0x06]) + fig00(*c()))))
    out.append(("behind_type1", make_fib(bytes([0x35, 0x00]) + b"ABCDEFGHIJKLMNOPabcd" + fig00(*c()))))
    for t in range(2, 7):
        out.append(("behind_type%d" % t, make_fib(_skip(4, t) + fig00(*c()))))
    a, b = c(), c()
    out.append(("two_fig00_last_wins", make_fib(fig00(*a) + fig00(*b))))
    for name, second in (("flag_cn", 0x80), ("flag_oe", 0x40), ("flag_pd", 0x20), ("flags_all", 0xE0)):
        out.append((name, make_fib(fig00(*c(), second=second))))
    out.append(("end_marker_in_front", make_fib(b"\xFF" + fig00(*c()))))
    out.append(("type7_e3", make_fib(bytes([0xE3, 1, 2, 3]) + fig00(*c()))))
    out.append(("type7_e0", make_fib(bytes([0xE0]) + fig00(*c()))))
    out.append(("type7_f0", make_fib(bytes([0xF0] + [0x5A] * 16) + fig00(*c()))))
    out.append(("type7_fe_swallows_all", make_fib(bytes([0xFE]) + fig00(*c()))))
    for ln in range(5):
        # what lies behind a short FIG 0/0 is walked as FIGs (its own EId and counter bytes first): 0xFF everywhere ends that walk
        out.append(("fig00_length_%d" % ln, make_fib(fig00(*c(), length=ln), fill=0xFF)))
    out.append(("fig00_length_4_then_fig", make_fib(fig00(9, 0x42, length=4) + bytes([0x11, 0x33]), fill=0xFF)))
    out.append(("fig_runs_past_30", make_fib(fig00(*c()) + _skip(14) + bytes([0x34]) + bytes([0x11] * 9))))
    out.append(("fig00_runs_past_30", make_fib(_skip(22) + fig00(*c(), length=12) + bytes([0x5A, 0x5A]))))
    out.append(("fig0_1_length_31", make_fib(bytes([0x1F, 0x01]) + bytes([0x00] * 4) + fig00(*c()))))
    for p in (24, 25, 26):
        out.append(("header_at_%d" % p, make_fib((_skip(p) + fig00(*c()))[:30])))
    for p in (27, 28, 29):
        out.append(("header_at_%d" % p, _late(p)))
    out.append(("fig00_then_zeros", make_fib(fig00(*c()), pad=False)))
    out.append(("all_zero", make_fib(b"", pad=False)))
    out.append(("zeros_then_bytes", make_fib(bytes(9) + bytes([0x20, 0x05, 0x13, 0x00, 0x00, 0x29]), pad=False)))
    for hi in range(20, 32):
        out.append(("cif_hi_%d" % hi, make_fib(fig00(hi, (hi * 29 + 3) % 256))))
    return out


NO_FIG00 = [("no_fig00_filler", FILLER),
            ("no_fig00_fig0_1", make_fib(bytes([0x04, 0x01, 0x08, 0x00, 0x10]))),
            ("no_fig00_type1", make_fib(bytes([0x35, 0x00]) + b"ABCDEFGHIJKLMNOPabcd"))]


def broken(fib):
    out = fib.copy()
    out[30] ^= 0x01
    return out


def later_fib_wins_blocks():
    """Two blocks of three FIBs: good A, bad-CRC C, good B (B's counter must stand) and good A, bad-CRC C, filler (A's must)."""
    a, b, c = make_fib(fig00(3, 201)), make_fib(fig00(4, 202)), broken(make_fib(fig00(5, 203)))
    return [a, c, b, make_fib(fig00(6, 204)), broken(make_fib(fig00(8, 205))), FILLER]


@functools.lru_cache(maxsize=None)
def random_fibs(n=2000, seed=20262):
    rng = np.random.default_rng(seed)
    return [make_fib(rng.integers(0, 256, 30).astype(np.uint8).tobytes()) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def sparse_fibs(n=1000, seed=20264):
    """Random FIBs with a valid CRC whose bytes are thinned by random masks: short FIGs, type 0 and extension 0 are frequent, so many
    of them carry one or more FIG 0/0 (of 2000 uniformly random FIBs about 1 in 100 does)."""
    rng = np.random.default_rng(seed)
    masks = np.array([0xFF, 0x1F, 0xE0, 0x07, 0x03, 0x00], np.uint8)
    return [make_fib((rng.integers(0, 256, 30).astype(np.uint8) & rng.choice(masks, 30)).tobytes()) for _ in range(n)]


# ---- soft bits -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fic_tables():
    n_in, m = ol.ora_fic_map()
    assert n_in == FIC_IN
    prbs = np.zeros(FIC_OUT, np.uint8)
    ol.oracle().ora_prbs(prbs, FIC_OUT)
    return m, prbs


def coded_block(fibs3, amp=100):
    """Three FIBs -> the 2304 transmitted soft bits of one FIC block at +-amp (energy dispersal, mother code, the oracle's puncturing)."""
    m, prbs = _fic_tables()
    bits = np.unpackbits(np.concatenate([np.asarray(f, np.uint8) for f in fibs3]))
    code = ds.conv_encode(bits ^ prbs).astype(np.int32)
    soft = np.zeros(FIC_IN, np.int32)
    tx = m >= 0
    soft[m[tx]] = (2 * code[tx] - 1) * amp
    return soft.astype(np.int16)


_MSC = dict(mc.CLASSES)
ADVERSARIAL = ("noise", "zero", "plus127", "minus127", "ternary", "sign127", "int16_edges", "byte_edges", "wide", "noisy")
CLASS_NAMES = ADVERSARIAL + ("clean",)
TIE_MAKERS = mc.TIE_MAKERS
NOISY_SIGMA = 105                                   # on +-100: most blocks lose one or two of their three FIBs


def class_block(name, rng, fibs3=None):
    if name == "clean":
        return coded_block(fibs3)
    if name == "noisy":
        return np.clip(coded_block(fibs3).astype(np.float64) + rng.normal(0, NOISY_SIGMA, FIC_IN), -32768, 32767).astype(np.int16)
    return np.asarray(_MSC[name](rng, None, FIC_IN)).astype(np.int16)


# ---- schedules -----------------------------------------------------------------------------------------------------------------------
def crafted_sequence(s):
    """The FIBs stream s carries in its carrier frames, twelve per frame.  Streams 0-2: good CRCs only (but for the middle FIB of the
    'later FIB wins' blocks); streams 3-5: every crafted case followed by the broken-CRC variant of ANOTHER case, whose counter would
    show if the kernel walked it."""
    singles = [f for _, f in crafted_singles()]
    rnd = sparse_fibs()
    if s < 3:
        seq = later_fib_wins_blocks() + singles
        seq += rnd[100 * s:100 * s + (-len(seq)) % 12]
        if s == 1:                                   # a whole frame without any FIG 0/0 behind the frame that set the counter
            seq = seq[:12] + [NO_FIG00[i % 3][1] for i in range(12)] + seq[12:]
        if s == 2:                                   # the same cases in other frames (and behind other class blocks) than in stream 0
            seq = seq[48:] + seq[:48]
    else:
        n = len(singles)
        seq = []
        for i in range(n):
            seq += [singles[i], broken(singles[(i + 7) % n])]
        k = (32 * (s - 3)) % len(seq)
        seq = seq[k:] + seq[:k]
    seq = seq + rnd[300 + 100 * s:300 + 100 * s + 96]
    return seq[:96]


def block_kinds(s, n_frames):
    """[(class name) per block] of stream s's frames: carrier frames are 'clean'; in the others class (j + 3 b + s) % 10 for block b of
    the j-th such frame, so that every class meets every block position within ten of them."""
    kinds, j = [], 0
    for f in range(n_frames):
        if f % CARRIER_EVERY == 0:
            kinds.append(["clean"] * 4)
        else:
            kinds.append([ADVERSARIAL[(j + 3 * b + s) % len(ADVERSARIAL)] for b in range(4)])
            j += 1
    return kinds


def stream_frames_count(s):
    return N_STEPS - len(ABSENT.get(s, ()))


@functools.lru_cache(maxsize=None)
def stream_frames(s):
    """(soft [n_frames, 9216] int16, kinds [n_frames][4]) of stream s, the frames it is present in, one after the other."""
    n = stream_frames_count(s)
    rng = np.random.default_rng([20263, s])
    kinds = block_kinds(s, n)
    seq, rnd = crafted_sequence(s), random_fibs()          # noisy blocks: uniformly random FIBs
    soft = np.zeros((n, 4, FIC_IN), np.int16)
    at = r = 0
    for f in range(n):
        for b in range(4):
            k = kinds[f][b]
            fibs3 = None
            if k == "clean":
                fibs3, at = seq[at:at + 3], at + 3
            elif k == "noisy":
                fibs3, r = rnd[700 + 150 * s + r:700 + 150 * s + r + 3], r + 3
            soft[f, b] = class_block(k, rng, fibs3)
    soft = soft.reshape(n, 4 * FIC_IN)
    soft.setflags(write=False)
    return soft, kinds


def symbol_calls(frames, short_after=None):
    """[(3072 soft bits, sym_idx)] for whole frames; short_after = f: one more frame in front of frame f that ends after its symbol 1 (its
    soft bits are frame f's, negated and halved)."""
    calls = []
    for f in range(frames.shape[0]):
        if short_after is not None and f == short_after:
            calls.append((np.ascontiguousarray(-(frames[f, :K2] // 2)), 1))
        for sym in range(3):
            calls.append((np.ascontiguousarray(frames[f, sym * K2:(sym + 1) * K2]), sym + 1))
    return calls


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def ora_block_errors(soft_block, dec_bits):
    """ora_viterbi_ber of one block: channel errors at its 2304 transmitted positions against the re-encoded decoded bits."""
    m, _ = _fic_tables()
    blk = np.zeros(3096, np.int16)
    blk[m >= 0] = soft_block[m[m >= 0]]
    b, e = C.c_int(0), C.c_int(0)
    ol.oracle().ora_viterbi_ber(blk, (m >= 0).astype(np.uint8), np.ascontiguousarray(dec_bits, np.uint8), FIC_OUT, C.byref(b), C.byref(e))
    assert b.value == FIC_IN
    return e.value


def oracle_calls(calls, mode):
    """oracle/fic.c over a list of symbol calls under ora_set_viterbi_mode(mode).  One record per call: the FIBs [12, 32] and CRC verdicts
    [12] as they stand, success_ratio, the BER pair, the block count, the oracle's CIF counter, the list of blocks the call completed,
    `ber_wrap`: in mode 0 the BER pair with every soft bit >= 32641 counted as a negative one (what the scalar build's `soft + 127` makes
    of it before the kernel's hard decision; differs from the oracle's pair only behind such a block; modes 1 and 2: the oracle's pair), and `wrap_blocks`: how many of the
    completed blocks held such a soft bit."""
    _, prbs = _fic_tables()
    L = ol.oracle()
    f = OraFic()
    L.ora_fic_init(C.byref(f))
    out = []
    index = done = 0
    bits = errs = blk = 0
    acc = np.zeros(4 * FIC_IN, np.int16)
    L.ora_set_viterbi_mode(mode)
    try:
        for soft, sym in calls:
            if sym == 1:
                index = done = 0
            L.ora_fic_process_block(C.byref(f), soft, sym)
            acc[done * FIC_IN + index:done * FIC_IN + index + K2] = soft
            total = index + K2
            completed = list(range(done, done + total // FIC_IN))
            index, done = total % FIC_IN, done + total // FIC_IN
            fb = np.frombuffer(f.fib_bits, np.uint8).reshape(4, FIC_OUT).copy()
            wrap_blocks = 0
            for b in completed:
                sb = acc[b * FIC_IN:(b + 1) * FIC_IN]
                wrapped = np.where(sb >= 32641, np.int16(-1), sb) if mode == 0 else sb       # modes 1, 2 saturate: nothing wraps
                wrap_blocks += int((sb >= 32641).any())
                bits += FIC_IN
                errs += ora_block_errors(wrapped, fb[b] ^ prbs)
                blk += 1
                if blk == 40:
                    blk, errs, bits = 0, errs // 2, bits // 2
            out.append(dict(fibs=np.packbits(fb.reshape(12, 256), axis=1), crc=np.frombuffer(f.fib_crc, np.uint8).copy(),
                            ratio=f.success_ratio, ber=(f.fic_bits, f.fic_errors), blocks=f.fic_block, cif=f.cif_count,
                            completed=completed, ber_wrap=(bits, errs), wrap_blocks=wrap_blocks))
            assert blk == f.fic_block and bits == f.fic_bits
    finally:
        L.ora_set_viterbi_mode(0)
    return out


@functools.lru_cache(maxsize=None)
def oracle_stream(s, mode):
    """One record per frame of stream s (the record of its symbol 3) plus `cif_model`: model_track over the oracle's own FIBs."""
    soft, _ = stream_frames(s)
    recs = oracle_calls(symbol_calls(soft), mode)[2::3]
    cif = 0
    for r in recs:
        cif = r["cif_model"] = model_track(cif, r["fibs"], r["crc"])
    return recs
