"""CPU-only: the crafted streams of tests/front_cases.py and its float64 model, proved on the oracle alone -- conditions on the INPUTS of
tests/test_gpu_front_stage.py, so that a device failure there is the device's.

  - the oracle stays in lock on every stream, with start = 504 and the same frame positions in the crafted frames;
  - the model's integer phase chain equals the oracle's oscillator in every frame;
  - the oracle's spectra (mixed in float, transformed in double, rounded once) differ from the model's by less than 4e-7 max|X| per symbol:
    a fifth of the device bound (1.7e-7 was measured when the test was written; an input that breaks this is changed, not the number);
  - the zero-correlation frames give the oracle a correlation of exactly (0, 0) and a fine-CFO step of exactly 0.0, in every quadrant
    range of |f| mod 1000 and for both signs of f;
  - the steered frames reach both sides of the +-20 degree clamp and both signs next to +-pi;
  - crafted null symbols occur with is_tii false and true;
  - the ring boundary falls, in two crafted frames of some stream, on every place of front_cases.PLACES, for every grid shape.
Prints the cover table and the oracle-against-model maximum."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import front_cases as fc
import oracle_lib as ol

ORACLE_BOUND = 4e-7
_SUMMARY = {}


def _summarise(st):
    """everything the tests below look at, without the spectra (a 48-stream case would hold 240 MB of them)"""
    o, kind = st["ora"], st["kind"]
    tr = o["trace"]["kind"]
    first_ok = int(np.argmax(tr == ol.EV_CORR_OK))
    N = st["n_frames"]
    walk = tr[first_ok:first_ok + 2 * N]
    r = dict(plan=st["plan"], kind=kind, families=st["families"], wrap=st["wrap"], null_crafted=sorted(st["null_crafted"]), n=int(o["n"]), n_frames=N, crafted=st["crafted"],
             locked=bool(np.array_equal(walk, np.tile([ol.EV_CORR_OK, ol.EV_FRAME_DONE], N))),
             start=o["start"][:N].tolist(), same_sym0=bool(np.array_equal(o["sym0"][:N], st["base_sym0"][:N])),
             fic_ratio=o["fic_ratio"][:N].tolist(), is_tii=o["is_tii"][:N].tolist(), f_sym=o["f_sym"][:N].tolist(),
             fc=o["fc"][:N].copy(), step=(o["fbb_end"][:N] - o["fbb"][:N]).tolist(),
             step_exact=[bool(o["fbb_end"][k] == o["fbb"][k]) for k in range(N)], chain=[], rel={}, fc_model={})
    for k in range(1, N):
        chain = int((int(o["phase_end"][k - 1]) - int(o["f_null"][k - 1]) * (int(o["start"][k]) + fc.TU)) % fc.FS)
        r["chain"].append(chain == int(o["phase_sym1"][k]) and int(o["f_sym"][k]) == int(np.round(o["fbb"][k])) and
                          int(o["f_null"][k]) == int(np.round(o["fbb_end"][k])))
    for k in st["crafted"]:
        m = fc.model_frame(st["vals"], o, k)
        r["chain"].append(m["phase_end"] == int(o["phase_end"][k]) and m["phase_sym1_chain"] == int(o["phase_sym1"][k]))
        mod = np.concatenate([m["phase_ref"][None], m["spec"], m["null"][None]])
        mx = np.abs(mod).max(axis=1)
        d = np.abs(o["spectra"][k].astype(np.complex128) - mod).max(axis=1)
        r["rel"][k] = (d, mx)
        r["fc_model"][k] = (m["cp"].sum() * np.exp(-2j * np.pi * (int(o["f_sym"][k]) % 1000) / 1000.0), float(m["cp_abs"].sum()))
    return r


def _case(case):
    if case not in _SUMMARY:
        n_streams, kind, variant = case
        fc.warm_up()
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            _SUMMARY[case] = list(pool.map(lambda s: _summarise(fc.build_stream(n_streams, kind, variant, s, spectra=True)), range(n_streams)))
    return _SUMMARY[case]


@pytest.mark.parametrize("case", fc.CASES, ids=["%d_%s_v%d" % c for c in fc.CASES])
def test_the_oracle_holds_its_lock_and_equals_the_model(case):
    worst, worst_at = 0.0, None
    for s, r in enumerate(_case(case)):
        N, crafted = r["n_frames"], r["crafted"]
        assert r["n"] >= N and r["locked"] and r["same_sym0"], (s, r["plan"], r["n"], r["start"])
        assert all(r["start"][k] == fc.TG for k in range(crafted[0] - fc.N_LOCK, N)), (s, r["start"])     # three frames in lock, the crafted ones, one behind
        assert all(r["fic_ratio"][k] == 0 for k in crafted), (s, r["fic_ratio"])          # the coarse-CFO branch runs in the crafted frames
        assert all(r["chain"]), (s, r["chain"])
        for k in crafted:
            d, mx = r["rel"][k]
            assert np.all(d <= ORACLE_BOUND * mx), (s, k, r["families"][k], float(np.max(d / np.where(mx > 0, mx, 1))))
            rel = float(np.max(np.where(mx > 0, d / np.where(mx > 0, mx, 1), 0.0)))
            if rel > worst:
                worst, worst_at = rel, (s, k, r["families"][k], int(np.argmax(np.where(mx > 0, d / np.where(mx > 0, mx, 1), 0.0))))
            # the oracle's summed correlation is the model's raw sums, turned once by e^{-j 2 pi f Tu / fs} (what k_frame_tail relies on):
            # one float accumulator over 75 x 504 products of mixed samples, so within (n + 8) 2^-24 of the sum of their moduli
            got, (want, moduli) = complex(r["fc"][k][0], r["fc"][k][1]), r["fc_model"][k]
            assert abs(got - want) <= (75 * fc.TG + 8) * 2.0 ** -24 * moduli, (s, k, got, want, moduli)
            if r["families"][k] == "zero" and r["kind"] != "u8":
                assert r["fc"][k].tobytes() == np.zeros(2, np.float32).tobytes() and r["step_exact"][k] and r["step"][k] == 0.0, (s, k, r["fc"][k])
    print("\n%d streams, %s ring, variant %d: oracle against model at most %.3g max|X| (stream, frame, family, symbol: %r); bound %.1g"
          % (case + (worst, worst_at, ORACLE_BOUND)))
    assert worst > 2e-8                                  # ... and the comparison is not an identity


def _shape(g):
    return [r for c in fc.CASES if fc.grid_of(c[0]) == g for r in _case(c)]


@pytest.mark.parametrize("g", [75, 25, 15])
def test_the_cases_cover_every_place_quadrant_angle_and_null_symbol(g):
    rs = _shape(g)
    places = fc.PLACES_G75 if g == 75 else fc.PLACES
    hit = {}
    for r in rs:
        if len(r["wrap"]) == 2:                          # the boundary falls in two crafted frames, at the place the stream was given
            hit.setdefault(r["plan"]["place"][0], []).append("%s:%s" % (r["kind"], "+".join(r["families"][k] for k in sorted(r["wrap"]))))
    print("\nG = %d: ring boundary at (frame-relative place: ring kind and the two crafted frames it falls in)" % g)
    for name, rel in places:
        print("  %-24s sym0%+7d  %s" % (name, rel, ", ".join(hit.get(name, ["-- not reached --"]))))
    assert all(name in hit for name, _ in places), [n for n, _ in places if n not in hit]
    assert all(len(r["wrap"]) == 2 for r in rs)
    # zero-correlation frames: quadrant range of |f| mod 1000 x sign of f (exact zeros: cf32 and s16 rings)
    quads = {}
    for r in rs:
        for k, fam in r["families"].items():
            if fam == "zero" and r["kind"] != "u8":
                quads.setdefault(fc.quadrant(r["f_sym"][k]), []).append(r["f_sym"][k])
    print("  zero-correlation frames, (sign of f, quadrant of |f| mod 1000) -> f:", {q: sorted(set(v))[:4] for q, v in sorted(quads.items())})
    need = [(sg, q) for sg in (1, -1) for q in range(4)]
    if g != 75:                                          # (15 streams cannot hold all eight; the two larger shapes must)
        assert all(q in quads for q in need), [q for q in need if q not in quads]
    assert (1, 2) in quads or (-1, 2) in quads           # the range in which k_frame_tail's rotation turned (+0, +0) into (-0, +0)
    # steered frames: the oracle's own angle
    # (cf32 and s16 rings: the rounding of a u8 ring's prefixes to codes moves the angle by some 0.01 degrees)
    ang = [float(np.degrees(np.arctan2(r["fc"][k][1], r["fc"][k][0]))) for r in rs for k, fam in r["families"].items() if fam == "steer" and r["kind"] != "u8"]
    print("  steered frames, the oracle's angle in degrees:", sorted(set(round(a, 3) for a in ang)))
    for want in (0.0, 19.9, -19.9, 20.1, -20.1, 179.99, -179.99):
        assert any(abs(a - want) < 0.005 for a in ang), (want, sorted(ang))
    assert any(19.0 < a < 20.0 for a in ang) and any(20.0 < a < 21.0 for a in ang) and any(-20.0 < a < -19.0 for a in ang) and any(-21.0 < a < -20.0 for a in ang)
    assert any(a > 179.9 for a in ang) and any(a < -179.9 for a in ang)
    steps = [r["step"][k] for r in rs for k, fam in r["families"].items() if fam == "steer" and r["kind"] != "u8"]
    lim = 20.0 / 360.0 * 1000.0
    assert any(abs(s - lim) < 1e-3 for s in steps) and any(abs(s + lim) < 1e-3 for s in steps) and any(1.0 < abs(s) < lim - 0.1 for s in steps)
    # crafted null symbols with and without TII
    tii = {bool(r["is_tii"][k]) for r in rs for k in r["null_crafted"]}
    print("  crafted null symbols with is_tii:", sorted(tii))
    assert tii == {False, True}
