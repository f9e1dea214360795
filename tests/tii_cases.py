"""Inputs for the TII detector on the device (csrc/tii_core.h) and a float64 model of the detector (dabx_tii_process, csrc/tii.cpp) that
also reports how close each round came to deciding otherwise.

The device's detector keeps the host's order of every float sum and product; only |z| and arg may differ from libm's in the last bits.  A
round whose every decision has a relative margin of at least MIN_MARGIN (1e-5, about 170 float ulps) must therefore give the same ids,
sub-ids, flags and order on the device as on the host: the margin is a condition on the INPUTS (tests/test_tii_cases.py proves it on the
CPU), not a tolerance on the kernel.  Decisions whose two sides are exactly equal by construction (0 against 0; the strengths of one
collision list, which are one number) have no margin: no arithmetic can move them apart."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402
import test_tii  # noqa: E402

MIN_MARGIN = 1e-5
P_0F, P_3C, P_F0 = (ds.TII_PATTERNS.index(v) for v in (0x0F, 0x3C, 0xF0))


def _tables():
    i = np.arange(768)
    k = -768 + 2 * i
    c0 = np.where(k < 0, k, k + 1)
    b = np.where(c0 < 0, c0 + 2048, c0)
    prs = ds.prs_spectrum()
    q = lambda z: np.round(np.angle(z) / (np.pi / 2)).astype(int) & 3   # noqa: E731
    return b, (q(prs[b]) - q(prs[b + 1])) & 3


BIN, TURN = _tables()


def _margin(a, b):
    """smallest relative distance of the pairs (a, b); pairs that are both exactly 0 do not count"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    m = np.maximum(np.abs(a), np.abs(b))
    ok = m > 0
    return float(np.min(np.abs(a - b)[ok] / m[ok])) if ok.any() else np.inf


def model_round(acc, pairs, thr, collisions, coll_sub):
    """One dabx_tii_process in float64.  acc [2048] complex: the sum of the null-symbol spectra; pairs [768] complex128: the state, advanced
    in place.  Returns (results strongest first as (main, sub, strength, phase_deg, non_etsi), smallest margin, set of branches taken)."""
    acc = np.asarray(acc, np.complex128)
    pairs += 0.01 * (acc[BIN] * np.conj(acc[BIN + 1]) - pairs)
    work = pairs.copy().reshape(4, 192)
    margin, taken = np.inf, set()
    mag = np.abs(work)
    s, mx, at = mag.sum(0), mag.max(0), mag.argmax(0)              # (argmax: the first maximum, as the host's x > mx)
    two = np.sort(mag, 0)
    margin = min(margin, _margin(two[3], two[2]), _margin(s, 1.5 * mx))
    lone = (s < 1.5 * mx) & (mx > 0)
    if lone.any():
        taken.add("lone_carrier")
        cols = np.nonzero(lone)[0]
        work[at[cols], cols] *= ((s[cols] - mx[cols]) / 3) / mx[cols]
    etsi, turned = work.sum(0), (work * (-1j) ** TURN.reshape(4, 192)).sum(0)
    ea, ta = np.abs(etsi), np.abs(turned)
    top = max(ea.max(), ta.max())
    noise = min(1e9, ea.reshape(8, 24).mean(0).min())
    level = noise * float(np.power(np.float32(10), np.float32(thr) / np.float32(10)))
    margin = min(margin, _margin(ea, level), _margin(ta, level))
    res = []
    for sub in range(24):
        ix = sub + 24 * np.arange(8)
        ge, gt = ea[ix] > level, ta[ix] > level
        n_e, n_t = int(ge.sum()), int(gt.sum())
        s_e, s_t = etsi[ix][ge].sum() if n_e else 0j, turned[ix][gt].sum() if n_t else 0j
        non_etsi = False
        if n_e >= 4 or n_t >= 4:
            margin = min(margin, _margin(abs(s_t), abs(s_e)))
            non_etsi = abs(s_t) > abs(s_e)
        tab, tab_abs, hit, total = (turned, ta, gt, s_t) if non_etsi else (etsi, ea, ge, s_e)
        count = int(hit.sum())
        pat = int(sum(0x80 >> g for g in range(8) if hit[g]))
        if count < 4:
            continue
        taken.add("non_etsi" if non_etsi else "etsi")
        if count == 4:
            taken.add("count_4")
            main = ds.TII_PATTERNS.index(pat)
        else:
            taken.add("count_gt_4")
            cand = np.array([sum(tab[ix[g]] for g in range(8) if p & (0x80 >> g)) for p in ds.TII_PATTERNS])
            order = np.argsort(-np.abs(cand), kind="stable")
            margin = min(margin, _margin(abs(cand[order[0]]), abs(cand[order[1]])))
            main, total = int(order[0]), cand[order[0]]
        res.append((main, sub, abs(total) / top / 4, np.degrees(np.angle(total)), int(non_etsi)))
        if count > 4 and collisions:
            others = [g for g in range(8) if not (ds.TII_PATTERNS[main] & (0x80 >> g)) and hit[g]]
            rest = sum(tab[ix[g]] for g in others) if others else 0j
            strength = abs(rest) / top / (count - 4)
            if sub == coll_sub:
                taken.add("collision_list")
                for m, p in enumerate(ds.TII_PATTERNS):
                    if bin(p & pat).count("1") == 4 and m != main:
                        res.append((m, sub, strength, np.degrees(np.angle(rest)), int(non_etsi)))
            else:
                taken.add("collision_99")
                res.append((99, sub, strength, np.degrees(np.angle(rest)), int(non_etsi)))
    res.sort(key=lambda r: -r[2])                                  # (stable: equal strengths keep the order they were made in)
    st = np.array([r[2] for r in res])
    if len(st) > 1:
        differ = st[:-1] != st[1:]
        if differ.any():
            margin = min(margin, _margin(st[:-1][differ], st[1:][differ]))
    if not res:
        taken.add("no_result")
    if len(res) > 32:
        taken.add("more_than_32")
    return res, margin, taken


def run_model(collisions, sub_id, thr, rounds):
    """-> per round (results, margin, branches), the state carried from round to round"""
    pairs = np.zeros(768, np.complex128)
    return [model_round(np.sum([np.asarray(z, np.complex64) for z in r], axis=0, dtype=np.complex128), pairs, thr, collisions, sub_id) for r in rounds]


def round_sums(rounds):
    """the float32 sum a detector is handed per round: the spectra added one by one, as dabx_tii_add does"""
    out = []
    for r in rounds:
        a = np.zeros(2048, np.complex64)
        for z in r:
            a = (a + np.asarray(z, np.complex64)).astype(np.complex64)
        out.append(a)
    return out


def new_scenarios():
    """name -> (collisions, sub_id, threshold_db, rounds), as test_tii.scenarios(); the branch each is named for: BRANCH"""
    def maker(seed):
        rng = np.random.default_rng(seed)

        def sp(*tx, s=0.02, scale=1.0):
            z = (rng.standard_normal(2048) + 1j * rng.standard_normal(2048)) * s
            for (m, c, a, e) in tx:
                z = z + ds.tii_null_spectrum(m, c, a, e) * np.exp(1j * rng.uniform(0, 2 * np.pi))
            return (z * scale).astype(np.complex64)
        return rng, sp

    sc = {}
    sc["all_zero"] = (0, 0, 8, [[np.zeros(2048, np.complex64)] * 3 for _ in range(2)])
    _, sp = maker(11)
    sc["huge_1e11"] = (0, 0, 6, [[sp((12, 5, 1.0, True), (44, 20, 0.5, False), scale=1e11) for _ in range(4)] for _ in range(3)])
    _, sp = maker(12)
    sc["tiny_1e-11"] = (0, 0, 6, [[sp((12, 5, 1.0, True), (44, 20, 0.5, False), scale=1e-11) for _ in range(4)] for _ in range(3)])
    # 23 of the 24 sub-ids carry two transmitters whose patterns share two groups (six groups above the level: a best-of-70 search each),
    # with the collision listing on that is a main id and a "99" per sub-id: 46 results
    rng, sp = maker(13)
    amps = [(float(rng.uniform(0.4, 1.0)), float(rng.uniform(0.4, 1.0))) for _ in range(23)]
    crowd = [t for c, (a, b) in enumerate(amps) for t in ((P_0F, c, a, True), (P_3C, c, b, True))]
    sc["crowded"] = (1, 99, 6, [[sp(*crowd) for _ in range(3)] for _ in range(2)])
    _, sp = maker(14)
    sc["collision_99_three"] = (1, 3, 6, [[sp((P_0F, 7, 1.0, True), (P_3C, 7, 0.7, True), (P_F0, 7, 0.5, True), (20, 2, 0.6, True)) for _ in range(4)] for _ in range(2)])
    _, sp = maker(15)
    sc["collision_list_six"] = (1, 7, 6, [[sp((P_0F, 7, 1.0, True), (P_3C, 7, 0.7, True)) for _ in range(4)] for _ in range(2)])
    # a transmitter that is there for a round and then gone, another that comes later: what the IIR carries decides rounds 2 to 4
    _, sp = maker(16)
    sc["state_carries"] = (0, 0, 6, [[sp((30, 4, 1.0, True)) for _ in range(5)], [sp() for _ in range(5)], [sp((61, 15, 0.4, False)) for _ in range(5)],
                                     [sp((61, 15, 0.4, False)) for _ in range(5)]])
    return sc


BRANCH = {"all_zero": "no_result", "huge_1e11": "non_etsi", "tiny_1e-11": "non_etsi", "crowded": "more_than_32", "collision_99_three": "collision_99",
          "collision_list_six": "collision_list", "state_carries": "non_etsi",
          "single": "count_4", "three_tx": "count_4", "non_etsi": "non_etsi", "collision_99": "collision_99", "collision_list": "collision_list",
          "lone_carrier": "lone_carrier", "noise_only": "no_result", "weak_low_threshold": "etsi"}


def all_scenarios():
    sc = dict(test_tii.scenarios())
    sc.update(new_scenarios())
    return sc
