"""Crafted streams for the DC / IQ correction (k_dciq, csrc/pipeline.hip), its references, and a float32 restatement of the kernel's tile
algorithm.  No device anywhere in this file: tests/test_dciq_cases.py proves the cases, the cover and the bounds on the CPU,
tests/test_gpu_dciq_stage.py holds the device to the float64 reference under those bounds.

A CASE is one engine of three streams with a two-frame ring: per stream its own samples and its own partition into LAUNCHES (k_dciq runs
over all streams at every push or commit of any of them and starts its tiles of 4096 samples at the stream's dciq_done, so the partition
is part of the input).  case["groups"] is the list of launch groups, each a vector of new samples per stream (0: the stream is idle);
after every group the tests look at every stream.

References (run_reference):
  f64       the oracle's ora_dciq_buffer_f64, the five filters with double states, sample by sample: THE expectation
  f32       the oracle's ora_dciq_buffer, the reference receiver's own float recurrence: recorded as the reference's rounding noise, no bound
  closed    closed_form(): numpy float64, y_n = (1 - a)^n y_0 + a (1 - a)^n cumsum(x_k / (1 - a)^k) level by level (the second reference)
The RESTATEMENT (restate) repeats k_dciq in numpy float32, lane by lane, operation by operation (-ffp-contract=off on the device: every
operation is one IEEE operation; np.float32 division and square root are correctly rounded, as the device's).  It is not a reference: it
shows what a correct scan's error is (the bounds are 4 x its distance from f64, at least 2^-23 of the scale) and, with a MUTATION named,
that the bounds catch the faults such a kernel can have."""
import numpy as np

import oracle_lib as ol

TF, FS = 196608, 2048000
RING = 2 * TF                                            # ring_frames = 2
S = 3
PER, TILE = 16, 4096
F32 = np.float32
ALPHA = F32(1.0) / F32(FS)
INIT = (0.0, 0.0, 1.0, 1.0, 0.0)                         # meanI, meanQ, meanII, meanQQ, meanIQ (sample_reader.h:102-106)
STATE_NAMES = ("meanI", "meanQ", "meanII", "meanQQ", "meanIQ")
AMPS = (3e-4, 0.26, 60.0)
FLOOR = 2.0 ** -23
LENGTHS = (1, 15, 16, 17, 255 * 16 + 1, 4095, 4096, 4097, 8192 + 5, 40000)
MUTATIONS = ("inclusive", "no_pre", "total3", "stale_total", "ignore_n", "clamp", "slot5")
MUTATION_TEXT = {
    "inclusive": "every thread starts from its inclusive prefix",
    "no_pre": "`pre` dropped: waves 1..3 start from the tile's state",
    "total3": "`total` composed of three wave totals",
    "stale_total": "a filter's tile end state taken with the total of the scan before it (meanQ with I's, meanII with Q's, ...)",
    "ignore_n": "`k < n` ignored in the composition: the zero filler is filtered in",
    "clamp": "the ring wrap replaced by a clamp to ring_len - 1",
    "slot5": "state slot 8 s replaced by 5 s",
}


# ------------------------------------------------------------------------------------------------------------------ references
def _oracle_run(fn, dtype, data, tos, mode):
    """one stream through the oracle's serial filter, piece by piece -> (outputs complex64, state after every piece [len(tos), 5])"""
    out = np.ascontiguousarray(data[:tos[-1] if len(tos) else 0]).astype(np.complex64).copy()
    st = np.array(INIT, dtype)
    states, pos = [], 0
    for to in tos:
        if to > pos:
            piece = np.ascontiguousarray(out[pos:to])
            fn(piece, to - pos, mode, st)
            out[pos:to] = piece
            pos = to
        states.append(st.copy())
    return out, np.array(states).reshape(len(tos), 5)


def run_reference(data, tos, mode, which="f64"):
    L = ol.oracle()
    if which == "f64":
        return _oracle_run(L.ora_dciq_buffer_f64, np.float64, data, tos, mode)
    return _oracle_run(L.ora_dciq_buffer, np.float32, data, tos, mode)


def _pole(x, y0):
    """y_n = y_{n-1} + a (x_n - y_{n-1}) for n = 1..N in closed form (float64; (1 - a)^-n < e for n up to 2 M)"""
    a = float(ALPHA)
    n = np.arange(1, len(x) + 1, dtype=np.float64)
    d = np.exp(n * np.log1p(-a))
    return d * (y0 + a * np.cumsum(x / d))


def closed_form(data, mode, st0=INIT):
    """The whole stream at once -> (outputs complex128, unrounded; end state [5])."""
    v = np.asarray(data, np.complex64)
    vi, vq = v.real.astype(np.float64), v.imag.astype(np.float64)
    mI, mQ = _pole(vi, st0[0]), _pole(vq, st0[1])
    xi, xq = vi - mI, vq - mQ
    st = list(st0)
    if len(v):
        st[0], st[1] = mI[-1], mQ[-1]
    if mode != 2:
        return xi + 1j * xq, np.array(st)
    mII, mIQ = _pole(xi * xi, st0[2]), _pole(xi * xq, st0[4])
    with np.errstate(all="ignore"):
        xc = xq - mIQ / mII * xi
        mQQ = _pole(xc * xc, st0[3])
        out = xi + 1j * (xc * np.sqrt(mII / mQQ))
    if len(v):
        st[2], st[3], st[4] = mII[-1], mQQ[-1], mIQ[-1]
    return out, np.array(st)


# ------------------------------------------------------------------------------------------------------------------ restatement
def _then(fa, fb, ga, gb):
    """aff_then: g after f, maps kept as y -> y - e y + b"""
    return (fa + ga) - ga * fa, (fb - ga * fb) + gb


def _apply(fa, fb, y):
    return y + (fb - fa * y)


_LANE = np.arange(256) & 63
_K = np.arange(PER)


def _compose(x, valid, mut):
    fa, fb = np.zeros(256, F32), np.zeros(256, F32)
    ga = np.full(256, ALPHA, F32)
    for k in range(PER):
        na, nb = _then(fa, fb, ga, ALPHA * x[:, k])
        if mut == "ignore_n":
            fa, fb = na, nb
        else:
            fa, fb = np.where(valid[:, k], na, fa), np.where(valid[:, k], nb, fb)
    return fa, fb


def _scan(fa, fb, mut):
    """aff_block_exclusive -> (exclusive prefix per thread (a, b), total (a, b))"""
    ia, ib = fa.copy(), fb.copy()
    for o in (1, 2, 4, 8, 16, 32):
        na, nb = _then(np.roll(ia, o), np.roll(ib, o), ia, ib)              # __shfl_up; lanes below o keep their own (the guard)
        m = _LANE >= o
        ia, ib = np.where(m, na, ia), np.where(m, nb, ib)
    sa, sb = ia[63::64].copy(), ib[63::64].copy()                            # sh[w]
    pa, pb = np.zeros(4, F32), np.zeros(4, F32)
    for w in range(4):
        a, b = np.zeros(1, F32), np.zeros(1, F32)
        for q in range(w):
            a, b = _then(a, b, sa[q:q + 1], sb[q:q + 1])
        pa[w], pb[w] = a[0], b[0]
    if mut == "no_pre":
        pa[:], pb[:] = 0, 0
    ta, tb = _then(sa[0:1], sb[0:1], sa[1:2], sb[1:2])
    ta, tb = _then(ta, tb, sa[2:3], sb[2:3])
    if mut != "total3":
        ta, tb = _then(ta, tb, sa[3:4], sb[3:4])
    ea, eb = np.roll(ia, 1), np.roll(ib, 1)
    ea[_LANE == 0], eb[_LANE == 0] = 0, 0
    if mut == "inclusive":
        ea, eb = ia, ib
    ra, rb = _then(np.repeat(pa, 64), np.repeat(pb, 64), ea, eb)
    return ra, rb, ta[0], tb[0]


def _kernel(ri, rq, st, frm, to, mode, ring_len, mut):
    """k_dciq's block of one stream: ring (two float32 arrays) corrected in place over [frm, to), st [5] float32 updated."""
    meanI, meanQ, meanII, meanQQ, meanIQ = (F32(v) for v in st)
    stale = mut == "stale_total"
    for t0 in range(frm, to, TILE):
        mine = t0 + np.arange(256, dtype=np.int64) * PER
        n = np.clip(to - mine, 0, PER)
        valid = _K[None, :] < n[:, None]
        idx = (mine % ring_len)[:, None] + _K[None, :]
        idx = np.where(idx >= ring_len, ring_len - 1 if mut == "clamp" else idx - ring_len, idx)
        vi = np.where(valid, ri[idx], F32(0)).astype(F32)
        vq = np.where(valid, rq[idx], F32(0)).astype(F32)
        # ---- level 1
        fIa, fIb = _compose(vi, valid, mut)
        fQa, fQb = _compose(vq, valid, mut)
        ea, eb, tIa, tIb = _scan(fIa, fIb, mut)
        mI_end, mI = _apply(tIa, tIb, meanI), _apply(ea, eb, meanI)
        ea, eb, tQa, tQb = _scan(fQa, fQb, mut)
        mQ_end = _apply(tIa, tIb, meanQ) if stale else _apply(tQa, tQb, meanQ)
        mQ = _apply(ea, eb, meanQ)
        for k in range(PER):
            m = valid[:, k]
            mI = np.where(m, mI + ALPHA * (vi[:, k] - mI), mI)
            mQ = np.where(m, mQ + ALPHA * (vq[:, k] - mQ), mQ)
            vi[:, k] = np.where(m, vi[:, k] - mI, vi[:, k])
            vq[:, k] = np.where(m, vq[:, k] - mQ, vq[:, k])
        meanI, meanQ = mI_end, mQ_end
        if mode == 2:
            # ---- level 2
            ii, iq = vi * vi, vi * vq
            fa, fb = _compose(ii, valid, mut)
            ga, gb = _compose(iq, valid, mut)
            ea, eb, tIIa, tIIb = _scan(fa, fb, mut)
            mII_end = _apply(tQa, tQb, meanII) if stale else _apply(tIIa, tIIb, meanII)
            mII = _apply(ea, eb, meanII)
            ea, eb, tIQa, tIQb = _scan(ga, gb, mut)
            mIQ_end = _apply(tIIa, tIIb, meanIQ) if stale else _apply(tIQa, tIQb, meanIQ)
            mIQ = _apply(ea, eb, meanIQ)
            mIIk = np.zeros((256, PER), F32)
            for k in range(PER):
                m = valid[:, k]
                mII = np.where(m, mII + ALPHA * (ii[:, k] - mII), mII)
                mIQ = np.where(m, mIQ + ALPHA * (iq[:, k] - mIQ), mIQ)
                phi = mIQ / mII
                vq[:, k] = np.where(m, vq[:, k] - phi * vi[:, k], vq[:, k])
                mIIk[:, k] = mII
            meanII, meanIQ = mII_end, mIQ_end
            # ---- level 3
            qq = vq * vq
            fa, fb = _compose(qq, valid, mut)
            ea, eb, tQQa, tQQb = _scan(fa, fb, mut)
            mQQ_end = _apply(tIQa, tIQb, meanQQ) if stale else _apply(tQQa, tQQb, meanQQ)
            mQQ = _apply(ea, eb, meanQQ)
            for k in range(PER):
                m = valid[:, k]
                mQQ = np.where(m, mQQ + ALPHA * (qq[:, k] - mQQ), mQQ)
                vq[:, k] = np.where(m, vq[:, k] * np.sqrt(mIIk[:, k] / mQQ), vq[:, k])
            meanQQ = mQQ_end
        ri[idx[valid]], rq[idx[valid]] = vi[valid], vq[valid]
    st[:] = (meanI, meanQ, meanII, meanQQ, meanIQ)


def restate(data, groups, mode, ring_len=RING, mutation=None):
    """The engine's rings and state memory through the launch groups -> (out[s] complex64: every sample as the ring held it right after the
    launch that corrected it; states [group][s][5] float32, read at slot 8 s as dx.dciq_read does)."""
    n_s = len(data)
    ri, rq = [np.zeros(ring_len, F32) for _ in range(n_s)], [np.zeros(ring_len, F32) for _ in range(n_s)]
    mem = np.zeros(8 * n_s, F32)
    for s in range(n_s):
        mem[8 * s:8 * s + 5] = INIT
    stride = 5 if mutation == "slot5" else 8
    out = [np.zeros(int(sum(g[s] for g in groups)), np.complex64) for s in range(n_s)]
    done, states = [0] * n_s, []
    with np.errstate(all="ignore"):
        for g in groups:
            for s in range(n_s):
                if not g[s]:
                    continue
                frm, to = done[s], done[s] + int(g[s])
                where = np.arange(frm, to) % ring_len
                ri[s][where], rq[s][where] = data[s][frm:to].real, data[s][frm:to].imag          # the push (never mutated)
                _kernel(ri[s], rq[s], mem[stride * s:stride * s + 5], frm, to, mode, ring_len, mutation)
                out[s][frm:to] = ri[s][where] + 1j * rq[s][where]
                done[s] = to
            states.append(mem.reshape(n_s, 8)[:, :5].copy())
    return out, np.array(states)


# ------------------------------------------------------------------------------------------------------------------ bounds
def tos_of(groups, s):
    return [int(v) for v in np.cumsum([g[s] for g in groups])]


def distances(case, out, states):
    """Distance of (out, states) from the f64 reference, per stream: outputs absolute (max over the finite expected samples; inf where
    finiteness differs), each state relative to its own magnitude (max over the groups; an expected 0 has to be 0)."""
    res = []
    for s in range(S):
        want, wst = case["f64"][s]
        o = np.asarray(out[s])
        d_out = 0.0
        for a, b in ((o.real, want.real), (o.imag, want.imag)):
            fin = np.isfinite(b)
            if not np.array_equal(np.isfinite(a), fin):
                d_out = np.inf
            elif fin.any():
                d_out = max(d_out, float(np.abs(a[fin].astype(np.float64) - b[fin]).max()))
        d_st = np.zeros(5)
        got = np.asarray(states)[:, s, :].astype(np.float64)
        for j in range(5):
            for g in range(len(wst)):
                w, v = wst[g, j], got[g, j]
                if not np.isfinite(w):
                    d = 0.0 if np.isnan(v) == np.isnan(w) and not np.isfinite(v) else np.inf
                elif w == 0.0:
                    d = 0.0 if v == 0.0 else np.inf
                else:
                    d = abs(v - w) / abs(w) if np.isfinite(v) else np.inf
                d_st[j] = max(d_st[j], d)
        res.append({"out": d_out, "st": d_st})
    return res


def finish(case):
    """references, the restatement and the bounds of a case (cached in the case)"""
    if "bound" in case:
        return case
    data, groups, mode = case["data"], case["groups"], case["mode"]
    case["f64"] = [run_reference(data[s], tos_of(groups, s), mode, "f64") for s in range(S)]
    case["f32"] = [run_reference(data[s], tos_of(groups, s), mode, "f32") for s in range(S)]
    case["restated"] = restate(data, groups, mode)
    case["dist"] = distances(case, *case["restated"])
    case["ref_noise"] = distances(case, [c[0] for c in case["f32"]],
                                  np.stack([c[1] for c in case["f32"]], axis=1) if groups else np.zeros((0, S, 5)))
    case["bound"] = [{"out": max(4.0 * d["out"], FLOOR * case["A"]), "st": np.maximum(4.0 * d["st"], FLOOR)} for d in case["dist"]]
    return case


def ratios(case, out, states):
    """largest distance / bound per stream -> [(out ratio, [5 state ratios])]"""
    finish(case)
    return [(d["out"] / b["out"], d["st"] / b["st"]) for d, b in zip(distances(case, out, states), case["bound"])]


# ------------------------------------------------------------------------------------------------------------------ inputs
def _noise(rng, n, a, rms=1.0):
    return (a * rms * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0))


def _impair(x, gain, deg):
    ph = np.deg2rad(deg)
    return x.real + 1j * gain * (x.imag * np.cos(ph) + x.real * np.sin(ph))


def family(name, rng, n, a, step_at):
    """n samples of full scale a.  step_at: where a step family changes (the middle of a tile and of a thread of the stream's partition)."""
    x = _noise(rng, n, a, 0.3)
    if name == "noise_dc":
        x = x + a * (0.1 - 0.07j)
    elif name == "noise_dc09":
        x = 0.1 * x + a * (0.9 - 0.9j)
    elif name == "dc_step":
        x = 0.1 * x
        x[step_at:] += a * (0.9 + 0.9j)
    elif name == "impair_mild":
        x = _impair(x, 1.06, 3.0) + a * (0.1 - 0.07j)
    elif name == "impair_strong":
        x = _impair(x, 1.5, 20.0) + a * (0.1 - 0.07j)
    elif name == "i_zero":
        x = 1j * x.imag
    elif name == "q_zero":
        x = x.real + 0j
    elif name == "silence":
        x = np.zeros(n, np.complex128)
    elif name == "silence_then_signal":
        x[:step_at] = 0
    else:
        raise ValueError(name)
    return x.astype(np.complex64)


FAMILY_GROUPS = (("noise_dc", "dc_step", "impair_mild"), ("impair_strong", "i_zero", "q_zero"), ("silence", "silence_then_signal", "noise_dc09"))
_PIECES = (5000, 17, 4096, 1, 8197, 15, 4095, 16, 4097, 4081)


def interleave(parts):
    """per-stream lists of launch lengths -> launch groups with one busy stream each, the streams taking turns"""
    groups, k = [], 0
    while any(k < len(p) for p in parts):
        for s, p in enumerate(parts):
            if k < len(p):
                g = [0] * len(parts)
                g[s] = p[k]
                groups.append(tuple(g))
        k += 1
    return groups


def _step_place(pieces):
    """the middle of the second tile of the 8197-sample launch, 8 samples into thread 128"""
    at = 0
    for p in pieces:
        if p == 8197:
            return at + TILE + 128 * PER + 8
        at += p
    raise ValueError


def family_case(group, a, mode):
    names = FAMILY_GROUPS[group]
    rng = np.random.default_rng(1000 + 10 * group + mode)
    parts = [list(np.roll(_PIECES, 3 * s)) for s in range(S)]
    data = [family(names[s], rng, int(sum(parts[s])), a, _step_place(parts[s])) for s in range(S)]
    return {"name": "families_%d_A%g_m%d" % (group, a, mode), "mode": mode, "A": a, "data": data, "groups": interleave(parts),
            "families": names, "step_at": [_step_place(p) for p in parts]}


def partition_case(mode):
    """Every launch length of LENGTHS in every stream, in its own order; one busy stream per launch, and a run in which stream 2 alone is
    busy.  The 15- and 1-sample launches are placed so that the partly filled thread is reached at every n."""
    rng = np.random.default_rng(20 + mode)
    orders = ([16, 1, 4097, 15, 4081, 17, 4095, 8197, 4096, 40000], [4095, 17, 8197, 1, 16, 40000, 15, 4096, 4097, 4081],
              [40000, 15, 4096, 4081, 1, 8197, 16, 17, 4095, 4097])
    parts = [list(o) for o in orders]
    for p in parts:
        assert sorted(p) == sorted(LENGTHS)
    groups = interleave(parts)
    # ... then stream 2 alone, stream 0 idle: launches that end in a thread with n = 1 .. 15 samples, and one that ends on the wave boundary
    tail = [16 * 7 + n for n in range(1, 16)] + [64 * PER, 3 * 64 * PER]
    groups += [(0, 0, t) for t in tail]
    parts[2] += tail
    a = 0.26
    data = [(_noise(rng, int(sum(parts[s])), a, 1.0) + a * (0.03 - 0.02j) * (s + 1)).astype(np.complex64) for s in range(S)]
    return {"name": "partition_m%d" % mode, "mode": mode, "A": a, "data": data, "groups": groups}


# where the ring's boundary falls in the launch that crosses it: (name, samples in the ring before that launch, its length)
WRAPS_A = (("at_from", RING, 4097), ("thread_boundary", RING - 16 * 37, 4096), ("thread_offset_1", RING - 16 * 5 - 1, 4095))
WRAPS_B = (("thread_offset_15", RING - 16 * 200 - 15, 8197), ("last_partial_tile", RING - TILE - 500, TILE + 1000), ("short_launch", RING - 9, 17))


def wrap_case(which, mode):
    """Each stream is filled up to a chosen distance from the end of the two-frame ring (between the pushes the engine is stepped: an
    unlocked stream consumes a frame's worth per step), then ONE launch crosses the boundary, then one more follows it."""
    wraps = WRAPS_A if which == "a" else WRAPS_B
    rng = np.random.default_rng(40 + mode + (10 if which == "b" else 0))
    a = 0.26
    parts = []
    for _name, before, length in wraps:
        parts.append([TF - 1000, before - (TF - 1000), length, 4097])
    groups = []
    for k in range(4):
        for s in range(S):
            g = [0] * S
            g[s] = parts[s][k]
            groups.append(tuple(g))
    data = [(_noise(rng, int(sum(parts[s])), a, 1.0) + a * (0.5 - 0.4j)).astype(np.complex64) for s in range(S)]
    return {"name": "wrap_%s_m%d" % (which, mode), "mode": mode, "A": a, "data": data, "groups": groups, "wraps": wraps,
            "process_before": {3 * 1: 1, 3 * 2: 1}}          # group index -> dabx_process(1) calls in front of it


NAN_LAUNCH = 4                                                  # stream 1's third launch (8197 samples, piece index 2 of its order)


def isolation_case(mode, with_nan=True):
    """family group 0 at A = 0.26 with one NaN in stream 1: 7 samples into thread 5 of wave 2 of a launch's first tile"""
    c = family_case(0, 0.26, mode)
    parts1 = list(np.roll(_PIECES, 3))
    k_launch = parts1.index(8197)
    at = int(sum(parts1[:k_launch])) + 2 * 64 * PER + 5 * PER + 7
    c["name"] = "isolation_m%d%s" % (mode, "" if with_nan else "_clean")
    c["nan_at"] = at
    assert k_launch + 1 < len(parts1)
    if with_nan:
        c["data"][1] = c["data"][1].copy()
        c["data"][1][at] = np.complex64(complex(np.nan, np.nan))
    return c


ENTRY_GROUPS = ((5000, 0, 17), (4096, 4096, 4096), (0, 8197, 1), (15, 4081, 0), (1, 0, 4095), (4097, 16, 0), (40000, 40000, 40000), (0, 1, 8197))
ENTRY_PATHS = ("push", "commit", "slab", "slab_2500")


def entry_case(mode):
    """The same samples and launch ranges through dabx_push_iq, through ring pointer + dabx_commit_iq (a group with equal counts: one
    commit with stream = -1) and through a cf32 slab ingest (unequal counts per stream, 0 among them)."""
    rng = np.random.default_rng(60 + mode)
    a = 0.26
    n = [int(sum(g[s] for g in ENTRY_GROUPS)) for s in range(S)]
    data = [(_impair(_noise(rng, n[s], a, 1.0), 1.06, 3.0) + a * (0.1 - 0.07j) * (s + 1)).astype(np.complex64) for s in range(S)]
    return {"name": "entry_m%d" % mode, "mode": mode, "A": a, "data": data, "groups": list(ENTRY_GROUPS)}


# input samples per stream and commit of the 2.5 MS/s slab leg (whole 1-ms blocks of 2500; 0 among them, unequal)
RESAMPLED_COMMITS = ((5000, 0, 2500), (2500, 7500, 0), (0, 2500, 10000), (7500, 5000, 2500), (2500, 2500, 2500))


def resampled_payloads(mode):
    """int16 recordings at 2.5 MS/s, one per stream: noise of rms 0.26 with a DC and the mild impairment"""
    rng = np.random.default_rng(80 + mode)
    out = []
    for s in range(S):
        n = int(sum(c[s] for c in RESAMPLED_COMMITS))
        x = _impair(_noise(rng, n, 0.26, 1.0), 1.06, 3.0) + 0.26 * (0.1 - 0.07j) * (s + 1)
        pairs = np.ascontiguousarray(x.astype(np.complex64)).view(np.float32)
        out.append(np.clip(np.round(pairs * 32768.0), -32768, 32767).astype("<i2"))
    return out


def model_case(data, groups, mode, a=0.26, name="measured"):
    """a case from samples only known at run time (the resampled leg: what a twin engine without the correction holds in its ring)"""
    return finish({"name": name, "mode": mode, "A": a, "data": [np.ascontiguousarray(d, np.complex64) for d in data], "groups": list(groups)})


def all_cases():
    """(group name, builder) for every case of the GPU file; built on demand (the wrap cases hold 400 000 samples per stream)"""
    cases = []
    for mode in (1, 2):
        cases.append(("partition", lambda m=mode: partition_case(m)))
        for w in ("a", "b"):
            cases.append(("wrap", lambda m=mode, w=w: wrap_case(w, m)))
        for g in range(len(FAMILY_GROUPS)):
            for a in AMPS:
                cases.append(("families", lambda m=mode, g=g, a=a: family_case(g, a, m)))
        cases.append(("isolation", lambda m=mode: isolation_case(m)))
        cases.append(("entry", lambda m=mode: entry_case(m)))
    return cases


# ------------------------------------------------------------------------------------------------------------------ cover
def launch_ranges(groups, s):
    """[(from, to)] of the launches in which stream s is busy"""
    out, at = [], 0
    for g in groups:
        if g[s]:
            out.append((at, at + int(g[s])))
            at += int(g[s])
    return out


def cover_of(groups):
    """what the launches of a case reach: lengths, n of the partly filled thread, ends on a wave boundary, idle patterns"""
    lengths, partial, wave_end, idle = set(), set(), 0, set()
    for g in groups:
        idle.add(tuple(int(v > 0) for v in g))
    for s in range(len(groups[0])):
        for frm, to in launch_ranges(groups, s):
            n = to - frm
            lengths.add(n)
            if n % PER:
                partial.add(n % PER)
            elif (n % TILE) // PER in (64, 128, 192):
                wave_end += 1
    return {"lengths": lengths, "partial_n": partial, "wave_boundary_ends": wave_end, "busy_patterns": idle}


def wrap_place(before, length, ring_len=RING):
    """where ring_len falls in the launch [before, before + length): (tile, thread, offset in the thread's 16, samples in that tile)"""
    assert before <= ring_len < before + length
    d = ring_len - before
    tile = d // TILE
    return tile, (d % TILE) // PER, d % PER, min(TILE, length - tile * TILE)
