"""GPU end-to-end parity: the stream-batched engine vs the CPU oracle receiver on the same IQ.

Bar (BASELINE.json / SURVEY.md 8d): FIB bytes + CRC flags, MSC logical-frame bytes and RS-corrected
super frames are BIT-EXACT; the float soft bits are compared by tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_lib as ol
from stage_driver import kernel_launches
from dabstar_amd import lib as dx

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

pytestmark = pytest.mark.gpu


def _engine_run(x, subch, n_frames, lcd=False, **kw):
    eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=max(1, len(subch)), out_frames=4, **kw)
    if subch:
        eng.set_subchannels(subch)
    if lcd:
        eng.set_lcd_statistics(1)        # the demapper instances that advance the LCD record's MER too (dabx_set_lcd_statistics)
    eng.push_iq(0, x)
    fibs, crc, msc, sfs, starts, fbbs = [], [], [[] for _ in subch], [[] for _ in subch], [], []
    eng.scalars = dict(clock_err=[], fic_ratio=[], snr_db=[], mer_db=[])       # per frame, as they stand when the frame is complete
    last_sf = [0] * len(subch)
    for step in range(n_frames + 3):
        before = eng.stats(0)["frames"]
        eng.process(1)
        st = eng.stats(0)
        if st["frames"] == before:
            continue
        f, c = eng.read_fibs(0, 1)
        fibs.append(f[0]); crc.append(c[0]); starts.append(st["last_start_index"]); fbbs.append(st["freq_offs_bb_hz"])
        eng.scalars["clock_err"].append(st["clock_err_hz"]); eng.scalars["fic_ratio"].append(st["fic_ratio_percent"])
        eng.scalars["snr_db"].append(st["snr_db_est"]); eng.scalars["mer_db"].append(st["mer_db_est"])
        for j in range(len(subch)):
            m = eng.read_msc(0, j, 4)
            msc[j].append((st["frames"], m))
    return eng, np.array(fibs), np.array(crc), msc, np.array(starts), np.array(fbbs)


def _check_frame_scalars(eng, fbbs, ora, n):
    """The per-frame receiver scalars that steer the NEXT frame (NCO frequency, clock-error phase ramp of the demapper,
    coarse-CFO enable) and the SNR estimate, against the oracle's values at the same point of the same frame.
    Tolerances: f_bb 0.05 Hz (float atan2 of a 37800-term correlation sum; one carrier is 1000 Hz, the NCO uses round(f_bb));
    clock error: same integer sample count through the same float expression -> equal; FIC ratio: integer -> equal;
    SNR: 0.02 dB (mMeanPowerOvrAll is a 115 200-step serial float recurrence in the reference, a weighted sum here)."""
    assert np.abs(np.asarray(fbbs[:n], np.float64) - ora["fbb_end"][:n]).max() <= 0.05
    assert np.array_equal(np.asarray(eng.scalars["clock_err"][:n], np.float32), ora["clock_err"][:n])
    assert np.array_equal(np.asarray(eng.scalars["fic_ratio"][:n]), ora["fic_ratio"][:n])
    a, b = np.asarray(eng.scalars["snr_db"][:n], np.float64), ora["snr_db"][:n].astype(np.float64)
    ok = np.isfinite(a) & np.isfinite(b)                       # an all-zero stretch (drop-out) makes 0/0 on both sides alike
    assert np.array_equal(np.isnan(a), np.isnan(b)) and ok.sum() >= n - 3 and np.abs(a[ok] - b[ok]).max() <= 0.02
    # MER of the same record (ofdm_decoder.cpp:204-208, 331-340): 0.02 dB where the engine tracks it (dabx_set_lcd_statistics), 0 where not
    m = np.asarray(eng.scalars.get("mer_db", [])[:n], np.float64)
    if m.size and np.nan_to_num(m, nan=1.0, posinf=1.0, neginf=1.0).any():
        w = ora["mer_db"][:n].astype(np.float64)
        ok = np.isfinite(m) & np.isfinite(w)                   # (a frame of zeros: 0 / 0 on both sides alike)
        assert ok.sum() >= n - 3 and np.array_equal(np.isfinite(m), np.isfinite(w)) and np.abs(m[ok] - w[ok]).max() <= 0.02, (m, w)


@pytest.mark.parametrize("seed,snr,cfo,toff", [(1, 20.0, 1234.5, 50000), (2, 12.0, -1987.0, 170001), (3, 30.0, 0.0, 3),
                                               (4, 18.0, 17350.0, 120000), (5, 15.0, -33100.0, 777)])   # coarse CFO: 17 and -33 carriers
def test_fic_and_msc_bit_exact_vs_oracle(seed, snr, cfo, toff):
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=seed)
    n_total = 28 * ds.TF
    x = ds.channel(ens.iq, snr_db=snr, cfo_hz=cfo, timing_offset=toff, seed=seed, n_out=n_total)
    ora = ol.oracle_run(x, subch)
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"], lcd=seed in (2, 4))
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 20
    assert bool(np.any(eng.scalars["mer_db"])) == (seed in (2, 4))        # off by default: the record then says 0
    if seed in (2, 4):
        assert snr - 3.0 < eng.scalars["mer_db"][n - 1] < snr + 3.0
    assert np.array_equal(starts[:n], ora["start"][:n])
    assert np.array_equal(crc[:n], ora["crc"][:n])
    assert np.array_equal(fibs[:n], ora["fibs"][:n])
    assert crc[6:n].all()                                      # locked and error free after the CFO has converged
    _check_frame_scalars(eng, fbbs, ora, n)
    assert snr - 1.0 < eng.scalars["snr_db"][n - 1] < snr + 9.0               # settling towards the channel's SNR (the noise IIR takes ~20 frames)
    # MSC logical frames: the engine ring keeps the newest 16 per sub-channel; the oracle kept the whole stream
    cnt = eng.counters()
    st = eng.stats(0)
    frames_done = st["frames"]
    k = frames_done * 4 - 16                                   # logical frames decoded per sub-channel (16-CIF warm-up)
    assert cnt["cifs_decoded"] == 18 * k
    total_sf = st["sf_ok"] // 18
    assert st["sf_ok"] == 18 * total_sf and st["sf_fail"] == 0 and total_sf >= 3
    for j in range(18):
        o = ora["msc"][j].reshape(-1, 192)
        got = eng.read_msc(0, j, 16)
        assert len(got) == 16 and np.array_equal(got, o[k - 16:k]), j
        sf_o = ora["sf"][j].reshape(-1, 880)
        got_sf = eng.read_superframes(0, j, 4)
        assert len(got_sf) == min(4, total_sf) and np.array_equal(got_sf, sf_o[total_sf - len(got_sf):total_sf]), j
        # ... and they are the transmitted super frames (cyclic ensemble of 8)
        assert any(np.array_equal(got_sf[-1], ens.superframes[j][q]) for q in range(8)), j
    # the oracle also pushes the CIFs of a final, partially read frame through its back ends: totals are
    # comparable only when both decoded the same number of logical frames
    if cnt["cifs_decoded"] == sum(x_["cif_out"] for x_ in ora["stats"]):
        assert cnt["sf_ok"] == sum(x_["sf_ok"] for x_ in ora["stats"])
        assert cnt["au_ok"] == sum(x_["au_ok"] for x_ in ora["stats"])
        assert cnt["rs_corrected"] == sum(x_["rs_corr"] for x_ in ora["stats"])
        assert cnt["au_bad"] == sum(x_["au_bad"] for x_ in ora["stats"])
    eng.close()


@pytest.mark.parametrize("profile,doppler,snr,ppm,drift", [("TU6", 20.0, 18.0, 0.0, 0.0), ("RA4", 60.0, 20.0, 0.0, 0.0),
                                                          ("SFN2", 40.0, 16.0, 8.0, 4.0), ("TU6", 100.0, 25.0, -15.0, 0.0)])
def test_mobile_channels_follow_the_oracle(profile, doppler, snr, ppm, drift):
    """Time-variant channels (tools/dab_synth.py::channel_mobile: COST-207 tap sets, every tap a Rayleigh process with Jakes
    Doppler spectrum, a sample clock that is off and drifts): the stand-in for recordings made in a moving car, which the
    reference does not ship.  What they exercise and static channels do not: the PRS correlation peak wanders and fades
    (phasereference.cpp:87-213: start indices move by several samples from frame to frame, first-peak picking on a changing
    impulse response), the per-carrier IIRs of the demapper chase a moving channel (ofdm_decoder.cpp:197-223), FIBs fail in
    fades, RS has real work.  The engine must walk every frame like the oracle: start indices, CRC flags, every FIB that
    passes its CRC, the per-frame scalars, and the MSC logical frames / super frames / RS counters of every sub-channel."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=33)
    x = ds.channel_mobile(ens.iq, profile, doppler_hz=doppler, snr_db=snr, cfo_hz=-520.0, timing_offset=9000, seed=33,
                          n_out=30 * ds.TF, clock_ppm=ppm, clock_drift_ppm_per_s=drift)
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=18, out_frames=4)
    eng.set_subchannels(subch)
    if profile == "TU6":
        eng.set_lcd_statistics(1)          # the MER's IIR through fades and (where a fade costs the lock) demapper resets
    eng.push_iq(0, x)
    fibs, crc, starts, fbbs, idle, steps = [], [], [], [], 0, 0
    eng.scalars = dict(clock_err=[], fic_ratio=[], snr_db=[], mer_db=[])
    while idle < 4 and steps < 400:                                # a fade may cost the lock: acquisition passes are steps without a frame
        before = eng.stats(0)
        eng.process(1)
        st = eng.stats(0)
        steps += 1
        idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
        if st["frames"] > before["frames"]:
            f, c = eng.read_fibs(0, 1)
            fibs.append(f[0]); crc.append(c[0]); starts.append(st["last_start_index"]); fbbs.append(st["freq_offs_bb_hz"])
            eng.scalars["clock_err"].append(st["clock_err_hz"]); eng.scalars["fic_ratio"].append(st["fic_ratio_percent"])
            eng.scalars["snr_db"].append(st["snr_db_est"]); eng.scalars["mer_db"].append(st["mer_db_est"])
    fibs, crc, starts, fbbs = np.array(fibs), np.array(crc), np.array(starts), np.array(fbbs)
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 24, (len(fibs), ora["n"], steps)
    assert np.array_equal(starts[:n], ora["start"][:n])
    assert len(set(starts[8:n].tolist())) >= 3                     # the channel does move the timing
    assert np.array_equal(crc[:n], ora["crc"][:n])
    ok = ora["crc"][:n].astype(bool)
    assert ok[8:].mean() > 0.6 and np.array_equal(fibs[:n][ok], ora["fibs"][:n][ok])
    if doppler >= 60.0:
        assert not ok[8:].all()                                    # FIBs do fail in the fades of the fast channels
    assert (fibs[:n][~ok] != ora["fibs"][:n][~ok]).any(axis=1).sum() <= 2      # garbage FIBs: the float demapper is equal within 1 LSB, not bit for bit
    _check_frame_scalars(eng, fbbs, ora, n)
    st = eng.stats(0)
    k = st["frames"] * 4 - 16
    same_len = all(o_["cif_out"] == k for o_ in ora["stats"])
    for j in range(18):
        o = ora["msc"][j].reshape(-1, 192)
        assert np.array_equal(eng.read_msc(0, j, 32), o[k - 32:k]), j
        sub = eng.subch_stats(0, j)
        o_sf = ora["sf"][j].reshape(-1, 880)
        q = min(4, sub["sf_ok"])
        assert q >= 3 and np.array_equal(eng.read_superframes(0, j, q), o_sf[sub["sf_ok"] - q:sub["sf_ok"]]), j
        if same_len:
            for a_, b_ in (("sf_ok", "sf_ok"), ("sf_fail", "sf_fail"), ("rs_corrected", "rs_corr"), ("rs_failed", "rs_fail"),
                           ("au_ok", "au_ok"), ("au_bad", "au_bad")):
                assert sub[a_] == ora["stats"][j][b_], (j, a_)
    if doppler >= 40.0:
        assert st["rs_corrected"] > 0                              # the RS stage corrected real errors
    eng.close()


@pytest.mark.parametrize("gain", [3.0e-4, 60.0])
def test_input_level_extremes_follow_the_oracle(gain):
    """The path is scale-free except for the noise-power floor (1/32767)^2 of the null-symbol estimate
    (ofdm_decoder.cpp:114-130) and the soft-bit truncation: a very weak and a very strong input (-70 dB / +36 dB
    relative to the usual level) must still give the oracle's bytes."""
    subch = ds.default_subchannels(6, 64)
    ens = ds.build_ensemble(10, subch, seed=15)
    x = (ds.channel(ens.iq, snr_db=17.0, cfo_hz=610.0, timing_offset=33333, seed=15, n_out=22 * ds.TF) * np.float32(gain)).astype(np.complex64)
    ora = ol.oracle_run(x, subch)
    # the level tracker starts at 0.1 (sample_reader.h:95): a weak input spends its first frames in failed acquisition
    # attempts while the level decays, each of them one engine step
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"] + 12)
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 16
    assert np.array_equal(starts[:n], ora["start"][:n])
    assert np.array_equal(crc[:n], ora["crc"][:n]) and np.array_equal(fibs[:n], ora["fibs"][:n])
    assert crc[6:n].all()
    k = eng.stats(0)["frames"] * 4 - 16
    for j in range(len(subch)):
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, 192)[k - 16:k]), j
    eng.close()


@pytest.mark.parametrize("strongest", [0, 1])
def test_multipath_channel_follows_the_oracle(strongest):
    """Two echoes (+37 and +210 samples, -4 and -9 dB, rotated) inside the guard interval: several correlation peaks for
    the first-peak / strongest-peak selection (phasereference.cpp:136-212), frequency-selective carriers for the demapper."""
    subch = ds.default_subchannels(9, 64)
    ens = ds.build_ensemble(10, subch, seed=61)
    x = ds.channel(ens.iq, snr_db=19.0, cfo_hz=-455.0, timing_offset=101010, seed=61, n_out=24 * ds.TF)
    y = x.copy()
    y[37:] += np.complex64(0.63 * np.exp(1j * 1.1)) * x[:-37]
    y[210:] += np.complex64(0.35 * np.exp(-1j * 2.3)) * x[:-210]
    y = y.astype(np.complex64)
    cfg = (3.0, strongest, 1)
    ora = ol.oracle_run(y, subch, config=cfg)
    eng, fibs, crc, msc, starts, fbbs = _engine_run(y, subch, ora["n"], sync_threshold=cfg[0], sync_strongest=bool(strongest))
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 18
    assert np.array_equal(starts[:n], ora["start"][:n])
    assert np.array_equal(crc[:n], ora["crc"][:n]) and np.array_equal(fibs[:n], ora["fibs"][:n])
    assert crc[6:n].all()
    k = eng.stats(0)["frames"] * 4 - 16
    for j in range(len(subch)):
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, 192)[k - 16:k]), j
    eng.close()


def test_arbitrary_push_sizes_give_the_same_result():
    """IDeviceHandler::getSamples hands over whatever the device has: the stream pushed in random pieces (1 .. 300 000
    samples) with a dabx_process call after each, through a ring of only 3 frames, must decode exactly like the same
    stream pushed at once."""
    subch = ds.default_subchannels(5, 64)
    ens = ds.build_ensemble(10, subch, seed=71)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=1500.0, timing_offset=5555, seed=71, n_out=21 * ds.TF)
    ref, fibs_ref, crc_ref, _, starts_ref, _ = _engine_run(x, subch, 21)
    rng = np.random.default_rng(5)
    eng = dx.Engine(n_streams=1, ring_frames=3, max_subch=len(subch), out_frames=4)
    eng.set_subchannels(subch)
    pos, fibs, crc = 0, [], []
    while pos < len(x):
        n = int(min(len(x) - pos, rng.choice([1, 7, 1000, 50021, 196608, 300000])))
        eng.push_iq(0, x[pos:pos + n])
        pos += n
        while True:
            before = eng.stats(0)["frames"]
            eng.process(1)
            if eng.stats(0)["frames"] == before:
                break
            f, c = eng.read_fibs(0, 1)
            fibs.append(f[0]); crc.append(c[0])
    a, b = eng.stats(0), ref.stats(0)
    for key in ("frames", "samples_consumed", "fib_ok", "sf_ok", "sf_fail", "rs_corrected", "au_ok", "cifs_decoded", "last_start_index"):
        assert a[key] == b[key], (key, a[key], b[key])
    assert np.array_equal(np.array(fibs), fibs_ref[:len(fibs)]) and np.array_equal(np.array(crc), crc_ref[:len(crc)])
    for j in range(len(subch)):
        assert np.array_equal(eng.read_msc(0, j, 16), ref.read_msc(0, j, 16)), j
        assert np.array_equal(eng.read_superframes(0, j, 2), ref.read_superframes(0, j, 2)), j
    eng.close(); ref.close()


def test_soft_bits_within_tolerance_and_transmitted_data_recovered():
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=7)
    x = ds.channel(ens.iq, snr_db=20.0, cfo_hz=-433.0, timing_offset=1000, seed=7, n_out=14 * ds.TF)
    ora = ol.oracle_run(x, subch, want_soft=True)
    eng = dx.Engine(n_streams=1, ring_frames=15, max_subch=18, capture_soft=True)
    eng.set_subchannels(subch)
    eng.push_iq(0, x)
    done = 0
    for _ in range(ora["n"] + 3):
        eng.process(1)
        fr = eng.stats(0)["frames"]
        if fr > done:
            done = fr
            if done in (1, 6, 12):
                got = eng.read_soft(0).astype(np.int32)
                exp = ora["soft"][done - 1].astype(np.int32)
                d = np.abs(got - exp)
                # 1 Hz steps of round(f_bb) can differ between the two float pipelines while the loop converges,
                # so the tight bound is asserted once it has settled; signs must agree wherever |soft| > 8.
                if done >= 6:          # measured (tools/soft_diff_stats.py): 2-4 soft bits in 1e5 differ, always by one LSB
                    assert d.max() <= 1 and (d > 0).mean() < 3e-4, (done, (d > 0).mean(), d.max())
                strong = np.abs(exp) > 8
                assert np.array_equal(got[strong] > 0, exp[strong] > 0)
    # transmitted FIBs recovered
    fibs, crc = eng.read_fibs(0, 1)
    assert crc.all()
    assert any(np.array_equal(fibs[0], ens.fibs[f]) for f in range(10))
    eng.close()


def test_fic_decode_stage_matches_oracle():
    rng = np.random.default_rng(3)
    ens = ds.build_ensemble(5, seed=9)
    soft = ((ens.tx_bits[:4, :3].reshape(4, 9216).astype(np.int16) * 2 - 1) * 70)
    soft = (soft + rng.normal(0, 45, soft.shape)).astype(np.int16)
    soft[3] = rng.integers(-100, 100, 9216)                 # garbage -> CRC failures, still identical
    fibs, crc = dx.fic_decode(soft)
    L = ol.oracle()
    for b in range(4):
        fic = (C.c_uint8 * 40000)()                          # ora_fic is < 40 kB
        L.ora_fic_init(fic)
        for sidx in range(3):
            L.ora_fic_process_block(fic, np.ascontiguousarray(soft[b, sidx * 3072:(sidx + 1) * 3072]), sidx + 1)
        # fib_bits live at a fixed offset: recompute through the public capture instead
        exp_bits = np.zeros((4, 768), np.uint8)
        n_in, m = ol.ora_fic_map()
        prbs = np.zeros(768, np.uint8); L.ora_prbs(prbs, 768)
        for g in range(4):
            blk = np.zeros(3096, np.int16)
            blk[m >= 0] = soft[b, g * 2304:(g + 1) * 2304][m[m >= 0]]
            exp_bits[g] = ol.ora_viterbi(blk, 768) ^ prbs
        exp_fibs = np.packbits(exp_bits.reshape(12, 256), axis=1)
        exp_crc = np.array([L.ora_check_crc_bits(np.ascontiguousarray(exp_bits.reshape(12, 256)[i]), 256) for i in range(12)], np.uint8)
        assert np.array_equal(fibs[b], exp_fibs) and np.array_equal(crc[b], exp_crc), b
    assert crc[:3].all() and not crc[3].any()
    assert np.array_equal(fibs[0], ens.fibs[0])


@pytest.mark.parametrize("snr", [18.0, 4.2])
def test_many_streams_fast_msc_path_matches_single_stream_path(snr):
    """Lane-per-trellis MSC decoder (vit_t.hip, uniform configuration) vs the wave-per-trellis kernel:
    same IQ through a 24-stream engine forced onto the fast path and through single-stream engines."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=21)
    n_streams, n_frames = 24, 26
    xs = [ds.channel(ens.iq, snr_db=snr, cfo_hz=200.0 * (s - 12), timing_offset=7919 * s + 11, seed=100 + s,
                     n_out=(n_frames + 3) * ds.TF) for s in range(n_streams)]
    eng = dx.Engine(n_streams=n_streams, ring_frames=n_frames + 4, max_subch=18, msc_fast_min_jobs=1024)
    eng.set_subchannels(subch)
    for s in range(n_streams):
        eng.push_iq(s, xs[s])
    eng.process(n_frames)          # 6 batches of 4 frames + one of 2
    for s in (0, 7, 23):
        ref = dx.Engine(n_streams=1, ring_frames=n_frames + 4, max_subch=18)
        ref.set_subchannels(subch)
        ref.push_iq(0, xs[s])
        ref.process(n_frames)
        a, b = eng.stats(s), ref.stats(0)
        for key in ("frames", "fib_ok", "sf_ok", "sf_fail", "rs_corrected", "rs_failed", "au_ok", "au_bad", "cifs_decoded", "last_start_index"):
            assert a[key] == b[key], (s, key, a[key], b[key])
        assert a["frames"] >= n_frames - 2 and a["sf_ok"] > 0
        for j in (0, 9, 17):
            assert np.array_equal(eng.read_msc(s, j, 32), ref.read_msc(0, j, 32)), (s, j)
            assert np.array_equal(eng.read_superframes(s, j, 4), ref.read_superframes(0, j, 4)), (s, j)
        ref.close()
    eng.close()


def test_lcd_mer_in_the_many_stream_schedule_and_in_the_delivered_record():
    """dabx_set_lcd_statistics on an engine of 48 streams (two demapper launches per frame, the per-carrier IIR handed from one to the other
    through HBM like the rest of the state): the MER after every frame against the oracle's (0.02 dB), the FIBs untouched by the switch, the
    delivered stream record carrying the float dabx_get_stats shows for this frame or (the MSC symbols' demapper runs on a HIP stream of its
    own, the record is gathered behind the frame chain) for the one before; a fresh engine says 0."""
    ens = ds.build_ensemble(10, [], seed=9)
    n_streams, n_frames = 48, 12
    xs = {s: ds.channel(ens.iq, snr_db=14.0 + 0.25 * s, cfo_hz=-800.0 + 30.0 * s, timing_offset=1000 + 4099 * s, seed=500 + s,
                        n_out=(n_frames + 2) * ds.TF) for s in (0, 17, 47)}
    ora = {s: ol.oracle_run(xs[s], []) for s in xs}
    eng = dx.Engine(n_streams=n_streams, ring_frames=n_frames + 3, max_subch=1, out_frames=8, fic_only=True)
    assert eng.stats(0)["mer_db_est"] == 0.0
    eng.set_lcd_statistics(1)
    for s in range(n_streams):
        eng.push_iq(s, xs[s if s in xs else 0])
    eng.delivery_open(slots=4, what=1)
    got = {s: [] for s in xs}
    prev = {s: 0.0 for s in xs}
    done = 0
    while done < n_frames:
        eng.process(1)
        eng.synchronize()
        st = {s: eng.stats(s) for s in xs}
        ch = eng.delivery_next(wait=True)
        for s in xs:
            if int(ch.streams[s]["n_frames"]):
                got[s].append(st[s]["mer_db_est"])
                assert np.float32(ch.streams[s]["mer_db_est"]) in (np.float32(st[s]["mer_db_est"]), np.float32(prev[s])), s
                prev[s] = st[s]["mer_db_est"]
        ch.release()
        done += 1
    eng.delivery_close()
    for s in xs:
        n = min(len(got[s]), ora[s]["n"])
        assert n >= n_frames - 3, (s, n)
        assert np.abs(np.asarray(got[s][:n], np.float64) - ora[s]["mer_db"][:n]).max() <= 0.02, (s, got[s][:n], ora[s]["mer_db"][:n])
        f, c = eng.read_fibs(s, 8)
        assert c.all() and np.array_equal(f[-1], ora[s]["fibs"][min(len(got[s]), ora[s]["n"]) - 1])
    eng.close()


@pytest.mark.parametrize("class_min", [1, 256])
def test_profile_classes_decode_mixed_and_per_stream_layouts_lane_per_trellis(class_min):
    """Lane-per-trellis MSC decoder on a population of DIFFERENT ensembles: the sub-channels of all streams are grouped
    into classes of equal protection profile (UEP, EEP-A, EEP-B, 32..128 kbit/s here), one launch decodes every class.
    class_min = 1: every class goes lane-per-trellis (no wave-per-trellis launch at all); class_min = 256: the small
    classes stay wave-per-trellis and both kernels share a batch.  Reference: single-stream engines on the
    wave-per-trellis kernel."""
    mixed, full = _mixed_subchannels(), ds.default_subchannels(18, 64)
    n_streams, n_frames = 10, 26
    cfgs = [full if s % 2 == 0 else mixed for s in range(n_streams)]
    ens = {id(full): ds.build_ensemble(10, full, seed=41), id(mixed): ds.build_ensemble(10, mixed, seed=42)}
    xs = [ds.channel(ens[id(cfgs[s])].iq, snr_db=15.0 + s, cfo_hz=150.0 * (s - 5), timing_offset=6151 * s + 5, seed=200 + s,
                     n_out=(n_frames + 3) * ds.TF) for s in range(n_streams)]
    eng = dx.Engine(n_streams=n_streams, ring_frames=n_frames + 4, max_subch=18, msc_fast_min_jobs=64, msc_class_min_jobs=class_min)
    for s in range(n_streams):
        eng.set_subchannels(cfgs[s], stream=s)
    for s in range(n_streams):
        eng.push_iq(s, xs[s])
    dx.check(dx.load().dabx_set_profiling(eng._h, 1))
    eng.process(n_frames)
    launches = kernel_launches(eng)
    dx.check(dx.load().dabx_set_profiling(eng._h, 0))
    assert launches["k_msc_vitT"] >= 4 and launches["k_msc_prep"] == launches["k_msc_vitT"]
    assert (launches["k_msc_frame"] == 0) == (class_min == 1), launches
    for s in (0, 1, 6, 9):
        ref = dx.Engine(n_streams=1, ring_frames=n_frames + 4, max_subch=18)
        ref.set_subchannels(cfgs[s])
        ref.push_iq(0, xs[s])
        ref.process(n_frames)
        a, b = eng.stats(s), ref.stats(0)
        for key in ("frames", "fib_ok", "sf_ok", "sf_fail", "rs_corrected", "rs_failed", "au_ok", "au_bad", "cifs_decoded", "last_start_index"):
            assert a[key] == b[key], (s, key, a[key], b[key])
        assert a["frames"] >= n_frames - 2 and a["sf_ok"] > 0
        eng.subch = list(cfgs[s])
        for j in range(len(cfgs[s])):
            assert np.array_equal(eng.read_msc(s, j, 32), ref.read_msc(0, j, 32)), (s, j)
            if cfgs[s][j].dab_plus:
                assert np.array_equal(eng.read_superframes(s, j, 4), ref.read_superframes(0, j, 4)), (s, j)
            assert eng.subch_stats(s, j) == ref.subch_stats(0, j), (s, j)
        ref.close()
    # reconfiguration rebuilds the classes: stream 1 switches to the uniform layout and keeps decoding
    eng.set_subchannels(full, stream=1)
    eng.close()


def test_more_profiles_than_decoder_classes():
    """8 streams with random layouts drawn from 26 protection profiles (EEP-A 1..4, EEP-B, UEP; 16..160 kbit/s): more
    distinct profiles than the lane-per-trellis decoder has classes (16), so the largest classes go lane-per-trellis and
    the rest wave-per-trellis within the same batch.  Every stream must equal a single-stream engine."""
    rng = np.random.default_rng(2024)
    pool = [(k, p, 0) for k in (16, 32, 48, 64, 96) for p in (0, 1, 2, 3)] + [(32, 4, 0), (64, 6, 0), (96, 5, 0), (160, 2, 0)] + \
           [(32, 2, 1), (64, 3, 1)]
    uep_mask = lambda k, l: (ol.ora_uep_map(k, l)[1] >= 0).astype(np.uint8)                 # noqa: E731
    n_streams, n_frames = 8, 24
    cfgs = []
    for s in range(n_streams):
        order = rng.permutation(len(pool))
        cu, lay = 0, []
        for i in order:
            k, p, sh = pool[i]
            size = (ol.ora_uep_map if sh else ol.ora_eep_map)(k, p)[0] // 64
            if cu + size > 864 or len(lay) == 9:
                continue
            lay.append(ds.SubCh(len(lay) + 1 + 8 * s % 50, cu, size, k, p, sh, mask=uep_mask(k, p) if sh else None))
            cu += size
        cfgs.append(lay)
    assert len({(c.kbps, c.prot_level, c.short_form) for lay in cfgs for c in lay}) > 16
    xs = [ds.channel(ds.build_ensemble(10, cfgs[s], seed=300 + s).iq, snr_db=22.0, cfo_hz=90.0 * s - 300, timing_offset=3001 * s + 17,
                     seed=400 + s, n_out=(n_frames + 3) * ds.TF) for s in range(n_streams)]
    eng = dx.Engine(n_streams=n_streams, ring_frames=n_frames + 4, max_subch=9, msc_fast_min_jobs=64, msc_class_min_jobs=1)
    for s in range(n_streams):
        eng.set_subchannels(cfgs[s], stream=s)
        eng.push_iq(s, xs[s])
    dx.check(dx.load().dabx_set_profiling(eng._h, 1))
    eng.process(n_frames)
    launches = kernel_launches(eng)
    dx.check(dx.load().dabx_set_profiling(eng._h, 0))
    assert launches["k_msc_vitT"] >= 4 and launches["k_msc_frame"] == launches["k_msc_vitT"], launches
    for s in range(n_streams):
        ref = dx.Engine(n_streams=1, ring_frames=n_frames + 4, max_subch=9)
        ref.set_subchannels(cfgs[s])
        ref.push_iq(0, xs[s])
        ref.process(n_frames)
        a, b = eng.stats(s), ref.stats(0)
        for key in ("frames", "fib_ok", "sf_ok", "sf_fail", "rs_corrected", "rs_failed", "au_ok", "au_bad", "cifs_decoded"):
            assert a[key] == b[key], (s, key, a[key], b[key])
        assert a["frames"] >= n_frames - 2 and a["sf_ok"] > 0, (s, a)
        eng.subch = list(cfgs[s])
        for j in range(len(cfgs[s])):
            assert np.array_equal(eng.read_msc(s, j, 32), ref.read_msc(0, j, 32)), (s, j)
            assert np.array_equal(eng.read_superframes(s, j, 4), ref.read_superframes(0, j, 4)), (s, j)
        ref.close()
    eng.close()


def test_two_engines_driven_from_two_threads():
    """A handle is thread-compatible (one caller at a time), different handles are independent: two engines decoding
    different ensembles from two host threads at once give what each gives alone (shared constant tables behind a mutex,
    per-thread error strings, separate HIP streams)."""
    import threading
    layouts = [ds.default_subchannels(18, 64), _mixed_subchannels()]
    xs = [ds.channel(ds.build_ensemble(10, lay, seed=140 + i).iq, snr_db=18.0, cfo_hz=-700.0 + 900 * i, timing_offset=4000 + 999 * i,
                     seed=140 + i, n_out=21 * ds.TF) for i, lay in enumerate(layouts)]

    def run(i, out):
        eng = dx.Engine(n_streams=1, ring_frames=22, max_subch=18, out_frames=4)
        eng.set_subchannels(layouts[i])
        eng.push_iq(0, xs[i])
        for _ in range(12):
            eng.process(2)
        eng.subch = list(layouts[i])
        out[i] = (eng.stats(0), eng.read_fibs(0, 4), [eng.read_msc(0, j, 16) for j in range(len(layouts[i]))])
        eng.close()

    alone, together = {}, {}
    for i in range(2):
        run(i, alone)
    th = [threading.Thread(target=run, args=(i, together)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(2):
        assert set(together) == {0, 1} and together[i][0] == alone[i][0] and alone[i][0]["frames"] >= 18
        assert np.array_equal(together[i][1][0], alone[i][1][0]) and np.array_equal(together[i][1][1], alone[i][1][1])
        for a, b in zip(together[i][2], alone[i][2]):
            assert np.array_equal(a, b)


def test_subchannels_discovered_from_the_decoded_fic_then_decoded():
    """no configuration from outside -- FIG 0/1 + 0/2 from the engine's own FIBs select the
    sub-channels (what FibDecoder hands DabRadio::set_audio_channel), which then decode cleanly."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=33)
    x = ds.channel(ens.iq, snr_db=20.0, cfo_hz=-321.0, timing_offset=4242, seed=9, n_out=20 * ds.TF)
    eng = dx.Engine(n_streams=1, ring_frames=21, max_subch=18, out_frames=4)
    eng.push_iq(0, x)
    eng.process(6)
    found = eng.discover_subchannels(0)
    assert [(f.subch_id, f.cu_start, f.cu_size, f.kbps, f.prot_level, f.short_form, f.dab_plus) for f in found] == \
           [(c.subch_id, c.cu_start, c.cu_size, 64, 2, 0, 1) for c in subch]
    eng.set_subchannels(found)
    eng.process(12)                 # 7 + 5 frames: the de-interleaver warm-up ends inside the first MSC batch
    st = eng.stats(0)
    assert st["sf_fail"] == 0 and st["sf_ok"] >= 18 and st["fib_ok"] >= st["fib_total"] - 24   # two settling frames, as in the oracle
    ref = ol.oracle_run(x, subch)
    for j in (0, 5, 17):
        sf = eng.read_superframes(0, j, 4)
        assert len(sf) == 4                                   # (48 - 16) logical frames -> 4..6 windows, ring read of 4
        osf = ref["sf"][j].reshape(-1, 880)
        for k in range(4):
            assert any(np.array_equal(sf[k], ens.superframes[j][q]) for q in range(8)), (j, k)
            assert any(np.array_equal(sf[k], o) for o in osf), (j, k)
    eng.close()


def test_eti_frames_carry_the_fic_and_the_logical_frames_of_each_cif():
    """dabx_read_eti (eti_generator.cpp:169-199): every emitted frame == the oracle's ETI assembly of that CIF's FIBs,
    FIG 0/0 counter and the oracle receiver's MSC bytes; frames are consecutive across calls."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=12, cif_start=240)          # CIF counter wraps 249 -> 0 inside the run
    x = ds.channel(ens.iq, snr_db=22.0, cfo_hz=77.0, timing_offset=2222, seed=4, n_out=22 * ds.TF)
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=23, max_subch=18, out_frames=8)
    eng.set_subchannels(subch)
    eng.push_iq(0, x)
    frames = []
    for chunk in (5, 7, 3, 6):
        eng.process(chunk)
        f, lost = eng.read_eti(0, 64)
        assert lost == 0
        frames.append(f)
    frames = np.concatenate(frames)
    n_frames = eng.stats(0)["frames"]
    assert len(frames) == 4 * n_frames - 16                               # one per CIF once the de-interleavers are filled
    descs = [dx.SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, 1, 0) for c in subch]
    fct = []
    for i, f in enumerate(frames):
        r = 16 + i                                                        # CIF index since lock
        F, k = divmod(r, 4)
        fib = ora["fibs"][F].reshape(-1)
        hi, lo = int(fib[4] & 0x1F), int(fib[5])                          # FIG 0/0 leads FIB 0 of every CIF in the synthetic
        for g in range(4):                                                # ensemble: the state after the frame is FIB 9's
            if ora["crc"][F][3 * g]:
                hi, lo = int(ora["fibs"][F][3 * g][4] & 0x1F), int(ora["fibs"][F][3 * g][5])
        msc = [ora["msc"][j].reshape(-1, 192)[r - 16] for j in range(18)]
        want, _ = ol.ora_eti_frame(hi, lo, k, descs, fib[96 * k:96 * k + 96], msc)
        assert np.array_equal(f, want), i
        fct.append(int(f[4]))
    assert len(set(fct)) >= 30 and min(fct) < 10 and max(fct) > 240    # FCT ran through the 249 -> 0 wrap
    eng.close()


def test_sixty_four_subchannels_discovered_decoded_and_packed_into_eti():
    """The most sub-channels an ensemble can carry (SubChId is 6 bits): 64 x 8 kbit/s EEP 3-A DAB+.  Discovery from the FIC
    (the FIG 0/1 / 0/2 description is spread over several FIBs and frames), decode of all 64 slots, per-slot counters and
    ETI frames with 64 stream-characterisation entries -- all equal to the oracle's."""
    subch = [ds.SubCh(i, 6 * i, 6, 8, 2, 0) for i in range(64)]
    ens = ds.build_ensemble(10, subch, seed=88)
    x = ds.channel(ens.iq, snr_db=18.0, cfo_hz=-120.0, timing_offset=1234, seed=88, n_out=22 * ds.TF)
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=23, max_subch=64, out_frames=8)
    eng.push_iq(0, x)
    eng.process(6)
    found = eng.discover_subchannels(0)                # in order of arrival: the rotation is entered wherever lock came
    assert sorted((f.subch_id, f.cu_start, f.cu_size, f.kbps, f.prot_level, f.short_form, f.dab_plus) for f in found) == \
           [(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, 1) for c in subch]
    eng.close()
    eng = dx.Engine(n_streams=1, ring_frames=23, max_subch=64, out_frames=8)
    eng.set_subchannels(subch)
    eng.push_iq(0, x)
    eng.process(ora["n"])
    frames, lost = eng.read_eti(0, 64)
    st = eng.stats(0)
    assert lost == 0 and st["frames"] >= ora["n"] - 1
    k = st["frames"] * 4 - 16
    for j in range(64):
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, 24)[k - 16:k]), j
        sub, o = eng.subch_stats(0, j), ora["stats"][j]
        if sub["cifs_decoded"] == o["cif_out"]:
            assert (sub["sf_ok"], sub["rs_corrected"], sub["au_ok"], sub["au_bad"]) == (o["sf_ok"], o["rs_corr"], o["au_ok"], o["au_bad"]), j
        assert sub["sf_ok"] >= 8, (j, sub)
    descs = [dx.SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, 1, 0) for c in subch]
    assert len(frames) == min(32, k)                                      # the rings keep the newest 32 CIFs (8 frames of FIBs)
    first = k - len(frames)                                               # index of the first logical frame returned
    for i in (0, 1, len(frames) - 1):
        r = 16 + first + i
        F, q = divmod(r, 4)
        fib = ora["fibs"][F].reshape(-1)
        hi, lo = int(fib[4] & 0x1F), int(fib[5])
        for g in range(4):
            if ora["crc"][F][3 * g]:
                hi, lo = int(ora["fibs"][F][3 * g][4] & 0x1F), int(ora["fibs"][F][3 * g][5])
        msc = [ora["msc"][j].reshape(-1, 24)[r - 16] for j in range(64)]
        want, _ = ol.ora_eti_frame(hi, lo, q, descs, fib[96 * q:96 * q + 96], msc)
        assert np.array_equal(frames[i], want), i
    eng.close()


def _mixed_subchannels():
    uep = lambda k, l: (ol.ora_uep_map(k, l)[1] >= 0).astype(np.uint8)                   # noqa: E731
    return [ds.SubCh(3, 0, 24, 32, 3, 1, mask=uep(32, 3), dab_plus=0),                   # UEP 32k level 3, MP2-style payload
            ds.SubCh(7, 30, 48, 32, 0, 0), ds.SubCh(12, 80, 128, 128, 1, 0),             # EEP 1-A, EEP 2-A
            ds.SubCh(20, 210, 54, 96, 6, 0), ds.SubCh(21, 270, 24, 48, 3, 0),            # EEP 3-B, EEP 4-A
            ds.SubCh(33, 300, 48, 64, 2, 0), ds.SubCh(40, 350, 54, 64, 4, 0),            # EEP 3-A, EEP 1-B
            ds.SubCh(63, 410, 116, 128, 2, 1, mask=uep(128, 2))]                         # UEP 128k level 2 carrying DAB+


def test_mixed_ensemble_uep_eep_a_b_bit_exact_and_discoverable():
    """Heterogeneous ensemble (UEP short form, EEP-A levels 1-4, EEP-B, 32..128 kbit/s, one non-DAB+ sub-channel):
    FIC-driven configuration, wave-per-trellis MSC kernel with per-sub-channel trellis lengths, DAB+ stage with
    4..16 RS code words per super frame -- all bit-exact vs the oracle receiver."""
    subch = _mixed_subchannels()
    ens = ds.build_ensemble(10, subch, seed=77)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=-840.0, timing_offset=91000, seed=6, n_out=24 * ds.TF)
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=25, max_subch=8, out_frames=4)
    eng.push_iq(0, x)
    eng.process(5)
    found = eng.discover_subchannels(0)
    assert [(f.subch_id, f.cu_start, f.cu_size, f.kbps, f.prot_level, f.short_form, f.dab_plus) for f in found] == \
           [(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, c.dab_plus) for c in subch]
    eng.close()
    # same configuration from the start, as the oracle has it
    eng = dx.Engine(n_streams=1, ring_frames=25, max_subch=8, out_frames=4)
    eng.set_subchannels(found)
    eng.push_iq(0, x)
    eng.process(ora["n"])
    st = eng.stats(0)
    assert st["frames"] >= ora["n"] - 1 and st["fib_ok"] >= st["fib_total"] - 36
    k = st["frames"] * 4 - 16
    for j, c in enumerate(subch):
        nb = 3 * c.kbps
        o = ora["msc"][j].reshape(-1, nb)
        got = eng.read_msc(0, j, 16)
        assert got.shape == (16, nb) and np.array_equal(got, o[k - 16:k]), j
        if c.dab_plus:                                                    # super frames incl. RS failure paths (sub-channel 7)
            sf_o = ora["sf"][j].reshape(-1, 110 * c.kbps // 8)
            got_sf = eng.read_superframes(0, j, 3)
            assert len(got_sf) == 3
            at = [i for i in range(len(sf_o) - 2) if np.array_equal(sf_o[i:i + 3], got_sf)]
            assert at and at[-1] >= len(sf_o) - 4, (j, at, len(sf_o))
    eng.close()


def test_adding_a_service_does_not_disturb_running_ones():
    """MscHandler::set_channel only adds a Backend (msc_handler.cpp:95-131): the slot that keeps its description decodes
    straight through; the new slot starts its own 16-CIF fill; an emptied slot (kbps = 0) stops."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=52)
    x = ds.channel(ens.iq, snr_db=21.0, cfo_hz=150.0, timing_offset=1234, seed=3, n_out=24 * ds.TF)
    ora = ol.oracle_run(x, subch)
    A, B = subch[4], subch[13]
    mk = lambda c: dx.SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, 1, 0)   # noqa: E731
    empty = dx.SubchDesc(0, 0, 0, 0, 0, 0, 0, 0)
    eng = dx.Engine(n_streams=1, ring_frames=25, max_subch=4, out_frames=4)
    eng.set_subchannels([mk(A)])
    eng.push_iq(0, x)
    eng.process(8)
    a0 = eng.subch_stats(0, 0)
    assert a0["cifs_decoded"] == 8 * 4 - 16 and a0["subch_id"] == A.subch_id
    eng.set_subchannels([mk(A), empty, mk(B)])                   # B goes to slot 2, slot 1 stays empty
    eng.process(9)
    a1, b1, e1 = eng.subch_stats(0, 0), eng.subch_stats(0, 2), eng.subch_stats(0, 1)
    assert a1["start_cif"] == a0["start_cif"] == 0 and a1["cifs_decoded"] == 17 * 4 - 16      # no restart, no gap
    assert b1["start_cif"] == 32 and b1["cifs_decoded"] == 9 * 4 - 16 and not e1["active"]
    eng.subch = [A, None, B]
    oa = ora["msc"][4].reshape(-1, 192)
    assert np.array_equal(eng.read_msc(0, 0, 32), oa[17 * 4 - 16 - 32:17 * 4 - 16])           # A: bit-exact across the change
    ob = ora["msc"][13].reshape(-1, 192)
    assert np.array_equal(eng.read_msc(0, 2, 20), ob[32:52])     # B's first logical frame is CIF 32 + 16 = the oracle's 33rd
    eng.set_subchannels([empty, empty, mk(B)])                   # stop A
    eng.process(3)
    a2, b2 = eng.subch_stats(0, 0), eng.subch_stats(0, 2)
    assert not a2["active"] and b2["cifs_decoded"] == 12 * 4 - 16 and b2["start_cif"] == 32
    eng.close()


def test_tii_null_symbols_are_accumulated_and_identified():
    """TII (dab_processor.cpp:273-300): the engine sums the FFTs of the TII null symbols on the GPU; dabx_read_tii runs the
    (reference-pinned) detector on the sum.  Same transmitters, strengths and counts as the detector fed by the oracle
    receiver's sum; the accumulator restarts after a read."""
    subch = ds.default_subchannels(18, 64)
    tx = [(12, 5, 1.0, True), (40, 17, 0.6, True), (63, 20, 0.5, False)]
    ens = ds.build_ensemble(10, subch, seed=61, tii=tx)
    x = ds.channel(ens.iq, snr_db=25.0, cfo_hz=60.0, timing_offset=3000, seed=2, n_out=23 * ds.TF)
    L = ol.oracle()
    rx = L.ora_rx_create(ol.make_descs(subch), len(subch))
    n = L.ora_rx_run(rx, x, len(x), 20)
    acc = np.zeros(2048, np.complex64)
    n_tii = L.ora_rx_take_tii(rx, acc)
    L.ora_rx_destroy(rx)
    det = dx.Tii()
    det.add(acc)
    want = det.process(6)
    det.close()
    assert n == 20 and n_tii >= 8
    assert {(m, c, e) for m, c, _, _, e in want} == {(12, 5, 0), (40, 17, 0), (63, 20, 1)}
    eng = dx.Engine(n_streams=1, ring_frames=24, max_subch=18, out_frames=4)
    eng.set_subchannels(subch)
    eng.push_iq(0, x)
    eng.process(12)
    none, k = eng.read_tii(0, min_frames=100)
    assert none == [] and 4 <= k <= 6                       # below min_frames: nothing consumed
    eng.process(8)
    got, k = eng.read_tii(0, min_frames=4, threshold_db=6)
    assert k == n_tii
    assert [(m, c, e) for m, c, _, _, e in got] == [(m, c, e) for m, c, _, _, e in want]
    for g, w in zip(got, want):
        assert abs(g[2] - w[2]) <= 2e-3 * w[2] and abs(((g[3] - w[3] + 180) % 360) - 180) < 0.5
    assert eng.read_tii(0, min_frames=1)[1] == 0            # accumulator was cleared by the read
    eng.close()


@pytest.mark.parametrize("acquire_mode", [1, 2])
@pytest.mark.parametrize("gap_kind", ["silence", "noise", "shifted"])
def test_loss_of_lock_and_reacquisition_follow_the_oracle(gap_kind, acquire_mode):
    """DabProcessor FSM (dab_processor.cpp:110-265): a drop-out in the middle of the stream -- PRS correlation fails, back to
    the null-dip search, demapper reset, coarse CFO again -- must be walked exactly like the oracle receiver walks it:
    same start indices, same FIB bytes / CRC flags frame by frame, same number of frames.  Both ways of running the search
    (dabx_config.acquire_mode: 1 in step on the front-end stream, 2 on its own HIP stream next to the steps) walk the same
    samples to the same decisions; only the step in which a frame appears differs."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=71)
    x = ds.channel(ens.iq, snr_db=18.0, cfo_hz=-1333.0, timing_offset=5555, seed=7, n_out=34 * ds.TF).copy()
    rng = np.random.default_rng(5)
    a, b = int(11.3 * ds.TF), int(13.1 * ds.TF)
    if gap_kind == "silence":
        x[a:b] = 0
    elif gap_kind == "noise":
        x[a:b] = ((rng.standard_normal(b - a) + 1j * rng.standard_normal(b - a)) * 0.2).astype(np.complex64)
    else:                                                   # the transmitter jumps: 0.37 frame of samples vanish
        x = np.concatenate([x[:a], x[a + int(0.37 * ds.TF):]])
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=18, out_frames=4, acquire_mode=acquire_mode)
    eng.set_subchannels(subch)
    if acquire_mode == 1:
        eng.set_lcd_statistics(1)          # OfdmDecoder::reset zeroes the MER's IIR with the rest (ofdm_decoder.cpp:92)
    eng.push_iq(0, x)
    fibs, crc, starts, fbbs, idle, steps = [], [], [], [], 0, 0
    eng.scalars = dict(clock_err=[], fic_ratio=[], snr_db=[], mer_db=[])
    while idle < 4 and steps < 400:                         # a step without a frame is an acquisition pass: keep going
        before = eng.stats(0)
        eng.process(1)
        st = eng.stats(0)
        steps += 1
        idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
        if st["frames"] > before["frames"]:
            f, c = eng.read_fibs(0, 1)
            fibs.append(f[0]); crc.append(c[0]); starts.append(st["last_start_index"]); fbbs.append(st["freq_offs_bb_hz"])
            eng.scalars["clock_err"].append(st["clock_err_hz"]); eng.scalars["fic_ratio"].append(st["fic_ratio_percent"])
            eng.scalars["snr_db"].append(st["snr_db_est"]); eng.scalars["mer_db"].append(st["mer_db_est"])
    fibs, crc, starts, fbbs = np.array(fibs), np.array(crc), np.array(starts), np.array(fbbs)
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 24, (len(fibs), ora["n"], steps)
    assert eng.counters()["sync_lost"] >= 1
    # The null-dip search after the loss compares against SampleReader's signal level, a per-sample IIR over every sample
    # ever read (sample_reader.cpp:246-248); the engine tracks it chunk by chunk in read order (k_frame_tail), close enough
    # for the search to stop at the very same sample.
    d = starts[:n].astype(int) - ora["start"][:n].astype(int)
    first_after = 11                                         # frames 0..10 precede the drop-out
    assert np.all(d == 0), (d, first_after)
    assert np.array_equal(crc[:n], ora["crc"][:n])
    assert np.array_equal(fibs[:n], ora["fibs"][:n])
    assert abs(fbbs[n - 1] - ora["fbb"][n - 1]) < 1.0 and abs(fbbs[n - 1] + 1333.0) < 2.0     # same CFO estimate at the end
    _check_frame_scalars(eng, fbbs, ora, n)                 # f_bb, clock error, FIC ratio, SNR: every frame, through the loss of lock
    assert crc[n - 6:n].all() and not crc[:n].all()         # locked again at the end
    if len(fibs) == ora["n"]:                               # the back ends ran straight through the drop-out on both sides
        k = 4 * ora["n"] - 16
        for j in (0, 8, 17):
            o = ora["msc"][j].reshape(-1, 192)
            if len(o) == k:
                assert np.array_equal(eng.read_msc(0, j, 24), o[k - 24:k]), j
    eng.close()


@pytest.mark.parametrize("gain", [0.25, 3e-4, 40.0])
def test_exact_level_tracker_is_bit_identical_to_the_oracle(gain):
    """dabx_config.exact_level_tracker = 1: SampleReader's level IIR (sample_reader.cpp:245-248, one float update per sample
    read) is run sample by sample in lock too.  Through acquisition, 10 locked frames, a drop-out, the null-dip search after it
    and re-acquisition, sLevel and peakLevel after every frame are BIT-IDENTICAL to the oracle's, at three input levels 100 dB
    apart.  The default (chunk-wise) tracker walks the same frames with the same start indices and stays within 1e-4
    relative of the exact level -- the reference's own SSE/AVX build does the same thing more coarsely (one update per
    get_samples call with alpha * n, sample_reader.cpp:170-176)."""
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=gain, seed=17, n_out=30 * ds.TF).copy()
    a, b = int(10.6 * ds.TF), int(12.2 * ds.TF)
    x[a:b] = 0                                                     # silence: the PRS correlation fails, back to the null-dip search
    ora = ol.oracle_run(x, subch)

    def run(exact):
        eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=4, out_frames=4, exact_level_tracker=exact)
        eng.set_subchannels(subch)
        eng.push_iq(0, x)
        lv, pk, starts, crc, idle, steps = [], [], [], [], 0, 0
        while idle < 4 and steps < 400:
            before = eng.stats(0)
            eng.process(1)
            st = eng.stats(0)
            steps += 1
            idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
            if st["frames"] > before["frames"]:
                lv.append(st["signal_level"]); pk.append(st["peak_level"]); starts.append(st["last_start_index"])
                crc.append(eng.read_fibs(0, 1)[1][0])
        lost = eng.counters()["sync_lost"]
        margin.append(eng.stats(0)["level_margin_events"])
        eng.close()
        return np.array(lv, np.float32), np.array(pk, np.float32), np.array(starts), np.array(crc), lost

    margin = []
    lv, pk, starts, crc, lost = run(True)
    n = min(len(lv), ora["n"])
    assert n >= ora["n"] - 1 and n >= 22 and lost >= 1
    assert np.array_equal(starts[:n], ora["start"][:n]) and np.array_equal(crc[:n], ora["crc"][:n])
    assert np.array_equal(lv[:n].view(np.uint32), ora["s_level"][:n].view(np.uint32)), np.abs(lv[:n] - ora["s_level"][:n]).max()
    assert np.array_equal(pk[:n].view(np.uint32), ora["peak_level"][:n].view(np.uint32))
    lv0, _pk0, starts0, crc0, _ = run(False)
    assert np.array_equal(starts0[:n], ora["start"][:n]) and np.array_equal(crc0[:n], ora["crc"][:n])
    assert np.abs(lv0[:n].astype(np.float64) - ora["s_level"][:n]).max() <= 1e-4 * ora["s_level"][:n].max()
    # dabx_stats.level_margin_events: how many of the search's comparisons came within 1e-4 of their threshold -- the only places
    # where the chunk-wise tracker (good to ~1e-5) could have decided differently.  Two searches of a few thousand comparisons each:
    # a handful at most, and the same count from both trackers when they walk the same way.
    assert 0 <= margin[0] <= 20 and abs(margin[1] - margin[0]) <= 2, margin


def _level_after(x, n):
    """SampleReader's sLevel after reading x[0..n) from its start value (sample_reader.cpp:245-248): every sample goes through
    get_samples exactly once, in order, whatever the state machine does with it -- so the level at a read position is a function of the
    samples alone."""
    return np.float32(ol.oracle().ora_level_walk(np.ascontiguousarray(x[:n], np.complex64), n, 0.1))


@pytest.mark.parametrize("gain", [0.25, 3e-4])
def test_search_after_a_lost_lock_starts_from_the_references_level(gain):
    """The default level tracker (cfg.exact_level_tracker = 0): chunk-wise in lock, where nothing reads it, and when the lock is lost
    the samples read since the search handed the stream over are walked exactly (level_from_anchor in k_acquire).  The null-symbol
    search then runs with the level the sample-serial recurrence has: after every step that leaves the stream searching, sLevel
    is BIT-IDENTICAL to the recurrence over all samples read so far -- before the first lock, and after 10 frames in lock and a
    drop-out.  Mode 2 (chunk-wise only, the behaviour before round 4) is close but not equal there."""
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=gain, seed=17, n_out=30 * ds.TF).copy()
    a, b = int(10.6 * ds.TF), int(14.4 * ds.TF)                   # a drop-out long enough for steps that search and find nothing
    x[a:b] = 0
    ora = ol.oracle_run(x, subch)

    def run(mode):
        eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=4, out_frames=4, exact_level_tracker=mode)
        eng.set_subchannels(subch)
        eng.push_iq(0, x)
        searching, starts, idle, steps = [], [], 0, 0
        while idle < 4 and steps < 400:
            before = eng.stats(0)
            eng.process(1)
            st = eng.stats(0)
            steps += 1
            idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
            if st["frames"] > before["frames"]:
                starts.append(st["last_start_index"])
            elif before["state"] == 1 and st["state"] == 1 and st["samples_consumed"] > before["samples_consumed"]:      # searched, still searching
                # (a step that BEGAN out of lock: in the step in which the correlation fails the search has not seen the stream yet)
                searching.append((st["samples_consumed"], np.float32(st["signal_level"]), st["frames"]))
        st = eng.stats(0)
        eng.close()
        return searching, np.array(starts), st

    searching, starts, st = run(0)
    n = min(len(starts), ora["n"])
    assert n >= ora["n"] - 1 and n >= 20 and np.array_equal(starts[:n], ora["start"][:n])
    after_lock = [t for t in searching if t[2] >= 5]
    assert len(searching) >= 2 and len(after_lock) >= 1, searching
    for pos, lv, _frames in searching:
        want = _level_after(x, pos)
        assert lv.view(np.uint32) == want.view(np.uint32), (pos, lv, want)
    assert st["level_rewalk_events"] >= 1 and st["level_unanchored_events"] == 0, st
    searching2, starts2, st2 = run(2)
    assert np.array_equal(starts2[:n], ora["start"][:n]) and st2["level_rewalk_events"] == 0
    diffs = [abs(float(lv) - float(_level_after(x, pos))) / float(lv) for pos, lv, frames in searching2 if frames >= 5]
    assert diffs and 0 < max(diffs) < 1e-4, diffs


def test_level_anchor_that_has_left_the_ring_is_counted():
    """Same stream, fed frame by frame through a ring of four frames: when the lock is lost after ten frames, the samples read since
    the search handed the stream over are long overwritten -- the level continues from the chunk-wise value (as before round 4: same
    walk here), and dabx_stats.level_unanchored_events says so."""
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=0.25, seed=17, n_out=30 * ds.TF).copy()
    x[int(10.6 * ds.TF):int(12.2 * ds.TF)] = 0
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=4, max_subch=4, out_frames=4)
    eng.set_subchannels(subch)
    starts, pushed = [], 0
    for _ in range(200):
        st = eng.stats(0)
        room = 4 * ds.TF - (pushed - st["samples_consumed"])
        m = min(room, ds.TF, len(x) - pushed)
        if m > 0:
            eng.push_iq(0, x[pushed:pushed + m]); pushed += m
        before = st
        eng.process(1)
        st = eng.stats(0)
        if st["frames"] > before["frames"]:
            starts.append(st["last_start_index"])
        elif m <= 0 and st["samples_consumed"] == before["samples_consumed"]:
            break
    st = eng.stats(0)
    eng.close()
    n = min(len(starts), ora["n"])
    assert n >= 20 and np.array_equal(np.array(starts[:n]), ora["start"][:n])
    # (the stream re-locks for one frame on its way through the drop-out: that second loss finds its anchor in the ring)
    assert st["level_unanchored_events"] == 1 and st["level_rewalk_events"] <= 1, st


def test_level_is_exact_again_when_two_walks_around_the_chunk_wise_value_have_merged():
    """A stream fed frame by frame through a ring of 13 frames loses its lock after 24 frames in lock: the anchor (where the search handed
    the stream over) left the ring long ago.  level_from_anchor then starts two walks 2^-9 below and above the chunk-wise level of the
    oldest frame boundary still in the ring; the recurrence forgets its start value, the two merge into one float after a few frames, and
    that float is the exact level: in every step that leaves the stream searching sLevel is bit-identical to the recurrence over all samples
    read (level_healed_events = 1, nothing unanchored)."""
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=0.25, seed=17, n_out=34 * ds.TF).copy()
    x[int(26.6 * ds.TF):int(30.4 * ds.TF)] = 0
    ring = 13
    eng = dx.Engine(n_streams=1, ring_frames=ring, max_subch=4, out_frames=4)
    eng.set_subchannels(subch)
    searching, pushed, frames_at_loss = [], 0, None
    for _ in range(300):
        st = eng.stats(0)
        m = min(ring * ds.TF - (pushed - st["samples_consumed"]), ds.TF, len(x) - pushed)
        if m > 0:
            eng.push_iq(0, x[pushed:pushed + m]); pushed += m
        before = st
        eng.process(1)
        st = eng.stats(0)
        if before["state"] == 1 and st["state"] == 1 and st["samples_consumed"] > before["samples_consumed"] and st["frames"] >= 20:
            searching.append((st["samples_consumed"], np.float32(st["signal_level"])))
        if m <= 0 and st["samples_consumed"] == before["samples_consumed"]:
            break
    st = eng.stats(0)
    eng.close()
    assert st["frames"] >= 26 and len(searching) >= 2, (st["frames"], searching)
    for pos, lv in searching:
        want = _level_after(x, pos)
        assert lv.view(np.uint32) == want.view(np.uint32), (pos, lv, want)
    assert st["level_healed_events"] == 1 and st["level_unanchored_events"] == 0, st


@pytest.mark.parametrize("announce", [False, True])
def test_zero_copy_producers_keep_the_level_anchor_by_announcing_their_writes(announce):
    """A device-resident producer (dabx_iq_ring_dev + dabx_commit_iq) writes where the library cannot see: after a plain commit a lost lock
    finds no trustworthy anchor (level_unanchored_events), the walk is the oracle's all the same here.  A producer that says how far it
    writes before it does (dabx_announce_write) keeps the anchor: the search resumes from the exact level."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=0.25, seed=17, n_out=30 * ds.TF).copy()
    x[int(10.6 * ds.TF):int(14.4 * ds.TF)] = 0
    x = np.ascontiguousarray(x, np.complex64)
    ora = ol.oracle_run(x, subch)
    eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=4, out_frames=4)
    eng.set_subchannels(subch)
    ptr, cap = eng.ring_ptr(0)
    assert cap >= len(x)
    if announce:
        eng.announce_write(len(x))
    assert hip.hipMemcpy(C.c_void_p(ptr), C.c_void_p(x.ctypes.data), C.c_size_t(8 * len(x)), 1) == 0          # host to device
    eng.commit(len(x))
    searching, starts, idle = [], [], 0
    for _ in range(400):
        before = eng.stats(0)
        eng.process(1)
        st = eng.stats(0)
        idle = idle + 1 if st["samples_consumed"] == before["samples_consumed"] else 0
        if st["frames"] > before["frames"]:
            starts.append(st["last_start_index"])
        elif before["state"] == 1 and st["state"] == 1 and st["samples_consumed"] > before["samples_consumed"] and st["frames"] >= 5:
            searching.append((st["samples_consumed"], np.float32(st["signal_level"])))
        if idle >= 4:
            break
    st = eng.stats(0)
    eng.close()
    n = min(len(starts), ora["n"])
    assert n >= 20 and np.array_equal(np.array(starts[:n]), ora["start"][:n]) and len(searching) >= 1
    exact = [lv.view(np.uint32) == _level_after(x, pos).view(np.uint32) for pos, lv in searching]
    if announce:
        assert all(exact) and st["level_rewalk_events"] >= 1 and st["level_unanchored_events"] == 0, (exact, st)
    else:
        assert not any(exact) and st["level_unanchored_events"] >= 1 and st["level_rewalk_events"] == 0, (exact, st)


def test_failed_sync_attempts_do_not_starve_a_stream():
    """A stream whose candidates keep failing the PRS correlation (fuzz seed 5001, stream 18: a fading channel 25 carriers off
    frequency, strongest-peak sync with threshold 4 -- false null dips every few thousand samples; the oracle needs 7.7 frames of
    failed attempts before its first lock) must still move through its samples at about a frame per step, like the reference,
    which goes straight back to the null-dip search (dab_processor.cpp:154-160, 396-400): the engine retries inside the step
    until a frame of samples is consumed.  (One attempt per step consumed 3.7 frames in 62 steps.)  The walk itself is the
    oracle's: same start indices, same FIBs."""
    import fuzz_cases as F
    layouts, cases, xs, _ = F.draw_streams(5001, only=18)
    x, subch = xs[18], layouts[cases[18][0]]
    ora = ol.oracle_run(x, subch, config=(4.0, 1, 2))
    assert ora["n"] >= 14 and ora["start"][0] > 0
    eng = dx.Engine(n_streams=1, ring_frames=len(x) // ds.TF + 1, max_subch=len(subch), out_frames=4, sync_threshold=4.0, sync_strongest=True, soft_bit_type=2)
    eng.set_subchannels(subch)
    eng.push_iq(0, x)
    fibs, crc, starts = [], [], []
    for step in range(1, 27):
        before = eng.stats(0)
        eng.process(1)
        st = eng.stats(0)
        if step == 7:
            assert st["frames"] == 0 and st["samples_consumed"] >= 5.5 * ds.TF, st        # seven steps of nothing but failed attempts: > 5.5 frames walked
        if st["frames"] > before["frames"]:
            f, c = eng.read_fibs(0, 1)
            fibs.append(f[0]); crc.append(c[0]); starts.append(st["last_start_index"])
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 13, (len(fibs), ora["n"])
    assert np.array_equal(np.array(starts)[:n], ora["start"][:n])
    assert np.array_equal(np.array(crc)[:n], ora["crc"][:n])
    ok = ora["crc"][:n].astype(bool)
    assert np.array_equal(np.array(fibs)[:n][ok], ora["fibs"][:n][ok])
    eng.close()


def test_streams_in_different_states_and_configurations_do_not_interact():
    """One engine, four streams: a different ensemble and sub-channel set on each (per-stream dabx_set_subchannels), one
    stream that receives its samples late, one with a drop-out, one left without any samples.  Every stream must produce
    exactly what a single-stream engine produces on the same samples."""
    mixed = _mixed_subchannels()
    full = ds.default_subchannels(18, 64)
    few = [full[2], full[9]]
    cfgs = [full, mixed, few, full]
    xs = []
    for s, cfg in enumerate(cfgs[:3]):
        ens = ds.build_ensemble(10, full if cfg is few else cfg, seed=80 + s)
        xs.append(ds.channel(ens.iq, snr_db=17.0 + 3 * s, cfo_hz=500.0 * (s - 1), timing_offset=40000 * s + 77, seed=30 + s, n_out=21 * ds.TF).copy())
    xs[2][int(8.2 * ds.TF):int(9.9 * ds.TF)] = 0                      # stream 2 loses lock for a while
    late = 6 * ds.TF                                                   # stream 1 gets nothing for the first 6 steps
    eng = dx.Engine(n_streams=4, ring_frames=22, max_subch=18, out_frames=4)
    for s in range(4):
        eng.set_subchannels(cfgs[s], stream=s)
    eng.push_iq(0, xs[0])
    eng.push_iq(2, xs[2])
    eng.process(6)
    assert eng.stats(1)["frames"] == 0 and eng.stats(3)["frames"] == 0 and eng.stats(0)["frames"] >= 4
    eng.push_iq(1, xs[1])
    for _ in range(30):
        eng.process(3)
    del late
    # a stream that lost its lock is searched NEXT to the steps of the others (also with sync = 1, since round 5) and joins the first step
    # after its search has finished: it needs a few more calls than a lone stream to get through the same samples
    idle, last = 0, None
    for _ in range(60):
        eng.process(1)
        now = [(eng.stats(s)["frames"], eng.stats(s)["samples_consumed"]) for s in range(4)]
        idle = idle + 1 if now == last else 0
        last = now
        if idle >= 4:
            break
    for s in range(3):
        ref = dx.Engine(n_streams=1, ring_frames=22, max_subch=18, out_frames=4)
        ref.set_subchannels(cfgs[s])
        ref.push_iq(0, xs[s])
        for _ in range(32):
            ref.process(3)
        a, b = eng.stats(s), ref.stats(0)
        for key in ("frames", "samples_consumed", "fib_ok", "fib_total", "sf_ok", "sf_fail", "rs_corrected", "au_ok", "au_bad",
                    "cifs_decoded", "last_start_index", "cif_count"):
            assert a[key] == b[key], (s, key, a[key], b[key])
        assert a["frames"] >= 15, (s, a["frames"], a["state"])
        fa, fb = eng.read_fibs(s, 4), ref.read_fibs(0, 4)
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1]), s
        eng.subch = ref.subch = list(cfgs[s])
        for j in range(len(cfgs[s])):
            assert np.array_equal(eng.read_msc(s, j, 16), ref.read_msc(0, j, 16)), (s, j)
            if getattr(cfgs[s][j], "dab_plus", 1):
                assert np.array_equal(eng.read_superframes(s, j, 2), ref.read_superframes(0, j, 2)), (s, j)
            assert eng.subch_stats(s, j) == ref.subch_stats(0, j), (s, j)
        ref.close()
    assert eng.stats(3)["frames"] == 0 and eng.stats(3)["samples_consumed"] == 0
    eng.close()


@pytest.mark.parametrize("threshold,strongest,soft_type", [(3.0, 0, 2), (3.0, 0, 3), (4.5, 1, 1), (2.0, 1, 3)])
def test_receiver_options_follow_the_oracle(threshold, strongest, soft_type):
    """ProcessParams: sync threshold, sync on the strongest peak, soft-bit generator 1..3 (ofdm_decoder.cpp:231-251) -- through
    the whole engine: start indices, FIB bytes, MSC bytes bit-exact; soft bits within the demapper tolerance."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=90 + soft_type)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=700.0, timing_offset=66000, seed=11, n_out=22 * ds.TF)
    ora = ol.oracle_run(x, subch, want_soft=True, config=(threshold, strongest, soft_type))
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"], sync_threshold=threshold, sync_strongest=bool(strongest),
                                                    soft_bit_type=soft_type, capture_soft=True)
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 18
    assert np.array_equal(starts[:n], ora["start"][:n])
    assert np.array_equal(crc[:n], ora["crc"][:n]) and np.array_equal(fibs[:n], ora["fibs"][:n])
    assert crc[6:n].all()
    k = eng.stats(0)["frames"] * 4 - 16
    for j in (1, 10, 16):
        o = ora["msc"][j].reshape(-1, 192)
        assert np.array_equal(eng.read_msc(0, j, 16), o[k - 16:k]), j
    if len(fibs) == ora["n"]:                               # soft bits of the last frame, same frame on both sides
        d = np.abs(eng.read_soft(0).astype(int) - ora["soft"][ora["n"] - 1].astype(int))
        assert d.max() <= 3 and np.mean(d > 1) < 2e-3, (d.max(), np.mean(d > 1))
    eng.close()


@pytest.mark.parametrize("ppm", [40.0, -65.0])
def test_sample_clock_offset_is_tracked_like_the_oracle(ppm):
    """A receiver clock that runs fast or slow: the PRS start index wanders, frames are read with +-1..8 samples more or
    less, the clock-error IIR moves (dab_processor.cpp:226-251).  Engine == oracle frame by frame."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=101)
    x0 = ds.channel(ens.iq, snr_db=19.0, cfo_hz=-220.0, timing_offset=12000, seed=13, n_out=27 * ds.TF)
    t = np.arange(int(26 * ds.TF)) * (1.0 + ppm * 1e-6)                     # linear interpolation at the offset rate
    i0 = np.floor(t).astype(np.int64)
    fr = (t - i0).astype(np.float32)
    x = (x0[i0] * (1 - fr) + x0[i0 + 1] * fr).astype(np.complex64)
    ora = ol.oracle_run(x, subch)
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"])
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 22
    # the start index follows the oracle frame by frame, re-acquisitions included
    d = starts[:n].astype(int) - ora["start"][:n].astype(int)
    bad = np.nonzero(~np.all(ora["crc"][:n] == 1, axis=1))[0]
    locked_from = int(bad[-1]) + 1 if len(bad) else 0                       # start of the final, uninterrupted lock
    assert np.all(d == 0), (d, locked_from)
    assert len(set(starts[locked_from:n].tolist())) >= 2                    # the index does wander
    assert np.array_equal(crc[:n], ora["crc"][:n]) and np.array_equal(fibs[:n], ora["fibs"][:n])
    assert crc[locked_from:n].all() and n - locked_from >= 10
    _check_frame_scalars(eng, fbbs, ora, n)                                  # incl. the clock error the demapper's phase ramp uses
    st = eng.stats(0)
    ce = -st["clock_err_hz"] / (2.048 * ppm)                                # 1 ppm = 2.048 Hz of sample clock; IIR still settling
    assert 0.5 < ce < 1.3, st["clock_err_hz"]
    k = st["frames"] * 4 - 16
    for j in (0, 9, 17):
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, 192)[k - 16:k]), j
    eng.close()


@pytest.mark.parametrize("snr", [5.0, 3.8])
def test_low_snr_error_paths_follow_the_oracle(snr):
    """Close to the threshold: FIB CRC failures, fire-code misses, RS corrections and RS failures (which leave partially
    corrected data, reed_solomon.cpp:140-439), bad AU CRCs, super-frame resynchronisation -- every counter of every
    sub-channel and every byte as in the oracle."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=120)
    # the recording ends 30 000 samples into a frame: too short for the oracle to finish another CIF, so both sides have
    # decoded exactly the same CIFs and every counter is comparable
    x = ds.channel(ens.iq, snr_db=snr, cfo_hz=333.0, timing_offset=20000, seed=17, n_out=25 * ds.TF + 20000 + 30000)
    ora = ol.oracle_run(x, subch)
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"])
    n = min(len(fibs), ora["n"])
    assert len(fibs) == ora["n"] and n >= 18
    assert np.array_equal(starts[:n], ora["start"][:n])
    assert np.array_equal(crc[:n], ora["crc"][:n]) and np.array_equal(fibs[:n], ora["fibs"][:n])
    compared = 0
    seen = dict(rs_corrected=0, rs_failed=0, au_bad=0, sf_fail=0)
    for j in range(18):
        st, o = eng.subch_stats(0, j), ora["stats"][j]
        assert st["cifs_decoded"] == o["cif_out"], (j, st["cifs_decoded"], o["cif_out"])
        compared += 1
        for a, b in (("sf_ok", "sf_ok"), ("sf_fail", "sf_fail"), ("rs_corrected", "rs_corr"), ("rs_failed", "rs_fail"),
                     ("fc_corrected", "fc_corr"), ("au_ok", "au_ok"), ("au_bad", "au_bad")):
            assert st[a] == o[b], (j, a, st[a], o[b])
        for key in seen:
            seen[key] += st[key]
        k = st["cifs_decoded"]
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, 192)[k - 16:k]), j
        sf_o = ora["sf"][j].reshape(-1, 880)
        got = eng.read_superframes(0, j, 3)
        if len(sf_o) >= 3:
            assert np.array_equal(got, sf_o[len(sf_o) - 3:]), j
    assert compared == 18 and seen["rs_corrected"] > 0     # the paths were exercised
    if snr < 4:
        assert seen["rs_failed"] + seen["au_bad"] + seen["sf_fail"] > 0, seen
    eng.close()


def test_push_refuses_to_overwrite_unread_samples():
    eng = dx.Engine(n_streams=2, ring_frames=3, max_subch=0, fic_only=True)
    x = np.zeros(2 * ds.TF, np.complex64)
    eng.push_iq(0, x)
    with pytest.raises(dx.DabxError):
        eng.push_iq(0, x)                                   # 4 frames into a 3-frame ring
    eng.push_iq(1, x)                                       # the other stream is independent
    eng.push_iq(0, x[:ds.TF])                               # exactly full is fine
    with pytest.raises(dx.DabxError):
        eng.push_iq(0, x[:1])
    eng.close()


def test_largest_and_smallest_subchannels():
    """Sizes at both ends: a 320 kbit/s DAB+ sub-channel (240 CU, 40 RS code words per super frame, 960-byte logical
    frames, AUs of up to 960 bytes) beside an 8 kbit/s one (1 code word, 24-byte frames) -- bit-exact vs the oracle."""
    subch = [ds.SubCh(1, 0, 240, 320, 2, 0), ds.SubCh(2, 300, 12, 8, 0, 0)]
    ens = ds.build_ensemble(10, subch, seed=131)
    x = ds.channel(ens.iq, snr_db=15.0, cfo_hz=410.0, timing_offset=7777, seed=19, n_out=23 * ds.TF + 50000)
    ora = ol.oracle_run(x, subch)
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"])
    n = min(len(fibs), ora["n"])
    assert len(fibs) == ora["n"] and n >= 20
    assert np.array_equal(crc[:n], ora["crc"][:n]) and np.array_equal(fibs[:n], ora["fibs"][:n])
    for j, c in enumerate(subch):
        st, o = eng.subch_stats(0, j), ora["stats"][j]
        assert st["cifs_decoded"] == o["cif_out"] and st["cifs_decoded"] >= 60
        for a, b in (("sf_ok", "sf_ok"), ("sf_fail", "sf_fail"), ("rs_corrected", "rs_corr"), ("rs_failed", "rs_fail"),
                     ("au_ok", "au_ok"), ("au_bad", "au_bad")):
            assert st[a] == o[b], (j, a, st[a], o[b])
        assert st["sf_ok"] >= 10
        k, nb = st["cifs_decoded"], 3 * c.kbps
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, nb)[k - 16:k]), j
        sf_o = ora["sf"][j].reshape(-1, 110 * c.kbps // 8)
        assert np.array_equal(eng.read_superframes(0, j, 3), sf_o[len(sf_o) - 3:]), j
        assert any(np.array_equal(sf_o[-1], ens.superframes[j][q]) for q in range(8)), j
    eng.close()


def test_maximum_dab_plus_rate_384_kbit_with_rs_corrections():
    """The largest sub-channel the DAB+ stage holds: 384 kbit/s (EEP 3-A, 288 CU; 48 RS code words per super frame fill the
    5-frame window in LDS to its last byte, 1152-byte logical frames, a 9216-step trellis) next to a 64 kbit/s one, at
    9.5 dB where Reed-Solomon has byte errors to correct -- bit-exact vs the oracle including every RS / AU counter (the
    synthetic super frame's sixth AU is longer than 960 bytes at this rate: counted as bad on both sides, mp4processor.cpp:300-304)."""
    subch = [ds.SubCh(1, 0, 288, 384, 2, 0), ds.SubCh(2, 400, 48, 64, 2, 0)]
    ens = ds.build_ensemble(10, subch, seed=133)
    x = ds.channel(ens.iq, snr_db=9.5, cfo_hz=-377.0, timing_offset=7777, seed=23, n_out=23 * ds.TF + 50000)
    ora = ol.oracle_run(x, subch)
    eng, fibs, crc, msc, starts, fbbs = _engine_run(x, subch, ora["n"])
    n = min(len(fibs), ora["n"])
    assert len(fibs) == ora["n"] and n >= 20
    assert np.array_equal(crc[:n], ora["crc"][:n])
    ok = ora["crc"][:n].astype(bool)
    assert np.array_equal(fibs[:n][ok], ora["fibs"][:n][ok])
    for j, c in enumerate(subch):
        st, o = eng.subch_stats(0, j), ora["stats"][j]
        assert st["cifs_decoded"] == o["cif_out"] and st["cifs_decoded"] >= 60
        for a, b in (("sf_ok", "sf_ok"), ("sf_fail", "sf_fail"), ("rs_corrected", "rs_corr"), ("rs_failed", "rs_fail"),
                     ("au_ok", "au_ok"), ("au_bad", "au_bad")):
            assert st[a] == o[b], (j, a, st[a], o[b])
        assert st["sf_ok"] >= 8
        k, nb = st["cifs_decoded"], 3 * c.kbps
        assert np.array_equal(eng.read_msc(0, j, 16), ora["msc"][j].reshape(-1, nb)[k - 16:k]), j
        sf_o = ora["sf"][j].reshape(-1, 110 * c.kbps // 8)
        assert np.array_equal(eng.read_superframes(0, j, 3), sf_o[len(sf_o) - 3:]), j
    assert eng.subch_stats(0, 0)["rs_corrected"] > 0                      # the decoder really had errors to correct at this SNR
    eng.close()


def test_growing_the_largest_bit_rate_keeps_every_running_service_and_stream():
    """Adding a sub-channel with a higher bit rate than any configured before widens the output-ring slots
    (dabx_set_subchannels re-strides the rings with their contents).  The reference's MscHandler::set_channel only adds a
    Backend (msc_handler.cpp:95-131): services already running -- on this and on every OTHER stream of the engine -- keep
    decoding without a gap, their counters, logical frames, super frames and ETI frames unaffected."""
    sub_a = [ds.SubCh(1, 0, 48, 64, 2, 0), ds.SubCh(2, 48, 48, 64, 2, 0)]
    sub_b = [ds.SubCh(7, 100, 96, 128, 2, 0), ds.SubCh(8, 300, 48, 64, 2, 0)]
    ens_a, ens_b = ds.build_ensemble(10, sub_a, seed=71), ds.build_ensemble(10, sub_b, seed=72)
    xa = ds.channel(ens_a.iq, snr_db=19.0, cfo_hz=333.0, timing_offset=4321, seed=71, n_out=25 * ds.TF)
    xb = ds.channel(ens_b.iq, snr_db=18.0, cfo_hz=-712.0, timing_offset=99999, seed=72, n_out=25 * ds.TF)
    ora_a, ora_b = ol.oracle_run(xa, sub_a), ol.oracle_run(xb, sub_b)
    mk = lambda c: dx.SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, 1, 0)   # noqa: E731
    eng = dx.Engine(n_streams=2, ring_frames=26, max_subch=2, out_frames=8)
    eng.set_subchannels([mk(c) for c in sub_a], stream=0)               # largest rate so far: 64 kbit/s
    eng.push_iq(0, xa)
    eng.push_iq(1, xb)
    eng.process(9)
    s0 = [eng.subch_stats(0, j) for j in range(2)]
    assert all(q["cifs_decoded"] == 9 * 4 - 16 for q in s0)
    eti_before, lost = eng.read_eti(0, 32)
    assert lost == 0 and len(eti_before) == 9 * 4 - 16
    eng.set_subchannels([mk(c) for c in sub_b], stream=1)               # 128 kbit/s on the OTHER stream: the rings grow
    eng.process(6)
    eti_mid, lost_mid = eng.read_eti(0, 64)                             # (the FIB ring holds 8 frames: read at least that often)
    eng.process(6)
    fr0, fr1 = eng.stats(0)["frames"], eng.stats(1)["frames"]
    assert fr0 == 21 and fr1 == 21
    eng.subch = list(sub_a)                                             # layout of the stream being read (wrapper: buffer sizes)
    for j in range(2):                                                  # stream 0: no restart, no gap, bytes == oracle
        q = eng.subch_stats(0, j)
        assert q["start_cif"] == s0[j]["start_cif"] == 0 and q["cifs_decoded"] == fr0 * 4 - 16
        o = ora_a["msc"][j].reshape(-1, 192)
        assert np.array_equal(eng.read_msc(0, j, 32), o[fr0 * 4 - 16 - 32:fr0 * 4 - 16]), j
        assert q["sf_ok"] == (fr0 * 4 - 20) // 5 and q["sf_fail"] == 0      # super frames start at CIFs that are multiples of 5: the first whole one begins at CIF 20
        sf_o = ora_a["sf"][j].reshape(-1, 880)
        assert np.array_equal(eng.read_superframes(0, j, 4), sf_o[q["sf_ok"] - 4:q["sf_ok"]]), j
    eti_after, lost = eng.read_eti(0, 64)                               # the ETI stream of stream 0 continues seamlessly
    assert lost == 0 and lost_mid == 0
    eti_after = np.concatenate([eti_mid, eti_after])
    assert len(eti_after) == 12 * 4
    both = np.concatenate([eti_before, eti_after])
    descs = [mk(c) for c in sub_a]
    for i in (0, len(eti_before) - 1, len(eti_before), len(eti_before) + 1, len(both) - 1):   # either side of the change == oracle assembly
        r = 16 + i
        F, k = divmod(r, 4)
        fib = ora_a["fibs"][F].reshape(-1)
        hi, lo = int(fib[4] & 0x1F), int(fib[5])
        for g in range(4):
            if ora_a["crc"][F][3 * g]:
                hi, lo = int(ora_a["fibs"][F][3 * g][4] & 0x1F), int(ora_a["fibs"][F][3 * g][5])
        msc = [ora_a["msc"][j].reshape(-1, 192)[r - 16] for j in range(2)]
        want, _ = ol.ora_eti_frame(hi, lo, k, descs, fib[96 * k:96 * k + 96], msc)
        assert np.array_equal(both[i], want), i
    eng.subch = list(sub_b)
    for j, c in enumerate(sub_b):                                       # stream 1: started at its own CIF, bytes == oracle
        q = eng.subch_stats(1, j)
        assert q["start_cif"] == 36 and q["cifs_decoded"] == fr1 * 4 - 36 - 16
        o = ora_b["msc"][j].reshape(-1, 3 * c.kbps)
        assert np.array_equal(eng.read_msc(1, j, 16), o[fr1 * 4 - 16 - 16:fr1 * 4 - 16]), j
    eng.close()


def test_dab_plus_is_refused_for_rates_the_super_frame_stage_cannot_hold():
    """k_dabplus stages a super frame of at most 384 kbit/s (48 RS code words) in LDS and DAB+ rates are multiples of
    8 kbit/s: anything else must be refused at configuration time (DABX_E_PROFILE), not decoded out of bounds."""
    eng = dx.Engine(n_streams=1, ring_frames=3, max_subch=2, out_frames=2)
    ok = dx.SubchDesc(1, 0, 6, 8, 2, 0, 1, 0)                            # 8 kbit/s EEP 3-A (n = 1): 6 CU
    eng.set_subchannels([ok])
    for kbps, cu, prot in ((392, 294, 2), (20, 15, 2)):                  # EEP 3-A: 6 n CU with n = kbps / 8 (20 is not a multiple of 8)
        bad = dx.SubchDesc(2, 300, cu, kbps, prot, 0, 1, 0)
        n_in = dx.load().dabx_profile_input_bits(kbps, prot, 0)
        if n_in < 0:
            continue                                                     # not a legal EEP profile at all: nothing to refuse
        with pytest.raises(dx.DabxError):
            eng.set_subchannels([ok, bad])
        plain = dx.SubchDesc(2, 300, cu, kbps, prot, 0, 0, 0)            # the same sub-channel without the DAB+ stage is fine
        eng.set_subchannels([ok, plain])
    eng.close()


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("snr", [4.4, 30.0])
def test_simd_viterbi_arithmetic_on_the_lane_per_trellis_decoder(mode, snr):
    """cfg.viterbi_tie_mode 1 / 2 with the MSC on the lane-per-trellis kernels (k_msc_vitT_avx2 / _sse2): 6 streams x 18
    sub-channels in one engine forced onto that path, against single-stream engines on the wave-per-trellis kernel (which the
    test below compares with the oracle receiver).  4.4 dB: ties and near-ties decide bits; 30 dB: strong symbols, the metrics
    sit near the renormalisation threshold for long stretches (saturation zone)."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=78)
    n_streams, n_frames = 6, 24
    xs = [ds.channel(ens.iq, snr_db=snr + 0.2 * s, cfo_hz=170.0 * (s - 3), timing_offset=5003 * s + 7, seed=780 + s, n_out=(n_frames + 3) * ds.TF)
          for s in range(n_streams)]
    eng = dx.Engine(n_streams=n_streams, ring_frames=n_frames + 4, max_subch=18, viterbi_tie_mode=mode, msc_fast_min_jobs=64, msc_class_min_jobs=1)
    eng.set_subchannels(subch)
    for s in range(n_streams):
        eng.push_iq(s, xs[s])
    dx.check(dx.load().dabx_set_profiling(eng._h, 1))
    eng.process(n_frames)
    launches = kernel_launches(eng)
    dx.check(dx.load().dabx_set_profiling(eng._h, 0))
    assert launches["k_msc_vitT"] >= 4 and launches["k_msc_frame"] == 0, launches
    for s in (0, 3, 5):
        ref = dx.Engine(n_streams=1, ring_frames=n_frames + 4, max_subch=18, viterbi_tie_mode=mode)
        ref.set_subchannels(subch)
        ref.push_iq(0, xs[s])
        ref.process(n_frames)
        a, b = eng.stats(s), ref.stats(0)
        for key in ("frames", "fib_ok", "sf_ok", "sf_fail", "rs_corrected", "rs_failed", "au_ok", "au_bad", "cifs_decoded", "last_start_index"):
            assert a[key] == b[key], (s, key, a[key], b[key])
        assert a["frames"] >= n_frames - 2 and (snr < 10 or a["sf_ok"] > 0)
        for j in range(18):
            assert np.array_equal(eng.read_msc(s, j, 32), ref.read_msc(0, j, 32)), (s, j)
            assert np.array_equal(eng.read_superframes(s, j, 4), ref.read_superframes(0, j, 4)), (s, j)
        ref.close()
    eng.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_avx2_viterbi_build_of_the_reference_is_selectable_for_the_whole_receiver(mode):
    """cfg.viterbi_tie_mode = 1 / 2: FIC and MSC are decoded with the arithmetic of the reference's VITERBI_AVX2 build
    (viterbi_16way.h) or of its VITERBI_SSE2 / NEON builds (viterbi_8way.h); both pinned against the reference's object code
    in test_gpu_viterbi / test_oracle_ref.  At 4.3 dB -- where trellis ties and near-ties decide bits -- the engine follows
    the oracle receiver switched to the same body, frame by frame, including the FIBs that fail their CRC and the super
    frames RS cannot repair.  (The SSE2 body differs from the scalar one only where a path metric saturates, which on a real
    signal only happens to paths that have already lost: no difference is demanded of it here.)"""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=77)
    x = ds.channel(ens.iq, snr_db=4.3, cfo_hz=-150.0, timing_offset=31000, seed=77, n_out=24 * ds.TF)
    L = ol.oracle()
    canon = ol.oracle_run(x, subch)
    L.ora_set_viterbi_mode(mode)
    try:
        ora = ol.oracle_run(x, subch)
    finally:
        L.ora_set_viterbi_mode(0)
    eng = dx.Engine(n_streams=1, ring_frames=25, max_subch=18, out_frames=4, viterbi_tie_mode=mode)
    eng.set_subchannels(subch)
    eng.push_iq(0, x)
    fibs, crc = [], []
    for _ in range(ora["n"] + 3):
        before = eng.stats(0)["frames"]
        eng.process(1)
        if eng.stats(0)["frames"] > before:
            f, c = eng.read_fibs(0, 1)
            fibs.append(f[0]); crc.append(c[0])
    fibs, crc = np.array(fibs), np.array(crc)
    n = min(len(fibs), ora["n"])
    assert n >= ora["n"] - 1 and n >= 18
    assert np.array_equal(crc[:n], ora["crc"][:n])
    ok = ora["crc"][:n].astype(bool)
    assert np.array_equal(fibs[:n][ok], ora["fibs"][:n][ok])                # every FIB that passes its CRC (failed ones: float demapper tolerance)
    k = eng.stats(0)["frames"] * 4 - 16
    same = 0
    for j in range(18):
        st, o = eng.subch_stats(0, j), ora["stats"][j]
        if st["cifs_decoded"] == o["cif_out"]:
            assert (st["sf_ok"], st["sf_fail"], st["rs_corrected"], st["rs_failed"]) == (o["sf_ok"], o["sf_fail"], o["rs_corr"], o["rs_fail"]), j
        got = eng.read_msc(0, j, 16)
        want = ora["msc"][j].reshape(-1, 192)[k - 16:k]
        same += int(np.array_equal(got, want))
    assert same >= 16                                                      # byte-exact logical frames on (nearly) all sub-channels at 4.3 dB
    # the two bodies do decode this signal differently somewhere
    differs = not np.array_equal(canon["fibs"][:n], ora["fibs"][:n]) or any(
        not np.array_equal(canon["msc"][j], ora["msc"][j]) for j in range(18))
    assert differs or mode == 2
    eng.close()


@pytest.mark.parametrize("fmt", ["u8", "i16"])
def test_async_pushes_from_page_locked_buffers_decode_like_synchronous_ones(fmt):
    """dabx_push_iq_async + dabx_host_register: three streams fed in 2-frame pieces from one page-locked recording buffer,
    many pushes queued before a single dabx_push_wait, decode exactly like the same samples pushed synchronously."""
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=81)
    x = ds.channel(ens.iq, snr_db=18.0, cfo_hz=-640.0, timing_offset=7171, seed=81, n_out=20 * ds.TF)
    pairs = (x * np.complex64(0.25 / np.sqrt(np.mean(np.abs(x) ** 2)))).view(np.float32)
    host = (np.clip(np.round(pairs * 128.0 + 127.38), 0, 255).astype(np.uint8) if fmt == "u8"
            else np.clip(np.round(pairs * 32768.0), -32768, 32767).astype(np.int16))
    ref = dx.Engine(n_streams=1, ring_frames=21, max_subch=4, out_frames=8)
    ref.set_subchannels(subch)
    ref.push_iq(0, host)
    ref.process(20)
    # (7 frames of ring for 2-frame pushes: with sync=False the search for the first null symbol runs next to the steps, which go
    # by unused until it has finished -- the streams start about two frames behind their producer and stay there)
    eng = dx.Engine(n_streams=3, ring_frames=7, max_subch=4, out_frames=8)
    eng.set_subchannels(subch)
    dx.host_register(host)
    try:
        step = 2 * ds.TF * 2                                  # 2 frames of interleaved I/Q values
        for pos in range(0, len(host), step):
            for s in range(3):
                eng.push_iq_async(s, host[pos:pos + step])   # 3 copies in flight, the caller does not wait
            eng.process(2, sync=False)
        eng.push_wait()
        eng.process(4)                                        # streams out of lock are searched NEXT to asynchronous steps: what that left over
    finally:
        dx.host_unregister(host)
    a = ref.stats(0)
    for s in range(3):
        b = eng.stats(s)
        for key in ("frames", "samples_consumed", "fib_ok", "fib_total", "sf_ok", "sf_fail", "cifs_decoded", "last_start_index"):
            assert a[key] == b[key], (s, key, a[key], b[key])
        fa, ca = ref.read_fibs(0, 8)
        fb, cb = eng.read_fibs(s, 8)
        assert np.array_equal(fa, fb) and np.array_equal(ca, cb)
        for j in range(4):
            assert np.array_equal(ref.read_msc(0, j, 16), eng.read_msc(s, j, 16)), (s, j)
    assert a["frames"] >= 17 and a["sf_ok"] > 0
    eng.close(); ref.close()


def test_repeated_drop_outs_under_asynchronous_pushes_follow_the_oracle():
    """The level anchor's bookkeeping next to a producer that keeps overwriting the ring: a stream with a drop-out every nine frames, fed
    one frame at a time with dabx_push_iq_async through a ring of six frames while the steps (and the search, on its own HIP stream) run
    asynchronously.  Some returns to the search find their anchor in the ring, some find it overwritten and use two walks or the
    chunk-wise value -- whichever, every frame is found where the oracle finds it, and every return is accounted for."""
    subch = ds.default_subchannels(4, 64)
    ens = ds.build_ensemble(10, subch, seed=171)
    x = ds.channel(ens.iq, snr_db=16.0, cfo_hz=911.0, timing_offset=77777, gain=0.25, seed=17, n_out=44 * ds.TF).copy()
    for k in (9.6, 18.6, 27.6, 36.6):
        x[int(k * ds.TF):int((k + 1.7) * ds.TF)] = 0
    x = np.ascontiguousarray(x, np.complex64)
    ora = ol.oracle_run(x, subch)
    ring = 6
    eng = dx.Engine(n_streams=1, ring_frames=ring, max_subch=4, out_frames=8)
    eng.set_subchannels(subch)
    dx.host_register(x)
    walk, seen, pushed, idle = [], 0, 0, 0
    try:
        for _ in range(600):
            st = eng.stats(0)
            m = min(ring * ds.TF - (pushed - st["samples_consumed"]), ds.TF, len(x) - pushed)
            if m > 0:
                eng.push_iq_async(0, x[pushed:pushed + m]); pushed += m
            eng.process(1, sync=False)
            st2 = eng.stats(0)
            if st2["frames"] > seen:
                pos, sti = eng.read_frame_info(0, st2["frames"] - seen)
                walk.extend(zip(pos.tolist(), sti.tolist())); seen = st2["frames"]
            idle = idle + 1 if (m <= 0 and st2["samples_consumed"] == st["samples_consumed"]) else 0
            if idle >= 6:
                break
        eng.push_wait()
    finally:
        dx.host_unregister(x)
    st = eng.stats(0)
    lost = eng.counters()["sync_lost"]
    eng.close()
    n = min(len(walk), ora["n"])
    assert n >= 30 and abs(len(walk) - ora["n"]) <= 1, (len(walk), ora["n"])
    assert [w[0] for w in walk[:n]] == ora["sym0"][:n].tolist() and [w[1] for w in walk[:n]] == ora["start"][:n].tolist()
    events = st["level_rewalk_events"] + st["level_healed_events"] + st["level_unanchored_events"]
    assert lost >= 4 and 4 <= events <= lost, (st, lost)


@pytest.mark.parametrize("mode", [1, 2])
def test_dc_and_iq_imbalance_correction_follows_the_oracle(mode):
    """cfg.dc_iq_correction (SampleReader::set_dc_and_iq_correction, sample_reader.cpp:218-243; off by default): a receiver
    front end with a DC offset and a Q channel that is 6 % too strong and 3 degrees skewed.  The GPU corrects the committed
    samples in place with a block scan of the five one-pole filters: floating point, so parity is a tolerance -- 4e-6 of full scale
    against the same filters with exact (double) states, and no further from the oracle's float recurrence than that recurrence's
    own rounding noise.  The receiver behind it decodes the same FIBs and MSC bytes as the oracle receiver with the correction on.
    (The scan itself -- launch partitions, ring wrap, several streams, the carried state, degenerate inputs -- is held to bounds of its
    own in tests/test_gpu_dciq_stage.py: a correct scan stays below 2.3e-7 of full scale DC only and 2.4e-6 with the IQ correction.)"""
    subch = ds.default_subchannels(6, 64)
    ens = ds.build_ensemble(10, subch, seed=95)
    x = ds.channel(ens.iq, snr_db=17.0, cfo_hz=380.0, timing_offset=52000, seed=95, n_out=22 * ds.TF)
    g, ph = 1.06, np.deg2rad(3.0)
    y = (x.real + 1j * g * (x.imag * np.cos(ph) + x.real * np.sin(ph)) + (0.03 - 0.02j)).astype(np.complex64)
    L = ol.oracle()
    rx = L.ora_rx_create(ol.make_descs(subch), len(subch))
    L.ora_rx_set_dc_iq(rx, mode)
    n = L.ora_rx_run(rx, y, len(y), 10000)
    cap = L.ora_rx_get_capture(rx).contents
    o_fibs = np.ctypeslib.as_array(cap.fibs, (n, 12, 32)).copy()
    o_crc = np.ctypeslib.as_array(cap.fib_crc, (n, 12)).copy()
    o_start = np.ctypeslib.as_array(cap.start_idx, (n,)).copy()
    o_msc = [ol.backend_bytes(rx, i, "msc").reshape(-1, 192) for i in range(len(subch))]
    L.ora_rx_destroy(rx)
    eng = dx.Engine(n_streams=1, ring_frames=23, max_subch=len(subch), out_frames=4, dc_iq_correction=mode)
    eng.set_subchannels(subch)
    pos, fibs, crc, starts = 0, [], [], []
    rng = np.random.default_rng(3)
    while pos < len(y):                                      # pushed in uneven pieces: the filters carry their state across calls
        m = int(min(len(y) - pos, rng.choice([4096, 100000, 3 * ds.TF + 17])))
        eng.push_iq(0, y[pos:pos + m])
        pos += m
        while True:
            before = eng.stats(0)["frames"]
            eng.process(1)
            st = eng.stats(0)
            if st["frames"] == before:
                break
            f, c = eng.read_fibs(0, 1)
            fibs.append(f[0]); crc.append(c[0]); starts.append(st["last_start_index"])
    # corrected samples in the ring: against the filters run with double-precision states (what the block scan computes up to
    # float rounding of its outputs), and against the oracle's float recurrence, whose own rounding noise is the larger part:
    # with ALPHA = 4.9e-7 a float update of a mean near 1 loses up to 6 % of its increment (measured here, not assumed)
    want32, want64 = y.copy(), y.copy()
    st5, st5d = np.array([0, 0, 1, 1, 0], np.float32), np.array([0, 0, 1, 1, 0], np.float64)
    L.ora_dciq_buffer(want32, len(y), mode, st5)
    L.ora_dciq_buffer_f64(want64, len(y), mode, st5d)
    got = eng.read_iq(0, 0, len(y))
    ref_noise = np.abs(want32 - want64).max()
    assert np.abs(got - want64).max() <= 4e-6                               # full scale 1, signal rms 0.26
    assert np.abs(got - want32).max() <= ref_noise + 4e-6
    assert ref_noise < (5e-6 if mode == 1 else 1e-3)
    assert abs(st5[0] - 0.03) < 0.01 and abs(st5[1] + 0.02) < 0.01        # the DC estimate has settled on the offset (1-s time constant, 2.1 s of signal)
    k = min(len(fibs), n)
    assert k >= n - 1 and k >= 18
    assert np.array_equal(np.array(starts)[:k], o_start[:k])
    assert np.array_equal(np.array(crc)[:k], o_crc[:k]) and np.array_equal(np.array(fibs)[:k], o_fibs[:k])
    assert np.array(crc)[8:k].all()
    kk = eng.stats(0)["frames"] * 4 - 16
    for j in range(len(subch)):
        assert np.array_equal(eng.read_msc(0, j, 16), o_msc[j][kk - 16:kk]), j
    eng.close()


@pytest.mark.parametrize("cfg", [
    {"schedule": 1},                                                   # every kernel on one HIP stream, in program order
    {"msc_fast_min_jobs": 64, "msc_class_min_jobs": 1},               # MSC on the lane-per-trellis kernels (own stream) even for 3 streams
    {"schedule": 1, "msc_fast_min_jobs": 64, "msc_class_min_jobs": 1},
    {"exact_level_tracker": True},                                     # the level tracker feeds nothing while in lock
], ids=lambda c: "+".join("%s=%s" % kv for kv in c.items()))
def test_schedule_and_decoder_choice_do_not_change_a_byte(cfg):
    """dabx_config.schedule only moves kernels between HIP streams, msc_fast_min_jobs / msc_class_min_jobs select which of the
    two MSC decoder kernels runs: soft bits of every symbol, FIBs and CRC flags, MSC bytes, super frames, the per-frame
    scalars and every counter are identical to the default configuration's (which the rest of this file compares with the
    oracle).  A missing dependency between the engine's streams shows up here as a difference."""
    subch = ds.default_subchannels(18, 64)
    ens = ds.build_ensemble(10, subch, seed=92)
    x = ds.channel(ens.iq, snr_db=8.0, cfo_hz=-1730.0, timing_offset=99000, seed=92, n_out=21 * ds.TF)

    def run(**kw):
        eng = dx.Engine(n_streams=3, ring_frames=22, max_subch=18, out_frames=8, capture_soft=True, **kw)
        eng.set_subchannels(subch)
        for s in range(3):
            eng.push_iq(s, x[2111 * s:])
        soft = []
        for m in (1, 1, 3, 7, 2, 5):                                   # 19 frames in calls of different sizes (MSC batches of 1..7 frames)
            eng.process(m)
            soft.append([eng.read_soft(s).copy() for s in range(3)])
        out = dict(soft=soft, stats=[eng.stats(s) for s in range(3)], fibs=[eng.read_fibs(s, 8) for s in range(3)],
                   msc=[[eng.read_msc(s, j, 16) for j in range(18)] for s in range(3)],
                   sf=[[eng.read_superframes(s, j, 2) for j in range(18)] for s in range(3)],
                   sub=[[eng.subch_stats(s, j) for j in range(18)] for s in range(3)], counters=eng.counters())
        eng.close()
        return out

    ref = run()
    got = run(**cfg)
    if cfg.get("exact_level_tracker"):                                 # the one field that mode is allowed to move (by ~1e-5 relative)
        for a_, b_ in zip(got["stats"], ref["stats"]):
            assert abs(a_["signal_level"] - b_["signal_level"]) <= 1e-4 * b_["signal_level"]
            a_["signal_level"] = b_["signal_level"]; a_["peak_level"] = b_["peak_level"]
    assert ref["stats"][0]["frames"] >= 17 and ref["counters"]["sf_ok"] > 0
    assert got["counters"] == ref["counters"] and got["stats"] == ref["stats"] and got["sub"] == ref["sub"]
    for a, b in zip(got["soft"], ref["soft"]):
        for s in range(3):
            assert np.array_equal(a[s], b[s]), s
    for s in range(3):
        assert np.array_equal(got["fibs"][s][0], ref["fibs"][s][0]) and np.array_equal(got["fibs"][s][1], ref["fibs"][s][1])
        for j in range(18):
            assert np.array_equal(got["msc"][s][j], ref["msc"][s][j]), (s, j)
            assert np.array_equal(got["sf"][s][j], ref["sf"][s][j]), (s, j)
