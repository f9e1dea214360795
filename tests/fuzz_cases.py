"""The random draws of the differential fuzz tests (tests/test_gpu_fuzz.py): three sub-channel layouts and, per seed, 24 streams with their own
channels.  No device is needed to draw them."""
import os
import sys

import numpy as np

import oracle_lib as ol

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools import dab_synth as ds  # noqa: E402

N_CASES, N_FRAMES = 24, 22


def _layouts():
    uep = lambda k, l: (ol.ora_uep_map(k, l)[1] >= 0).astype(np.uint8)                   # noqa: E731
    mixed = [ds.SubCh(3, 0, 24, 32, 3, 1, mask=uep(32, 3), dab_plus=0), ds.SubCh(7, 30, 48, 32, 0, 0),
             ds.SubCh(12, 80, 128, 128, 1, 0), ds.SubCh(20, 210, 54, 96, 6, 0), ds.SubCh(21, 270, 24, 48, 3, 0),
             ds.SubCh(33, 300, 48, 64, 2, 0), ds.SubCh(40, 350, 54, 64, 4, 0), ds.SubCh(63, 410, 116, 128, 2, 1, mask=uep(128, 2))]
    full = ds.default_subchannels(18, 64)
    return [full, mixed, [full[1], full[8], full[17]]]


def draw_streams(seed, only=None):
    """The N_CASES random streams of one seed: (layouts, cases, xs).  only = i: the draw stops after stream i (tools/debug_fuzz_case.py)."""
    layouts = _layouts()
    base = [ds.build_ensemble(10, lay, seed=500 + i) for i, lay in enumerate(layouts)]
    # what was transmitted, per layout and sub-channel: the logical frames and the super frames as byte strings
    draw_streams.tx_frames = [[{r.tobytes() for r in b.msc_bytes[j]} for j in range(len(b.subch))] for b in base]
    draw_streams.tx_superframes = [[{r.tobytes() for r in b.superframes[j]} if b.subch[j].dab_plus else set() for j in range(len(b.subch))] for b in base]
    rng = np.random.default_rng(seed)
    cases, xs = [], []
    for i in range(N_CASES):
        li = int(rng.integers(0, 3))
        snr = float(rng.uniform(3.5, 28.0))
        cfo = float(rng.uniform(-36000.0, 36000.0)) if i % 3 == 0 else float(rng.uniform(-2500.0, 2500.0))
        toff = int(rng.integers(0, ds.TF))
        gain = float(10 ** rng.uniform(-3.0, 1.5)) * 0.25
        if i % 7 == 4:                                    # a moving receiver: Rayleigh taps with Jakes Doppler, 5 .. 80 Hz, drifting sample clock
            snr = max(snr, 8.0)
            prof = ["TU6", "RA4", "SFN2", "HT6"][int(rng.integers(0, 4))]
            x = ds.channel_mobile(base[li].iq, prof, doppler_hz=float(rng.uniform(5.0, 80.0)), snr_db=snr, cfo_hz=cfo, timing_offset=toff,
                                  gain=gain, seed=700 + i, n_out=(N_FRAMES + 2) * ds.TF, clock_ppm=float(rng.uniform(-30.0, 30.0)),
                                  clock_drift_ppm_per_s=float(rng.uniform(-5.0, 5.0)))
        else:
            x = ds.channel(base[li].iq, snr_db=snr, cfo_hz=cfo, timing_offset=toff, gain=gain, seed=700 + i, n_out=(N_FRAMES + 2) * ds.TF)
        if i % 4 == 1:                                    # an echo inside the guard interval
            d = int(rng.integers(5, 400))
            x[d:] += np.complex64(rng.uniform(0.2, 0.8) * np.exp(1j * rng.uniform(0, 6.28))) * x[:-d].copy()
        if i % 5 == 2:                                    # a drop-out of 0.3 .. 2.5 frames somewhere after lock
            a = int(rng.uniform(7, 12) * ds.TF)
            x[a:a + int(rng.uniform(0.3, 2.5) * ds.TF)] *= np.float32(1e-3)
        if i % 6 == 3:                                    # sample-clock offset up to +-90 ppm (linear interpolation)
            ppm = float(os.environ.get("DABX_FUZZ_PPM", "90")) * 1e-6                            # 90 ppm of 4.7 M = 425 samples
            t = np.arange(len(x) - 1000, dtype=np.float64) * (1.0 + rng.uniform(-ppm, ppm))
            i0 = np.floor(t).astype(np.int64)
            fr = (t - i0).astype(np.float32)
            x = np.concatenate([(x[i0] * (1 - fr) + x[i0 + 1] * fr).astype(np.complex64), x[-1000:]])
        xs.append(np.ascontiguousarray(x, np.complex64))
        cases.append((li, snr, cfo, toff, gain))
        if only is not None and i == only:
            break
    return layouts, cases, xs, rng
