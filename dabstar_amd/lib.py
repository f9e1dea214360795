"""ctypes binding of libdabx.so (C ABI: include/dabx.h)."""
import ctypes as C
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class DabxError(RuntimeError):
    pass


def lib_path():
    """The product library.  DABX_LIB (read by this test/bench binding only -- the library itself reads no environment variable) names
    an experiment build instead (tools/build_variant.sh -> tools/_build/ab/*.so, same-box A/B runs of tools/ab.sh): nothing ever
    overwrites libdabx.so."""
    return os.environ.get("DABX_LIB") or os.path.join(HERE, "libdabx.so")


def load(build_if_missing=True):
    """Loads libdabx.so, building it in-tree with hipcc when absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if build_if_missing and not os.environ.get("DABX_LIB"):
        from . import build as _b
        if _b.needs_build():
            _b.build()
    if not os.path.exists(lib_path()):
        raise DabxError("libdabx.so is missing: run `python -m dabstar_amd.build` (needs hipcc)")
    L = C.CDLL(lib_path())
    L.dabx_last_error.restype = C.c_char_p
    for name in ("dabx_tii_destroy", "dabx_tii_reset"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = None
    L.dabx_tii_set_collisions.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.dabx_tii_add.argtypes = [C.c_void_p, C.c_void_p]
    L.dabx_tii_process.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    for name in ("dabx_convert_iq_bytes", "dabx_feed_bytes", "dabx_feed_bound"):
        getattr(L, name).restype = C.c_longlong
    L.dabx_feed_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.dabx_feed_bound.argtypes = [C.c_void_p, C.c_size_t]
    L.dabx_feed_close.argtypes = [C.c_void_p]
    L.dabx_convert_iq_bytes.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    # size_t arguments must not travel as C int (buffers of 2 GiB and more)
    L.dabx_push_iq.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t]
    L.dabx_push_iq_async.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t]
    L.dabx_push_wait.argtypes = [C.c_void_p]
    L.dabx_host_register.argtypes = [C.c_void_p, C.c_size_t]
    L.dabx_host_unregister.argtypes = [C.c_void_p]
    L.dabx_commit_iq.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    if hasattr(L, "dabx_delivery_next"):
        L.dabx_delivery_open.argtypes = [C.c_void_p, C.c_void_p]
        L.dabx_delivery_close.argtypes = [C.c_void_p]
        L.dabx_delivery_next.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.dabx_delivery_release.argtypes = [C.c_void_p, C.c_uint64]
        L.dabx_delivery_slab_bytes.argtypes = [C.c_void_p]
        L.dabx_delivery_wait_free.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dabx_delivery_slab_bytes.restype = C.c_longlong
    if hasattr(L, "dabx_set_packet_mode"):           # packet-mode data sub-channels
        L.dabx_set_packet_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_read_datagroups.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabx_get_packet_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_fibdec_packet_components.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    if hasattr(L, "dabx_set_pad_mode"):              # programme-associated data of DAB+ slots
        L.dabx_set_pad_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_read_pad_items.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabx_get_pad_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_set_mot_mode"):              # MOT objects of the X-PAD
        L.dabx_set_mot_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_read_mot_objects.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabx_get_mot_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_set_carousel_mode"):         # MOT objects of a packet-mode carousel
        L.dabx_set_carousel_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_get_carousel_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_set_data_mode"):             # TDC / IP / Journaline handlers of a packet-mode slot
        L.dabx_set_data_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_read_data_items.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabx_get_data_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_get_mp2_sync_stats"):        # ... and of DAB (MP2) audio slots
        L.dabx_get_mp2_sync_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_set_mp2_audio_mode"):        # MP2 audio of DAB audio slots
        L.dabx_set_mp2_audio_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_read_mp2_audio.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabx_get_mp2_audio_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_set_aac_stream_mode"):       # LOAS stream of DAB+ slots
        L.dabx_set_aac_stream_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_read_aac_frames.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
        L.dabx_get_aac_stream_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dabx_internal_aac_frame_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "dabx_announce_write"):            # (absent from libraries older than the level anchor: tools/ab.sh runs those through this binding too)
        L.dabx_announce_write.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    _LIB = L
    return L


def declared_symbols():
    """Every function name declared in include/dabx.h."""
    hdr = open(os.path.join(HERE, "..", "include", "dabx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(dabx_[a-z0-9_]+)\s*\(", hdr)))


def check(rc):
    if rc < 0:
        raise DabxError("libdabx error %d: %s" % (rc, load().dabx_last_error().decode()))
    return rc


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------- stage level
def viterbi(soft, nbits, tie_mode=0):
    """soft: [batch, 4*(nbits+6)] int16 -> [batch, nbits] uint8 (ViterbiSpiral::deconvolve); tie_mode 1 = the arithmetic of
    the reference's AVX2 / SSE2 builds."""
    soft = np.ascontiguousarray(soft, np.int16).reshape(-1, 4 * (nbits + 6))
    out = np.zeros((soft.shape[0], nbits), np.uint8)
    check(load().dabx_viterbi_mode(_p(soft), nbits, soft.shape[0], int(tie_mode), _p(out)))
    return out


def viterbi_lane_per_trellis(soft, nbits, tie_mode=0, always_clamp=False):
    """The same decode on the lane-per-trellis kernel of the MSC path (vit_t.hip) through the library's internal test entry
    (not part of include/dabx.h): unpunctured trellises, 64 per wavefront.  always_clamp forces the saturating step bodies of
    the tie modes in every cycle (must not change a bit)."""
    soft = np.ascontiguousarray(soft, np.int16).reshape(-1, 4 * (nbits + 6))
    out = np.zeros((soft.shape[0], nbits), np.uint8)
    check(load().dabx_internal_vitT(_p(soft), nbits, soft.shape[0], int(tie_mode), int(bool(always_clamp)), _p(out)))
    return out


def msc_inject(engine, stream, soft, first=0):
    """Internal test entry (not part of include/dabx.h): soft [n_cifs, 55296] int16 becomes the whole CIFs cif_no + first .. of
    `stream` in the engine's time-de-interleaver ring, converted as the demapper's output is (viterbi_tie_mode).  The stream's
    CIF counter only moves in msc_decode; first + n_cifs may not exceed one batch (28 CIFs)."""
    soft = np.ascontiguousarray(soft, np.int16).reshape(-1, 55296)
    check(load().dabx_internal_msc_inject(engine._h, int(stream), _p(soft), soft.shape[0], int(first)))


def msc_decode(engine, cifs_per_stream, batch_cifs):
    """Internal test entry: every stream counts cifs_per_stream[s] (0 .. batch_cifs) of its injected CIFs as received, then one MSC
    batch of batch_cifs CIFs runs exactly as dabx_process launches it (k_msc_prep + k_msc_vitT and / or k_msc_frame, DAB+ stage).
    Results: Engine.read_msc / Engine.subch_stats."""
    counts = np.ascontiguousarray(cifs_per_stream, np.int32).reshape(-1)
    if counts.size != engine.n_streams:
        raise ValueError("msc_decode needs one CIF count per stream")
    check(load().dabx_internal_msc_decode(engine._h, _p(counts), int(batch_cifs)))


def fic_inject(engine, stream, soft):
    """Internal test entry (not part of include/dabx.h): soft [9216] int16 becomes the FIC symbols of the next frame of `stream`,
    converted as the demapper's output is (viterbi_tie_mode).  Nothing is decoded before fic_decode_frame."""
    soft = np.ascontiguousarray(soft, np.int16).reshape(-1)
    if soft.size != 9216:
        raise ValueError("fic_inject needs the 9216 soft bits of one frame's FIC")
    check(load().dabx_internal_fic_inject(engine._h, int(stream), _p(soft)))


def fic_decode_frame(engine, present):
    """Internal test entry: k_fic_frame over all streams as the many-stream schedule launches it; present[s] = 0 means stream s has
    no frame (nothing of it may change), the others count the frame.  Results: Engine.read_fibs / Engine.stats."""
    present = np.ascontiguousarray(present, np.int32).reshape(-1)
    if present.size != engine.n_streams:
        raise ValueError("fic_decode_frame needs one flag per stream")
    check(load().dabx_internal_fic_decode(engine._h, _p(present)))


def demap_inject(engine, stream, spectra, null_fft=None, clock_err=0.0, np_sel=0):
    """Internal test entry (not part of include/dabx.h): spectra [76, 2048] complex64 in FFT bin order become the next frame of `stream`
    as the front end leaves it for the demapper -- symbol 0 the phase reference, symbols 1..75 the engine's spectra in carrier order --,
    clock_err and np_sel go into the stream's control record, and null_fft [2048] (optional) advances the noise-power buffer np_sel
    selects.  Nothing is demapped before demap_frame."""
    spectra = np.ascontiguousarray(spectra, np.complex64)
    if spectra.shape != (76, 2048):
        raise ValueError("demap_inject needs the 76 spectra of one frame")
    if null_fft is not None:
        null_fft = np.ascontiguousarray(null_fft, np.complex64).reshape(-1)
        if null_fft.size != 2048:
            raise ValueError("demap_inject: a null spectrum has 2048 bins")
    L = load()
    L.dabx_internal_demap_inject.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int]
    check(L.dabx_internal_demap_inject(engine._h, int(stream), _p(spectra), None if null_fft is None else _p(null_fft), float(clock_err), int(np_sel)))


def demap_frame(engine, present, schedule):
    """Internal test entry: the engine's demapper over all streams, launched as the front end launches it -- schedule 0: one
    k_demap_frame6(0, 75); 1: k_demap_fic, then k_demap_frame6(3, 75); 2: k_demap_whole -- in the instance the engine's soft-bit type,
    tie mode and LCD statistics select.  present[s] = 0: stream s has no frame (nothing of it may change).  Neither the CIF counter nor
    the frame count moves (fic_decode_frame / msc_decode do that).  Results: Engine.read_soft, Engine.stats."""
    present = np.ascontiguousarray(present, np.int32).reshape(-1)
    if present.size != engine.n_streams:
        raise ValueError("demap_frame needs one flag per stream")
    check(load().dabx_internal_demap_frame(engine._h, _p(present), int(schedule)))


FRONT_SCALARS = np.dtype([("frame_ok", "<i4"), ("np_sel", "<i4"), ("start_index", "<i4"), ("correction", "<i4"), ("f_frame", "<i4"),
                          ("phase_sym1", "<i4"), ("nco_phase", "<i4"), ("has_tii", "<i4"), ("frames", "<i8"), ("sym0_pos", "<u8"), ("rd", "<u8"),
                          ("f_sync", "<f4"), ("f_bb", "<f4"), ("phase_offs", "<f4"), ("clock_err", "<f4"), ("tii_cnt", "<i4", (2,)),
                          ("parity", "<i4"), ("pad_", "<i4")])     # dabx_front_scalars (csrc/engine_facade.cpp)
assert FRONT_SCALARS.itemsize == 88


def front_read(engine, stream, spectra=True):
    """Internal test entry (not part of include/dabx.h): what the frame chain (k_frame_head, k_symbols_persistent, k_frame_tail) of the
    last step left for `stream` of a drained engine, copied out without any kernel.  A dict of the control record's scalars (frame_ok,
    frames, sym0_pos, start_index, correction, f_frame, phase_sym1, nco_phase, f_sync, f_bb, phase_offs, clock_err, np_sel, rd, parity,
    tii_cnt) and phase_ref [2048] complex64 in bin order, spectra [75, 1536] complex64 in carrier order (spectra=False: left out),
    cp_part [75] complex64, abs_part [75] float32, null_power [2, 2048] float32 (both buffers; np_sel tells which is current) and
    tii_acc [2048] complex64 (None when the engine keeps no TII sum)."""
    sc = np.zeros(1, FRONT_SCALARS)
    phase_ref = np.zeros(2048, np.complex64)
    spec = np.zeros((75, 1536), np.complex64) if spectra else None
    cp_part = np.zeros(75, np.complex64)
    abs_part = np.zeros(75, np.float32)
    null_power = np.zeros((2, 2048), np.float32)
    tii_acc = np.zeros(2048, np.complex64)
    L = load()
    L.dabx_internal_front_read.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    check(L.dabx_internal_front_read(engine._h, int(stream), _p(sc), _p(phase_ref), None if spec is None else _p(spec), _p(cp_part), _p(abs_part),
                                     _p(null_power), _p(tii_acc)))
    out = {k: (sc[k][0].copy() if k == "tii_cnt" else sc[k][0].item()) for k in FRONT_SCALARS.names if k != "pad_"}
    out["f_bb"], out["f_sync"], out["clock_err"], out["phase_offs"] = (np.float32(sc[k][0]) for k in ("f_bb", "f_sync", "clock_err", "phase_offs"))
    out.update(phase_ref=phase_ref, spectra=spec, cp_part=cp_part, abs_part=abs_part, null_power=null_power,
               tii_acc=tii_acc if out["has_tii"] else None)
    return out


def dciq_read(engine, stream):
    """Internal test entry (not part of include/dabx.h): what k_dciq carries from launch to launch for `stream`, copied out without any
    kernel -> (state [5] float32: meanI, meanQ, meanII, meanQQ, meanIQ; done: the absolute index of the first sample not yet corrected)."""
    state = np.zeros(5, np.float32)
    done = C.c_uint64(0)
    L = load()
    L.dabx_internal_dciq_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    check(L.dabx_internal_dciq_read(engine._h, int(stream), _p(state), C.byref(done)))
    return state, int(done.value)


def fib_cif_count(fib32):
    """Internal, host only: (CIFCountHi, CIFCountLo) the library's FIG 0/0 walk reads out of one FIB of 32 bytes (CRC taken as good),
    or None -- the walk of k_fic_frame and of the ETI writer (csrc/fig00.h)."""
    fib32 = np.ascontiguousarray(fib32, np.uint8).reshape(-1)
    if fib32.size != 32:
        raise ValueError("a FIB has 32 bytes")
    hi, lo = C.c_int(-1), C.c_int(-1)
    return (hi.value, lo.value) if check(load().dabx_internal_fib_cif_count(_p(fib32), C.byref(hi), C.byref(lo))) else None


def profile_input_bits(kbps, prot_level, short_form=0):
    return check(load().dabx_profile_input_bits(kbps, prot_level, short_form))


def profile_map(kbps, prot_level, short_form=0):
    """Host only: (transmitted bits, index list as int32 with -1 for punctured positions)."""
    m = np.zeros(96 * kbps + 24, np.uint16)
    n = check(load().dabx_profile_map(kbps, prot_level, short_form, _p(m), m.size))
    out = m.astype(np.int32)
    out[m == 0xFFFF] = -1
    return n, out


def deconvolve(soft, kbps, prot_level, short_form=0):
    """soft: [batch, cu_size*64] int16 -> [batch, 24*kbps] uint8 (Protection::deconvolve)."""
    n_in = check(load().dabx_profile_input_bits(kbps, prot_level, short_form))
    soft = np.ascontiguousarray(soft, np.int16).reshape(-1, soft.shape[-1])
    assert soft.shape[1] >= n_in
    out = np.zeros((soft.shape[0], 24 * kbps), np.uint8)
    check(load().dabx_deconvolve(_p(soft), soft.shape[1], kbps, prot_level, short_form, soft.shape[0], _p(out)))
    return out


def rs_decode(cw):
    """cw: [batch,120] uint8 -> (out [batch,110], ret [batch] int16) (ReedSolomon::dec)."""
    cw = np.ascontiguousarray(cw, np.uint8).reshape(-1, 120)
    out = np.zeros((cw.shape[0], 110), np.uint8)
    ret = np.zeros(cw.shape[0], np.int16)
    check(load().dabx_rs_decode(_p(cw), cw.shape[0], _p(out), _p(ret)))
    return out, ret


def firecode_check(x):
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, 12)
    ok = np.zeros(x.shape[0], np.uint8)
    check(load().dabx_firecode_check(_p(x), x.shape[0], _p(ok)))
    return ok


def firecode_check_and_correct(x):
    x = np.ascontiguousarray(x, np.uint8).reshape(-1, 12).copy()
    ok = np.zeros(x.shape[0], np.uint8)
    check(load().dabx_firecode_check_and_correct(_p(x), x.shape[0], _p(ok)))
    return x, ok


def crc16_check(msgs, length):
    msgs = np.ascontiguousarray(msgs, np.uint8)
    ok = np.zeros(msgs.shape[0], np.uint8)
    check(load().dabx_crc16_check(_p(msgs), msgs.shape[1], length, msgs.shape[0], _p(ok)))
    return ok


def fft2048(x, inverse=False):
    x = np.ascontiguousarray(x, np.complex64).reshape(-1, 2048)
    out = np.zeros_like(x)
    check(load().dabx_fft2048(_p(x), x.shape[0], 1 if inverse else 0, _p(out)))
    return out


def prs_correlate(v, threshold, strongest=False):
    v = np.ascontiguousarray(v, np.complex64).reshape(-1, 2048)
    out = np.zeros(v.shape[0], np.int32)
    check(load().dabx_prs_correlate(_p(v), v.shape[0], C.c_float(threshold), int(strongest), _p(out)))
    return out


def coarse_cfo(fft0):
    fft0 = np.ascontiguousarray(fft0, np.complex64).reshape(-1, 2048)
    out = np.zeros(fft0.shape[0], np.int32)
    check(load().dabx_coarse_cfo(_p(fft0), fft0.shape[0], _p(out)))
    return out


class Demap:
    """Mirror of the reference's OfdmDecoder class surface (base/ofdm/ofdm_decoder.h:46-73), batched."""

    def __init__(self, batch=1):
        self.batch = batch
        self._h = C.c_void_p()
        check(load().dabx_demap_create(batch, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.dabx_demap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(load().dabx_demap_reset(self._h))

    def set_soft_bit_gen_type(self, t):
        check(load().dabx_demap_set_soft_bit_gen_type(self._h, t))

    def store_reference_symbol_0(self, fft):
        fft = np.ascontiguousarray(fft, np.complex64).reshape(self.batch, 2048)
        check(load().dabx_demap_store_reference_symbol_0(self._h, _p(fft)))

    def store_null_symbol_without_tii(self, fft):
        fft = np.ascontiguousarray(fft, np.complex64).reshape(self.batch, 2048)
        check(load().dabx_demap_store_null_symbol_without_tii(self._h, _p(fft)))

    def snr_db(self):
        out = np.zeros(self.batch, np.float32)
        check(load().dabx_demap_get_snr_db(self._h, _p(out)))
        return out

    def lcd_data(self):
        """(snr_db, mer_db, mean_value) of the LCD record, batch floats each (dabx_demap_get_lcd_data)."""
        out = [np.zeros(self.batch, np.float32) for _ in range(3)]
        load().dabx_demap_get_lcd_data.argtypes = [C.c_void_p] * 4
        check(load().dabx_demap_get_lcd_data(self._h, *[_p(o) for o in out]))
        return tuple(out)

    def decode_symbols(self, fft, clock_err):
        fft = np.ascontiguousarray(fft, np.complex64).reshape(self.batch, -1, 2048)
        ce = np.ascontiguousarray(np.broadcast_to(np.asarray(clock_err, np.float32), (self.batch,)))
        out = np.zeros((self.batch, fft.shape[1], 3072), np.int16)
        check(load().dabx_demap_decode_symbols(self._h, _p(fft), fft.shape[1], _p(ce), _p(out)))
        return out


# ---------------------------------------------------------------------------------- engine level
class Config(C.Structure):
    _fields_ = [("n_streams", C.c_int32), ("ring_frames", C.c_int32), ("max_subch", C.c_int32), ("out_frames", C.c_int32),
                ("sync_threshold", C.c_float), ("sync_strongest", C.c_int32), ("soft_bit_type", C.c_int32),
                ("fic_only", C.c_int32), ("capture_soft", C.c_int32), ("viterbi_tie_mode", C.c_int32), ("dc_iq_correction", C.c_int32),
                ("schedule", C.c_int32), ("msc_fast_min_jobs", C.c_int32), ("msc_class_min_jobs", C.c_int32),
                ("exact_level_tracker", C.c_int32), ("acquire_mode", C.c_int32)]


class SubchDesc(C.Structure):
    _fields_ = [("subch_id", C.c_int32), ("cu_start", C.c_int32), ("cu_size", C.c_int32), ("kbps", C.c_int32),
                ("prot_level", C.c_int32), ("short_form", C.c_int32), ("dab_plus", C.c_int32), ("reserved", C.c_int32)]


class SubchStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("start_cif", "cifs_decoded", "sf_count", "sf_ok", "sf_fail", "rs_corrected", "rs_failed",
                                         "fc_corrected", "au_ok", "au_bad")] + [("active", C.c_int32), ("subch_id", C.c_int32)]


class TiiResult(C.Structure):
    _fields_ = [("main_id", C.c_uint8), ("sub_id", C.c_uint8), ("strength", C.c_float), ("phase_deg", C.c_float),
                ("non_etsi_phase", C.c_int32)]

    def as_tuple(self):
        return (self.main_id, self.sub_id, self.strength, self.phase_deg, self.non_etsi_phase)


class TiiConfig(C.Structure):
    _fields_ = [("enable", C.c_int32), ("min_frames", C.c_int32), ("threshold_db", C.c_int32), ("collisions", C.c_int32),
                ("collision_sub_id", C.c_int32), ("reserved", C.c_int32 * 3)]          # dabx_tii_config


def _tii_tuples(res):
    """TII_RESULT records -> the tuples TiiResult.as_tuple gives"""
    return [(int(r["main_id"]), int(r["sub_id"]), float(r["strength"]), float(r["phase_deg"]), int(r["non_etsi_phase"])) for r in res]


class Tii:
    """Host-side TII detector (dabx_tii_*): TiiDetector of the reference."""

    def __init__(self):
        self._h = C.c_void_p()
        check(load().dabx_tii_create(C.byref(self._h)))

    def reset(self):
        load().dabx_tii_reset(self._h)

    def set_collisions(self, on, sub_id=0):
        load().dabx_tii_set_collisions(self._h, int(on), int(sub_id))

    def add(self, null_fft):
        v = np.ascontiguousarray(null_fft, np.complex64)
        assert v.size == 2048
        check(load().dabx_tii_add(self._h, _p(v)))

    def process(self, threshold_db, max_out=64):
        out = (TiiResult * max_out)()
        n = check(load().dabx_tii_process(self._h, int(threshold_db), out, max_out))
        return [out[i].as_tuple() for i in range(n)]

    def close(self):
        if self._h and _LIB is not None:
            _LIB.dabx_tii_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IqFormat(C.Structure):
    """dabx_iq_format: family 0 raw / 1 wav / 2 uff; container 0 u8, 1 s8, 2 i16, 3 i24, 4 i32, 5 f32."""
    _fields_ = [("family", C.c_int32), ("container", C.c_int32), ("big_endian", C.c_int32), ("swap_iq", C.c_int32),
                ("bits", C.c_int32), ("sample_rate", C.c_int32), ("data_offset", C.c_int64), ("data_bytes", C.c_int64),
                ("reference_quirks", C.c_int32), ("reserved", C.c_int32)]

    def sample_bytes(self):
        return 2 * (1, 1, 2, 3, 4, 4)[self.container]

    def as_tuple(self):
        """The probed description (family .. data_bytes); reference_quirks is a caller's switch, not part of it."""
        return tuple(getattr(self, k) for k, _ in self._fields_[:8])


class Stats(C.Structure):
    _fields_ = [("frames", C.c_int64), ("samples_consumed", C.c_int64), ("state", C.c_int32), ("fic_ratio_percent", C.c_int32),
                ("freq_offs_bb_hz", C.c_float), ("clock_err_hz", C.c_float), ("snr_db_est", C.c_float),
                ("last_start_index", C.c_int32), ("cif_count", C.c_int32),
                ("fib_ok", C.c_int64), ("fib_total", C.c_int64), ("sf_ok", C.c_int64), ("sf_fail", C.c_int64),
                ("rs_corrected", C.c_int64), ("rs_failed", C.c_int64), ("au_ok", C.c_int64), ("au_bad", C.c_int64),
                ("cifs_decoded", C.c_int64), ("signal_level", C.c_float), ("peak_level", C.c_float),
                ("level_margin_events", C.c_int64), ("level_rewalk_events", C.c_int64), ("level_unanchored_events", C.c_int64),
                ("level_healed_events", C.c_int64), ("fic_ber_bits", C.c_int64), ("fic_ber_errors", C.c_int64),
                ("mer_db_est", C.c_float), ("reserved_f", C.c_float), ("reserved", C.c_int64 * 1)]


# ---- bulk delivery (include/dabx.h "Bulk delivery"): the slab's records as numpy dtypes -----------------------------
CHUNK_FRAMES = 7
CHUNK_MAGIC = 0x43584244
DELIVER_FIB, DELIVER_MSC, DELIVER_SF, DELIVER_MSC_NOT_DABPLUS, DELIVER_DG, DELIVER_PAD, DELIVER_MOT = 1, 2, 4, 8, 16, 32, 64
CHUNK_HEADER = np.dtype([("magic", "<u4"), ("abi", "<u4"), ("seq", "<u8"), ("n_streams", "<i4"), ("max_subch", "<i4"),
                         ("max_frames", "<i4"), ("what", "<i4"), ("bytes", "<u8"), ("off_stream", "<u8"), ("off_subch", "<u8"),
                         ("off_fib", "<u8"), ("off_crc", "<u8"), ("off_frame", "<u8"), ("off_msc", "<u8"), ("off_sf", "<u8"),
                         ("off_dg", "<u8"), ("off_pad", "<u8"), ("off_mot", "<u8"), ("off_eti", "<u8")])
# the ETI section (DELIVER_ETI, opt-in: not part of what == 0): one record per stream, rows of ETI_FRAME_BYTES at rows_off
DELIVER_ETI = 128
ETI_FRAME_BYTES = 6144
CHUNK_ETI = np.dtype([("first_cif", "<i8"), ("n_eti", "<i4"), ("cifs_lost", "<i4"), ("cifs_waiting", "<i4"), ("cifs_refused", "<i4"),
                      ("cif_hi", "<i4"), ("cif_lo", "<i4"), ("rows_off", "<u8"), ("fib_frames", "<i8"), ("reserved", "<u8", 2)])
assert CHUNK_ETI.itemsize == 64
# the TII section (DELIVER_TII, opt-in like DELIVER_ETI): announced by the header's extension, which follows the header when `what` has a
# bit >= 256; one CHUNK_TII per stream, then 4 event slots per stream (a TII_EVENT + TII_MAX_RESULTS TII_RESULT records each)
DELIVER_TII = 256
TII_MAX_RESULTS = 32
CHUNK_EXT_MAGIC = 0x45584244                     # "DBXE"
CHUNK_HEADER_EXT = np.dtype({"names": ["magic", "bytes", "off_tii", "off_mp2_audio", "off_aac", "off_scope", "off_cir", "off_spectrum", "off_fig", "reserved"],
                             "formats": ["<u4", "<u4", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", "<u8", ("<u8", (1,))],
                             "offsets": [0, 4, 8, 16, 24, 32, 40, 48, 56, 56], "itemsize": 64})      # (off_fig is the last reserved word: one word, both names)
CHUNK_TII = np.dtype([("first_event", "<i8"), ("n_events", "<i4"), ("events_lost", "<i4"), ("ev_off", "<u8"), ("events_total", "<i8")])
TII_EVENT = np.dtype([("frame", "<i8"), ("n_results", "<i4"), ("n_found", "<i4"), ("frames_in_sum", "<i4"), ("epoch", "<i4"),
                      ("threshold_db", "<i4"), ("reserved", "<i4")])
TII_RESULT = np.dtype({"names": ["main_id", "sub_id", "strength", "phase_deg", "non_etsi_phase"], "formats": ["u1", "u1", "<f4", "<f4", "<i4"],
                       "offsets": [0, 1, 4, 8, 12], "itemsize": 16})          # dabx_tii_result, == TiiResult
TII_STATS = np.dtype([("events", "<i8"), ("results", "<i8"), ("truncated", "<i8"), ("resets", "<i8"), ("launches", "<i8"), ("reserved", "<i8", 3)])
TII_EVENT_SLOT_BYTES = 32 + 16 * TII_MAX_RESULTS
assert (CHUNK_HEADER_EXT.itemsize, CHUNK_TII.itemsize, TII_EVENT.itemsize, TII_RESULT.itemsize, TII_STATS.itemsize) == (64, 32, 32, 16, 64)
CHUNK_STREAM = np.dtype([("first_frame", "<i8"), ("n_frames", "<i4"), ("frames_lost", "<i4"), ("state", "<i4"),
                         ("fic_ratio_percent", "<i4"), ("cif_count", "<i4"), ("snr_db_est", "<f4"), ("freq_offs_bb_hz", "<f4"),
                         ("clock_err_hz", "<f4"), ("signal_level", "<f4"), ("fic_ber_bits", "<i4"), ("fic_ber_errors", "<i4"),
                         ("mer_db_est", "<f4"), ("fib_ok", "<i8"), ("fib_total", "<i8")])
CHUNK_FRAME = np.dtype([("sym0_pos", "<i8"), ("start_index", "<i4"), ("reserved", "<i4")])
CHUNK_SUBCH = np.dtype([("active", "<i4"), ("subch_id", "<i4"), ("kbps", "<i4"), ("dab_plus", "<i4"), ("start_cif", "<i8"),
                        ("first_cif", "<i8"), ("n_cifs", "<i4"), ("cifs_lost", "<i4"), ("first_sf", "<i8"), ("n_sf", "<i4"),
                        ("sf_lost", "<i4"), ("msc_off", "<u8"), ("sf_off", "<u8"), ("sf_pitch", "<i4"), ("reserved", "<i4"),
                        ("sf_ok", "<i8"), ("sf_fail", "<i8"), ("rs_corrected", "<i8"), ("rs_failed", "<i8"),
                        ("fc_corrected", "<i8"), ("au_ok", "<i8"), ("au_bad", "<i8"), ("sfi_off", "<u8")])
# dabx_superframe_info: what Mp4Processor::_process_super_frame knows when it hands the access units on (mp4processor.cpp:249-333)
SUPERFRAME_INFO = np.dtype([("num_aus", "u1"), ("au_crc_ok", "u1"), ("au_len_bad", "u1"), ("stream_parms", "u1"), ("au_start", "<u2", 7),
                            ("rs_corrected", "<u2"), ("rs_failed", "u1"), ("fc_corrected", "u1"), ("reserved", "<u2"), ("first_frame", "<i8")])
assert CHUNK_HEADER.itemsize == 128 and CHUNK_STREAM.itemsize == 72 and CHUNK_FRAME.itemsize == 16 and CHUNK_SUBCH.itemsize == 144
assert SUPERFRAME_INFO.itemsize == 32
# packet-mode data sub-channels (include/dabx.h): dabx_datagroup_info, one record per completed MSC data group, and dabx_packet_stats
DG_MAX_BYTES = 16384
DG_RING_MAX_BYTES = 131072                   # the largest byte ring of a slot (384 kbit/s: 56 logical frames + DG_MAX_BYTES, as a power of two)
DATAGROUP_INFO = np.dtype([("byte_pos", "<i8"), ("first_frame", "<i8"), ("last_frame", "<i8"), ("length", "<u2"), ("crc_flag", "u1"),
                           ("crc_ok", "u1"), ("reserved", "<u4")])
PACKET_COUNTERS = ("frames", "packets", "addr_match", "continuity_err", "crc_bad", "len_bad", "walk_short", "dg_count", "dg_bytes",
                   "dg_crc_bad", "dg_overflow")
PACKET_STATS = np.dtype([(k, "<i8") for k in PACKET_COUNTERS + ("dg_lost",)] + [("active", "<i4"), ("packet_address", "<i4"), ("reserved", "<i8", 3)])
PACKET_COMPONENT = np.dtype([("scid", "<i4"), ("subch_id", "<i4"), ("packet_address", "<i4"), ("dscty", "<i4"), ("dg_flag", "<i4"), ("sid", "<u4")])
# the slab's data-group section (dabx_chunk_dg): one row per (stream, slot), all zero for a slot that is not in packet mode
CHUNK_DG = np.dtype([("first_dg", "<i8"), ("n_dg", "<i4"), ("dg_lost", "<i4"), ("rec_off", "<u8"), ("bytes_off", "<u8"), ("n_bytes", "<i8")] +
                    [(k, "<i8") for k in PACKET_COUNTERS])
assert CHUNK_DG.itemsize == 128
assert DATAGROUP_INFO.itemsize == 32 and PACKET_STATS.itemsize == 128 and PACKET_COMPONENT.itemsize == 24
# programme-associated data (include/dabx.h): dabx_pad_item, one record per dynamic label / X-PAD MSC data group, and dabx_pad_stats
DL_MAX_BYTES = 256
PAD_LABEL, PAD_DATAGROUP = 1, 2
PAD_RING_BYTES = 131072                      # a PAD slot's byte ring
PAD_ITEM = np.dtype([("byte_pos", "<i8"), ("frame", "<i8"), ("length", "<u2"), ("kind", "u1"), ("au", "u1"), ("charset", "u1"),
                     ("crc_flag", "u1"), ("crc_ok", "u1"), ("reserved", "u1", 9)])
PAD_COUNTERS = ("superframes", "aus", "pad_aus", "fpad_other", "xpad_short", "xpad_variable", "xpad_other", "pad_bad", "labels", "label_bytes",
                "groups", "group_bytes", "li_bad", "dl_overflow", "dg_crc_bad", "dg_small")
PAD_STATS = np.dtype([(k, "<i8") for k in PAD_COUNTERS[:12] + ("items_lost",)] + [(k, "<i4") for k in PAD_COUNTERS[12:] + ("active", "reserved")])
# the slab's PAD section (dabx_chunk_pad): one row per (stream, slot), all zero for a slot without PAD decoding
CHUNK_PAD = np.dtype([("first_item", "<i8"), ("n_items", "<i4"), ("items_lost", "<i4"), ("item_off", "<u8"), ("bytes_off", "<u8"), ("n_bytes", "<i8")] +
                     [(k, "<i8") for k in ("superframes", "aus", "pad_aus", "pad_bad", "labels", "label_bytes", "groups", "group_bytes", "dg_crc_bad",
                                           "dl_overflow", "li_bad")])
assert PAD_ITEM.itemsize == 32 and PAD_STATS.itemsize == 128 and CHUNK_PAD.itemsize == 128
# PAD of DAB (MP2) audio frames: DABX_PAD_SOURCE_* and dabx_mp2_sync_stats (where Mp2Processor's frame sync of the slot stands)
PAD_SOURCES = {"dabplus": 0, "mp2": 1}
MP2_SEARCHING, MP2_GET_RATE, MP2_GET_DATA = 0, 1, 2
MP2_SYNC_STATS = np.dtype([(k, "<i8") for k in ("syncs", "frames", "hdr_refused", "rate_unsupported")] +
                          [(k, "<i4") for k in ("sample_rate", "state", "bit_count", "header_count", "last_sync_bit", "active")] + [("reserved", "<i4", 2)])
assert MP2_SYNC_STATS.itemsize == 64
# MP2 audio (include/dabx.h "MP2 audio"): dabx_mp2_audio_frame, one record per decoded MP2 frame with MP2_PCM_BYTES of PCM (1152 samples,
# interleaved L/R int16), dabx_mp2_audio_stats, and the slab's MP2 audio section (DELIVER_MP2_AUDIO, opt-in like DELIVER_ETI; announced by
# the header's extension): one CHUNK_MP2_AUDIO per (stream, slot), all zero for a slot without the mode
DELIVER_MP2_AUDIO = 512
MP2_PCM_BYTES = 4608
MP2_AUDIO_RING_BYTES = 512 * 1024
MP2_AUDIO_OVERREAD = 1                       # dabx_mp2_audio_frame.flags
MP2_AUDIO_FRAME = np.dtype([("byte_pos", "<i8"), ("frame", "<i8"), ("sample_rate", "<i4"), ("frame_size", "<i4"), ("header", "u1", 3),
                            ("stereo", "u1"), ("flags", "u1"), ("reserved", "u1", 3)])
MP2_AUDIO_STATS = np.dtype([(k, "<i8") for k in ("decode_calls", "frames_out", "bad_header", "refused", "overread", "launches")] +
                           [("sample_rate", "<i4"), ("frames_lost", "<i4")] + [(k, "<i2") for k in ("number_of_frames", "error_frames", "voffs", "active")])
CHUNK_MP2_AUDIO = np.dtype([("first_frame", "<i8"), ("n_frames", "<i4"), ("frames_lost", "<i4"), ("rec_off", "<u8"), ("bytes_off", "<u8"), ("n_bytes", "<i8")] +
                           [(k, "<i8") for k in ("decode_calls", "frames_out", "bad_header", "refused", "overread", "sample_rate", "voffs", "number_of_frames",
                                                 "error_frames")] + [("reserved", "<i8", 2)])
assert MP2_AUDIO_FRAME.itemsize == 32 and MP2_AUDIO_STATS.itemsize == 64 and CHUNK_MP2_AUDIO.itemsize == 128


class Mp2AudioConfig(C.Structure):
    """dabx_mp2_audio_config."""
    _fields_ = [("size", C.c_uint32), ("reserved", C.c_int32 * 7)]


# AAC stream (include/dabx.h "AAC stream"): dabx_aac_frame, one record per access unit of a DAB+ slot -- a LOAS/LATM frame of `length` bytes
# or, with length 0, a lost one (AAC_LOST_LEN / AAC_LOST_CRC: where the reference conceals) --, dabx_aac_stream_stats, and the slab's AAC
# section (DELIVER_AAC = 2048, opt-in like DELIVER_ETI; 1024 stays refused; announced by the header's extension): one CHUNK_AAC per
# (stream, slot), all zero for a slot without the mode
DELIVER_AAC = 2048
AAC_LOST_LEN, AAC_LOST_CRC = 1, 2            # dabx_aac_frame.flags
AAC_MAX_FRAME_BYTES = 974
AAC_FRAME = np.dtype([("byte_pos", "<i8"), ("first_frame", "<i8"), ("length", "<u2"), ("au_len", "<u2"), ("au", "u1"), ("num_aus", "u1"),
                      ("stream_parms", "u1"), ("flags", "u1"), ("reserved", "u1", 8)])
AAC_STREAM_STATS = np.dtype([(k, "<i8") for k in ("superframes", "records", "frames", "frame_bytes", "lost_len", "lost_crc", "launches", "lost")])
CHUNK_AAC = np.dtype([("first_frame", "<i8"), ("n_frames", "<i4"), ("frames_lost", "<i4"), ("rec_off", "<u8"), ("bytes_off", "<u8"), ("n_bytes", "<i8")] +
                     [(k, "<i8") for k in ("superframes", "records", "frames", "frame_bytes", "lost_len", "lost_crc")] + [("reserved", "<i8", 5)])
assert AAC_FRAME.itemsize == 32 and AAC_STREAM_STATS.itemsize == 64 and CHUNK_AAC.itemsize == 128


# IQ scope and carrier plots (include/dabx.h "IQ scope and carrier plots"): dabx_scope_record, one per shown symbol, with the IQ vector
# [1536] complex64 by nomCarrIdx and the carrier vector [1536] float32 by realCarrRelIdx behind it; dabx_scope_stats
SCOPE_CARRIERS = 1536
SCOPE_RECORD = np.dtype([("frame", "<i8"), ("symbol", "<i4"), ("iq_type", "u1"), ("carrier_type", "u1"), ("soft_bit_type", "u1"), ("reserved0", "u1"),
                         ("mean_value", "<f4"), ("mean_power_all", "<f4"), ("reserved", "<i4", 2)])
SCOPE_STATS = np.dtype([("shows", "<i8"), ("lost", "<i8"), ("launches", "<i8"), ("reserved", "<i8", 5)])
SCOPE_SLOT_BYTES = 32 + SCOPE_CARRIERS * 8 + SCOPE_CARRIERS * 4
# the slab's scope section (DELIVER_SCOPE = 8192, opt-in like DELIVER_ETI; 1024 and 4096 stay refused; announced by the header's extension):
# one CHUNK_SCOPE per stream, then CHUNK_FRAMES record slots for every stream that had the mode on when the delivery was opened
DELIVER_SCOPE = 8192
CHUNK_SCOPE = np.dtype([("first_record", "<i8"), ("n_records", "<i4"), ("records_lost", "<i4"), ("rec_off", "<u8"), ("records_total", "<i8")])
assert CHUNK_SCOPE.itemsize == 32
# EIqPlotType / ECarrierPlotType (glob_enums.h); the types the library refuses are left out
SCOPE_IQ_TYPES = {"PHASE_CORR_CARR_NORMED": 0, "PHASE_CORR_MEAN_NORMED": 1, "RAW_MEAN_NORMED": 2}
SCOPE_CARRIER_TYPES = {"SB_WEIGHT": 0, "EVM_PER": 1, "EVM_DB": 2, "STD_DEV": 3, "PHASE_ERROR": 4, "PRS_PHASE": 5, "PRS_PHASE_UNWRAP": 6,
                       "FOUR_QUAD_PHASE": 7, "REL_POWER": 8, "SNR": 9, "NULL_OVR_POW": 13}
assert SCOPE_RECORD.itemsize == 32 and SCOPE_STATS.itemsize == 64


# Channel impulse response and correlation plot (include/dabx.h "Channel impulse response and correlation plot"): dabx_cir_record, one per
# completed CIR window (kind 0: 385 values) or correlation show (kind 1: 2048 values, up to 69 indices), with the values [2048] float32 and the
# indices [72] int16 behind it; dabx_cir_stats
CIR_KIND_CIR, CIR_KIND_CORRELATION = 0, 1
CIR_ROWS = 385
CIR_WINDOW = 97 * 2048
CIR_PERIOD = 6 * 196608
CIR_CORR_LAGS = 2048
CIR_MAX_INDICES = 69
CIR_INDEX_ROOM = 72
CIR_RECORD = np.dtype([("frame", "<i8"), ("first_sample", "<i8"), ("threshold", "<f4"), ("rows_untrusted", "<i4"), ("n_values", "<i2"),
                       ("n_indices", "<i2"), ("kind", "u1"), ("reserved", "u1", 3)])
CIR_STATS = np.dtype([("shows", "<i8", 2), ("lost", "<i8"), ("rows_untrusted", "<i8"), ("launches", "<i8"), ("reserved", "<i8", 3)])
CIR_SLOT_BYTES = 32 + CIR_CORR_LAGS * 4 + CIR_INDEX_ROOM * 2
# the slab's CIR section (DELIVER_CIR = 32768, opt-in like DELIVER_SCOPE; 1024, 4096 and 16384 stay refused; announced by the header's
# extension): one CHUNK_CIR per stream, then CIR_CHUNK_RECORDS record slots for every stream that had the mode on when the delivery was opened
DELIVER_CIR = 32768
CIR_CHUNK_RECORDS = 4
CHUNK_CIR = np.dtype([("first_record", "<i8"), ("n_records", "<i4"), ("records_lost", "<i4"), ("rec_off", "<u8"), ("records_total", "<i8")])
assert CIR_RECORD.itemsize == 32 and CIR_STATS.itemsize == 64 and CHUNK_CIR.itemsize == 32


# RF spectrum and waterfall (include/dabx.h "RF spectrum and waterfall"): dabx_spectrum_record, one per show, with dabx_spectrum_limits_rec, db [512]
# float32 and row [512] uint8 behind it; dabx_spectrum_stats
SPECTRUM_BINS = 512
SPECTRUM_SIZE = 2048
SPECTRUM_PERIOD = 512000
SPECTRUM_RING = 8
SPECTRUM_AVERAGING = {"slow": 0, "medium": 1, "fast": 2}
SPECTRUM_RECORD = np.dtype([("frame", "<i8"), ("first_sample", "<i8"), ("untrusted", "<i4"), ("row_valid", "<i4"), ("inexact", "<i4"), ("reserved", "<i4")])
SPECTRUM_LIMITS = np.dtype([("glob_max", "<f4"), ("glob_min", "<f4"), ("loc_max", "<f4"), ("loc_min", "<f4"), ("y_min", "<f4"), ("y_max", "<f4"),
                            ("reserved", "<f4", 2)])
SPECTRUM_STATS = np.dtype([("shows", "<i8"), ("untrusted", "<i8"), ("lost", "<i8"), ("launches", "<i8"), ("inexact", "<i8"), ("reserved", "<i8", 3)])
SPECTRUM_SLOT_BYTES = 32 + 32 + SPECTRUM_BINS * 4 + SPECTRUM_BINS
# the slab's spectrum section (DELIVER_SPECTRUM = 65536, opt-in like DELIVER_CIR; 1024, 4096 and 16384 stay refused; announced by the header's
# extension): one CHUNK_SPECTRUM per stream, then SPECTRUM_CHUNK_RECORDS record slots for every stream that had the mode on when the delivery was opened
DELIVER_SPECTRUM = 65536
SPECTRUM_CHUNK_RECORDS = 6
CHUNK_SPECTRUM = np.dtype([("first_record", "<i8"), ("n_records", "<i4"), ("records_lost", "<i4"), ("rec_off", "<u8"), ("records_total", "<i8")])
assert SPECTRUM_RECORD.itemsize == 32 and SPECTRUM_LIMITS.itemsize == 32 and SPECTRUM_STATS.itemsize == 64 and CHUNK_SPECTRUM.itemsize == 32
# the FIC followed on the device (include/dabx.h, dabx_set_fig_mode): dabx_fig_label, dabx_fig_event (its payload as 8 words: fig_event_dict
# reads them by kind), dabx_fig_stats; the slab's FIG section (DELIVER_FIG = 262144, opt-in like DELIVER_SPECTRUM; 131072 stays refused like 1024, 4096 and 16384; announced by the header's
# extension): one CHUNK_FIG per stream, then FIG_CHUNK_RECORDS event slots for every stream that had the mode on when the delivery was opened
DELIVER_FIG = 262144
FIG_MAX_COMPONENTS, FIG_MAX_PACKETS, FIG_MAX_LABELS, FIG_MAX_EVENTS, FIG_CHUNK_RECORDS = 256, 64, 64, 256, 32
FIG_ANNOUNCE, FIG_SWAP, FIG_RESTART, FIG_TABLE, FIG_LABEL_EVENT = 1, 2, 3, 4, 5
FIG_LABEL = np.dtype([("id", "<u4"), ("char_flags", "<u2"), ("kind", "u1"), ("charset", "u1"), ("label", "u1", (16,)), ("pd", "u1"), ("scids", "u1"),
                      ("reserved", "u1", (6,))])
FIG_EVENT = np.dtype([("kind", "<i4"), ("epoch", "<i4"), ("frame", "<i8"), ("fib", "<i8"), ("cif", "<i8"), ("words", "<i4", (8,))])
FIG_COUNTERS = ("fibs_good", "fibs_bad", "figs", "end_markers", "fig_overrun", "fig_other_type", "fig0_other_ext", "fig00", "subch_new", "subch_known",
                "comp_new", "comp_known", "packet_new", "packet_known", "restarts", "swaps", "announces", "over_components", "over_packets",
                "over_labels", "label_new", "label_known", "label_charset", "label_short", "label_other_ext", "events", "launches")
FIG_STATS = np.dtype([(k, "<i8") for k in FIG_COUNTERS] + [("reserved", "<i8", (5,))])
CHUNK_FIG = np.dtype([("first_record", "<i8"), ("n_records", "<i4"), ("records_lost", "<i4"), ("rec_off", "<u8"), ("records_total", "<i8")])
assert (FIG_LABEL.itemsize, FIG_EVENT.itemsize, FIG_STATS.itemsize, CHUNK_FIG.itemsize) == (32, 64, 256, 32)


class FigConfig(C.Structure):
    _fields_ = [("enable", C.c_int32), ("reference_quirks", C.c_int32), ("service_info", C.c_int32), ("reserved", C.c_int32 * 1)]    # dabx_fig_config


def fig_label_dict(r):
    """A FIG_LABEL record as plain values (label: the 16 raw bytes)."""
    return dict(id=int(r["id"]), char_flags=int(r["char_flags"]), kind=int(r["kind"]), charset=int(r["charset"]), label=bytes(bytearray(r["label"])),
                pd=int(r["pd"]), scids=int(r["scids"]))


def fig_event_dict(ev):
    """A FIG_EVENT record as plain values: the head (kind, epoch, frame, fib, cif) and the payload its kind defines."""
    out = dict(kind=int(ev["kind"]), epoch=int(ev["epoch"]), frame=int(ev["frame"]), fib=int(ev["fib"]), cif=int(ev["cif"]))
    w = [int(v) for v in ev["words"]]
    if out["kind"] == FIG_ANNOUNCE:
        out.update(flags=w[0], occurrence_change=w[1], at_cif=(w[2] & 0xFFFFFFFF) | (w[3] << 32))
    elif out["kind"] == FIG_SWAP:
        out.update(n_changes=w[0], n_subch=w[1], n_components=w[2], n_packets=w[3])
    elif out["kind"] == FIG_TABLE:
        out.update(next=w[0], n_subch=w[1], n_components=w[2], n_packets=w[3])
    elif out["kind"] == FIG_LABEL_EVENT:
        out.update(label=fig_label_dict(np.array(ev["words"], "<i4").view(FIG_LABEL)[0]))
    elif out["kind"] == FIG_SI_TABLE:
        out.update(next=w[0], mask=w[1], n_global_defs=w[2], n_user_apps=w[3], n_fec=w[4], n_clusters=w[5], n_cluster_sids=w[6], n_languages=w[7] & 0xFFFF,
                   n_ptys=w[7] >> 16)
    elif out["kind"] == FIG_TIME:
        out.update(mjd=w[0], hour=w[1], minute=w[2], second=w[3], lto_minutes=w[4], utc_flag=w[5], lsi=w[6])
    elif out["kind"] in (FIG_ANNOUNCE_START, FIG_ANNOUNCE_STOP):
        out.update(cluster=w[0], flags=w[1], subch_id=w[2], n_services=w[3], next=w[4])
    return out


def _subch_dict(q):
    return {k: int(getattr(q, k)) for k in ("subch_id", "cu_start", "cu_size", "kbps", "prot_level", "short_form", "dab_plus")}


def _fig_rows(n, info, n_tab, subch, packets, n_labels, labels, stats, n_events, events):
    """the rows of dabx_fig_walk_device's outputs as one dict per decoder"""
    out = []
    for d in range(n):
        ne = int(n_events[d])
        out.append(dict(
            info={k: int(getattr(info[d], k)) for k, _ in FibdecInfo._fields_ if not k.startswith("reserved")},
            n_tab=n_tab[d].reshape(2, 3).tolist(),
            subch=[[_subch_dict(subch[(d * 2 + k) * 64 + i]) for i in range(int(n_tab[d, 3 * k]))] for k in range(2)],
            packets=[packets[d, k, :int(n_tab[d, 3 * k + 2])].copy() for k in range(2)],
            labels=[fig_label_dict(r) for r in labels[d, :int(n_labels[d])]],
            stats={k: int(stats[d][k]) for k in FIG_COUNTERS},
            n_events=ne,
            events=[fig_event_dict(e) for e in events[d, :min(ne, FIG_MAX_EVENTS)]]))
    return out


def _fig_out_buffers(n):
    return ((FibdecInfo * n)(), np.zeros((n, 6), np.int32), (SubchDesc * (n * 2 * 64))(), np.zeros((n, 2, FIG_MAX_PACKETS), PACKET_COMPONENT),
            np.zeros(n, np.int32), np.zeros((n, 4 * FIG_MAX_LABELS), FIG_LABEL), np.zeros(n, FIG_STATS), np.zeros(n, np.int64),
            np.zeros((n, FIG_MAX_EVENTS), FIG_EVENT))


def fig_walk_device(fibs, crc_ok, reference_quirks=False):
    """The FIG walk on the device, n fresh decoders in one call (a wave each, the device function of the engine's k_fig): fibs [n, n_fibs,
    32] uint8, crc_ok [n, n_fibs] -> one dict per decoder: info (as FibDecoder.info), n_tab [[current], [next]] x (sub-channels, components,
    packets), subch / packets of both configurations as the getters return them, labels, stats, n_events and the newest events."""
    fibs = np.ascontiguousarray(fibs, np.uint8)
    if fibs.ndim != 3 or fibs.shape[2] != 32:
        raise ValueError("fig_walk_device needs fibs [n, n_fibs, 32]")
    n, nf = fibs.shape[0], fibs.shape[1]
    crc_ok = np.ascontiguousarray(crc_ok, np.uint8).reshape(n, nf)
    bufs = _fig_out_buffers(n)
    info, n_tab, subch, packets, n_labels, labels, stats, n_events, events = bufs
    L = load()
    L.dabx_fig_walk_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 9
    check(L.dabx_fig_walk_device(_p(fibs), _p(crc_ok), n, nf, int(bool(reference_quirks)), info, _p(n_tab), subch, _p(packets), _p(n_labels), _p(labels),
                                 _p(stats), _p(n_events), _p(events)))
    return _fig_rows(n, *bufs)


def fig_timing(engine, on, max_launches=4096):
    """Internal measuring entry (tools/bench_fig.py): starts (on = True) or stops timing every k_fig launch with HIP events of its own;
    returns the milliseconds of the launches timed since the previous call, oldest first."""
    ms = np.zeros(max_launches, np.float32)
    L = load()
    L.dabx_internal_fig_timing.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    n = check(L.dabx_internal_fig_timing(engine._h, int(bool(on)), _p(ms), max_launches))
    return ms[:min(n, max_launches)].copy()


class FigHostDecoder:
    """Internal test entry (not part of include/dabx.h): the HOST build of the device's FIG walk (csrc/fig_core.h) on a decoder kept here as
    bytes.  walk(fibs, crc_ok) feeds FIBs, read() presents the decoder as one row of fig_walk_device.  Needs no device."""

    def __init__(self, reference_quirks=False):
        L = load()
        self._buf = np.zeros(L.dabx_internal_fig_host_bytes(), np.uint8)
        L.dabx_internal_fig_host_init.argtypes = [C.c_void_p, C.c_int]
        check(L.dabx_internal_fig_host_init(_p(self._buf), int(bool(reference_quirks))))

    def walk(self, fibs, crc_ok):
        fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
        crc_ok = np.ascontiguousarray(crc_ok, np.uint8).reshape(-1)
        L = load()
        L.dabx_internal_fig_host_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        check(L.dabx_internal_fig_host_walk(_p(self._buf), _p(fibs), _p(crc_ok), fibs.shape[0]))

    def read(self):
        bufs = _fig_out_buffers(1)
        info, n_tab, subch, packets, n_labels, labels, stats, n_events, events = bufs
        L = load()
        L.dabx_internal_fig_host_read.argtypes = [C.c_void_p] * 10
        check(L.dabx_internal_fig_host_read(_p(self._buf), info, _p(n_tab), subch, _p(packets), _p(n_labels), _p(labels), _p(stats), _p(n_events), _p(events)))
        return _fig_rows(1, *bufs)[0]


# the service information (include/dabx.h "Service information"; csrc/fig_si_core.h): the SI event kinds, the getters' records, the counters
# and the service directory's record
FIG_SI_TABLE, FIG_TIME, FIG_ANNOUNCE_START, FIG_ANNOUNCE_STOP = 6, 7, 8, 9
FIG_MAX_GLOBAL_DEFS, FIG_MAX_USER_APPS, FIG_MAX_LANGUAGES, FIG_MAX_PTYS, FIG_MAX_CLUSTERS, FIG_MAX_CLUSTER_SIDS, FIG_CLUSTER_LIST = 256, 128, 128, 128, 64, 512, 24
FIG_SI_HAS = dict(language=1, config=2, global_def=4, lto=8, user_apps=16, fec=32, pty=64, cluster=128)
FIG_JOIN = dict(subch=1, packet=2, global_def=4, user_apps=8, fec=16, language=32, pty=64, label=128)
FIG_SI_INFO = np.dtype([("has_config", "<i4", (2,)), ("n_services", "<i4", (2,)), ("count", "<i4", (2,)), ("has_lto", "<i4"), ("lto_minutes", "<i4"),
                        ("ecc", "<i4"), ("inter_table", "<i4"), ("lto_ext", "<i4"), ("time_set", "<i4"), ("mjd", "<i4"), ("hour", "<i4"), ("minute", "<i4"),
                        ("second", "<i4"), ("lsi", "<i4"), ("utc_flag", "<i4"), ("n_global_defs", "<i4", (2,)), ("n_user_apps", "<i4", (2,)),
                        ("n_fec", "<i4", (2,)), ("n_clusters", "<i4", (2,)), ("n_cluster_sids", "<i4", (2,)), ("n_languages", "<i4"), ("n_ptys", "<i4"),
                        ("reserved", "<i4", (2,))])
FIG_GLOBAL_DEF = np.dtype([("sid", "<u4"), ("scids", "i1"), ("pd", "i1"), ("ls", "i1"), ("ext", "i1"), ("subch_id", "<i2"), ("scid", "<i2")])
FIG_USER_APPS = np.dtype([("sid", "<u4"), ("size_bits", "<u2"), ("scids", "u1"), ("pd", "u1"), ("n_apps", "u1"), ("len", "u1", (6,)), ("reserved0", "u1"),
                          ("type", "<u2", (6,)), ("data", "u1", (6, 4)), ("reserved", "u1", (12,))])
FIG_LANGUAGE = np.dtype([("ls", "<i4"), ("id", "<i4"), ("language", "<i4"), ("reserved", "<i4")])
FIG_PTY = np.dtype([("sid", "<u4"), ("sd", "<i4"), ("code", "<i4"), ("reserved", "<i4")])
FIG_FEC = np.dtype([("subch_id", "<i4"), ("scheme", "<i4")])
FIG_CLUSTER = np.dtype([("cluster_id", "<i4"), ("flags", "<i4"), ("announcing", "<i4"), ("n_services", "<i4"), ("sid", "<u4", (FIG_CLUSTER_LIST,)),
                        ("reserved", "<i4", (4,))])
FIG_SI_COUNTERS = ("si_figs", "language_new", "language_known", "config_new", "config_known", "global_def_new", "global_def_known", "lto_new", "lto_known",
                   "time_set", "user_apps_new", "user_apps_known", "user_apps_clamped", "fec_new", "fec_known", "pty_new", "pty_known", "cluster_new",
                   "cluster_fallback", "cluster_zero", "cluster_sid_new", "cluster_sid_known", "asw_count", "asw_start", "asw_stop", "asw_unknown",
                   "over_global_defs", "over_user_apps", "over_languages", "over_ptys", "over_cluster_sids", "outside")
FIG_SI_STATS = np.dtype([(k, "<i8") for k in FIG_SI_COUNTERS])
FIG_SERVICE = np.dtype([("sid", "<u4"), ("comp_idx", "i1"), ("ps", "i1"), ("tmid", "i1"), ("ty", "i1"), ("scids", "i1"), ("subch_id", "i1"), ("prot_level", "i1"),
                        ("short_form", "i1"), ("cu_start", "<i2"), ("cu_size", "<i2"), ("kbps", "<i2"), ("packet_address", "<i2"), ("scid", "<i2"),
                        ("language", "<i2"), ("pty", "i1"), ("fec_scheme", "i1"), ("dg_flag", "i1"), ("pd", "i1"), ("n_apps", "u1"), ("app_len", "u1", (6,)),
                        ("reserved0", "u1"), ("app_type", "<u2", (6,)), ("app_data", "u1", (6, 4)), ("label", FIG_LABEL), ("joined", "<u4"),
                        ("reference_defined", "<i4"), ("reserved", "<i4", (4,))])
assert (FIG_SI_INFO.itemsize, FIG_GLOBAL_DEF.itemsize, FIG_USER_APPS.itemsize, FIG_LANGUAGE.itemsize, FIG_PTY.itemsize, FIG_FEC.itemsize, FIG_CLUSTER.itemsize,
        FIG_SI_STATS.itemsize, FIG_SERVICE.itemsize) == (128, 12, 64, 16, 16, 8, 128, 256, 128)


def _rec_dict(r, skip=("reserved", "reserved0")):
    """a numpy record as plain values (arrays as lists, nested records as dicts)"""
    out = {}
    for k in r.dtype.names:
        if k in skip:
            continue
        v = r[k]
        out[k] = fig_label_dict(v) if k == "label" else v.tolist() if isinstance(v, np.ndarray) else int(v)
    return out


def fig_user_apps_dict(r):
    """A FIG_USER_APPS record as plain values: its n_apps applications as (type, data length, the first four data bytes)."""
    n = int(r["n_apps"])
    return dict(sid=int(r["sid"]), scids=int(r["scids"]), pd=int(r["pd"]), size_bits=int(r["size_bits"]),
                apps=[(int(r["type"][k]), int(r["len"][k]), bytes(bytearray(r["data"][k]))) for k in range(n)])


def fig_service_dict(r):
    """A FIG_SERVICE record (dabx_fig_service) as plain values: the applications as in fig_user_apps_dict, the label as fig_label_dict or None."""
    out = _rec_dict(r, skip=("reserved", "reserved0", "app_len", "app_type", "app_data", "n_apps", "label"))
    out["apps"] = [(int(r["app_type"][k]), int(r["app_len"][k]), bytes(bytearray(r["app_data"][k]))) for k in range(int(r["n_apps"]))]
    out["label"] = None if int(r["label"]["kind"]) == 0xFF else fig_label_dict(r["label"])
    return out


def fig_cluster_dict(r):
    n = int(r["n_services"])
    return dict(cluster_id=int(r["cluster_id"]), flags=int(r["flags"]), announcing=int(r["announcing"]), n_services=n,
                sids=[int(v) for v in r["sid"][:min(n, FIG_CLUSTER_LIST)]])


def _fig_si_out_buffers(n):
    return (np.zeros(n, FIG_SI_INFO), np.zeros(n, FIG_SI_STATS), np.zeros((n, 2, FIG_MAX_GLOBAL_DEFS), FIG_GLOBAL_DEF), np.zeros((n, 2, FIG_MAX_USER_APPS), FIG_USER_APPS),
            np.zeros((n, 2, 64), FIG_FEC), np.zeros((n, 2, FIG_MAX_CLUSTERS), FIG_CLUSTER), np.zeros((n, FIG_MAX_LANGUAGES), FIG_LANGUAGE),
            np.zeros((n, FIG_MAX_PTYS), FIG_PTY), np.zeros((n, 2), np.int32), np.zeros((n, 2, FIG_MAX_COMPONENTS), FIG_SERVICE))


def _fig_si_rows(rows, si_info, si_stats, gd, ua, fec, cl, lang, pty, n_dir, dirs):
    """the SI outputs of dabx_fig_si_walk_device added to the rows of _fig_rows: row["si"] (the tables) and row["dir"] (both directories)"""
    for d, row in enumerate(rows):
        i = si_info[d]
        row["si"] = dict(
            info=_rec_dict(i), stats={k: int(si_stats[d][k]) for k in FIG_SI_COUNTERS},
            global_defs=[[_rec_dict(r) for r in gd[d, k, :int(i["n_global_defs"][k])]] for k in range(2)],
            user_apps=[[fig_user_apps_dict(r) for r in ua[d, k, :int(i["n_user_apps"][k])]] for k in range(2)],
            fec=[[(int(r["subch_id"]), int(r["scheme"])) for r in fec[d, k, :int(i["n_fec"][k])]] for k in range(2)],
            clusters=[[fig_cluster_dict(r) for r in cl[d, k, :int(i["n_clusters"][k])]] for k in range(2)],
            languages=[(int(r["ls"]), int(r["id"]), int(r["language"])) for r in lang[d, :int(i["n_languages"])]],
            ptys=[(int(r["sid"]), int(r["sd"]), int(r["code"])) for r in pty[d, :int(i["n_ptys"])]])
        row["dir"] = [[fig_service_dict(r) for r in dirs[d, k, :int(n_dir[d, k])]] for k in range(2)]
    return rows


def fig_si_walk_device(fibs, crc_ok, reference_quirks=False):
    """fig_walk_device with the service information followed (dabx_fig_si_walk_device: k_fig_si_batch, then k_fig_directory on both
    configurations): the rows of fig_walk_device, each with "si" (info, stats, global_defs / user_apps / fec / clusters of (current, next),
    languages, ptys) and "dir" (the service directory of (current, next), fig_service_dict)."""
    fibs = np.ascontiguousarray(fibs, np.uint8)
    if fibs.ndim != 3 or fibs.shape[2] != 32:
        raise ValueError("fig_si_walk_device needs fibs [n, n_fibs, 32]")
    n, nf = fibs.shape[0], fibs.shape[1]
    crc_ok = np.ascontiguousarray(crc_ok, np.uint8).reshape(n, nf)
    bufs, si = _fig_out_buffers(n), _fig_si_out_buffers(n)
    L = load()
    L.dabx_fig_si_walk_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 19
    check(L.dabx_fig_si_walk_device(_p(fibs), _p(crc_ok), n, nf, int(bool(reference_quirks)), *[b if isinstance(b, C.Array) else _p(b) for b in bufs + si]))
    return _fig_si_rows(_fig_rows(n, *bufs), *si)


class FigSiHostDecoder:
    """Internal test entry (not part of include/dabx.h): FigHostDecoder with the service information followed (csrc/fig_si_core.h on the
    host); read() presents the decoder as one row of fig_si_walk_device, the directory joined by the host build of the join.  No device."""

    def __init__(self, reference_quirks=False):
        L = load()
        self._buf = np.zeros(L.dabx_internal_fig_si_host_bytes(), np.uint8)
        L.dabx_internal_fig_si_host_init.argtypes = [C.c_void_p, C.c_int]
        check(L.dabx_internal_fig_si_host_init(_p(self._buf), int(bool(reference_quirks))))

    def walk(self, fibs, crc_ok):
        fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
        crc_ok = np.ascontiguousarray(crc_ok, np.uint8).reshape(-1)
        L = load()
        L.dabx_internal_fig_si_host_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        check(L.dabx_internal_fig_si_host_walk(_p(self._buf), _p(fibs), _p(crc_ok), fibs.shape[0]))

    def read(self):
        bufs, si = _fig_out_buffers(1), _fig_si_out_buffers(1)
        L = load()
        L.dabx_internal_fig_si_host_read.argtypes = [C.c_void_p] * 20
        check(L.dabx_internal_fig_si_host_read(_p(self._buf), *[b if isinstance(b, C.Array) else _p(b) for b in bufs + si]))
        return _fig_si_rows(_fig_rows(1, *bufs), *si)[0]


class SpectrumConfig(C.Structure):
    """dabx_spectrum_config."""
    _fields_ = [("enable", C.c_int32), ("averaging", C.c_int32), ("zoom_percent", C.c_int32), ("reserved", C.c_int32 * 5)]


def spectrum_rows_device(iq, state=None):
    """spectrum_viewer.cpp:169-218 on crafted windows (dabx_spectrum_rows_device): iq [n, 2048] complex64, one behind the other through one
    display buffer.  state = None: a fresh one (zeros), else [516] float32 from an earlier call.  -> (lin [n, 512], db [n, 512], ext [n, 4],
    state [516]): mYValVec, mDisplayBuffer behind each window, each window's extrema {glob max, glob min, loc max, loc min}."""
    iq = np.ascontiguousarray(iq, np.complex64).reshape(-1, SPECTRUM_SIZE)
    n = iq.shape[0]
    st = np.zeros(SPECTRUM_BINS + 4, np.float32) if state is None else np.array(state, np.float32).reshape(SPECTRUM_BINS + 4)
    lin = np.zeros((n, SPECTRUM_BINS), np.float32)
    db = np.zeros((n, SPECTRUM_BINS), np.float32)
    ext = np.zeros((n, 4), np.float32)
    L = load()
    L.dabx_spectrum_rows_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.dabx_spectrum_rows_device(_p(iq), n, _p(st), _p(lin), _p(db), _p(ext)))
    return lin, db, ext, st


def spectrum_limits(ext, limits, averaging="medium", zoom=0):
    """dabx_spectrum_limits, on the host: a show's extrema {glob max, glob min, loc max, loc min} into the four limits {Glob.Max, Glob.Min,
    Loc.Max, Loc.Min} -> (limits [4] float32, (yMin, yMax), row valid)."""
    e = np.array(ext, np.float32).reshape(4)
    l = np.array(limits, np.float32).reshape(4)
    y = np.zeros(2, np.float32)
    L = load()
    L.dabx_spectrum_limits.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    valid = check(L.dabx_spectrum_limits(_p(e), _p(l), SPECTRUM_AVERAGING.get(averaging, averaging), int(zoom), _p(y)))
    return l, (y[0], y[1]), bool(valid)


def spectrum_waterfall_row(db, y):
    """dabx_spectrum_waterfall_row, on the host: the colour indices of db for the range y = (yMin, yMax)."""
    d = np.ascontiguousarray(db, np.float32).reshape(-1)
    yy = np.array(y, np.float32).reshape(2)
    row = np.zeros(d.size, np.uint8)
    L = load()
    L.dabx_spectrum_waterfall_row.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    check(L.dabx_spectrum_waterfall_row(_p(d), d.size, _p(yy), _p(row)))
    return row


def spectrum_next_show(W, kind, a, b=0):
    """dabx_spectrum_next_show, on the host: the show position E of window W inside a searched range [a, b) (kind 0) or a frame whose
    symbol 0 ends at a (kind 1), or None."""
    L = load()
    L.dabx_spectrum_next_show.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64]
    L.dabx_spectrum_next_show.restype = C.c_int64
    E = L.dabx_spectrum_next_show(int(W), int(kind), int(a), int(b))
    if E < -1:
        check(int(E))
    return None if E < 0 else int(E)


def spectrum_look(walk, rd, state, sync_lost, frame_ok, sym0_pos):
    """dabx_spectrum_look, on the host: one look of k_spectrum.  walk = [W, pos, lost_seen, state_seen] -> (E or None, inexact, walk)."""
    w = np.array(walk, np.int64).reshape(4)
    inexact = C.c_int32(0)
    L = load()
    L.dabx_spectrum_look.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int64, C.c_int, C.c_uint64, C.c_void_p]
    L.dabx_spectrum_look.restype = C.c_int64
    E = L.dabx_spectrum_look(_p(w), int(rd), int(state), int(sync_lost), int(frame_ok), int(sym0_pos), C.byref(inexact))
    if E < -1:
        check(int(E))
    return (None if E < 0 else int(E)), inexact.value, w.tolist()


class CirConfig(C.Structure):
    """dabx_cir_config."""
    _fields_ = [("enable", C.c_int32), ("cir", C.c_int32), ("correlation", C.c_int32), ("reserved", C.c_int32 * 5)]


class ScopeConfig(C.Structure):
    """dabx_scope_config."""
    _fields_ = [("enable", C.c_int32), ("iq_type", C.c_int32), ("carrier_type", C.c_int32), ("symbol", C.c_int32), ("reserved", C.c_int32 * 4)]


class AacStreamConfig(C.Structure):
    """dabx_aac_stream_config."""
    _fields_ = [("size", C.c_uint32), ("format", C.c_int32), ("reserved", C.c_int32 * 6)]


def aac_ring_bytes(kbps):
    """Size of the byte ring of an AAC stream slot: the next power of two >= two batches of in-order super frames."""
    n = 1
    while n < 2 * 6 * (110 * (kbps // 8) + 72):
        n <<= 1
    return n


def aac_frame_host(au, stream_parms):
    """The LOAS frame (uint8 array) of one access unit of len(au) <= 960 bytes, built on the host by the pieces of k_aac_stream lane after
    lane (dabx_internal_aac_frame_host: a test entry, not part of include/dabx.h).  Needs no device."""
    au = np.ascontiguousarray(au, np.uint8)
    out = np.zeros(AAC_MAX_FRAME_BYTES, np.uint8)
    n = check(load().dabx_internal_aac_frame_host(_p(au) if len(au) else None, len(au), int(stream_parms), _p(out)))
    return out[:n].copy()


# MOT objects of the X-PAD (include/dabx.h): dabx_mot_object, one record per signal_new_mot_object, dabx_mot_stats and the slab's MOT
# section (dabx_chunk_mot): one row per (stream, slot), all zero for a slot without MOT decoding
MOT_OBJECT_BYTES_DEFAULT = 65536
MOT_NAME_ROOM = 8192
MOT_OBJECT = np.dtype([("byte_pos", "<i8"), ("frame", "<i8"), ("body_len", "<u4"), ("body_size", "<u4"), ("transport_id", "<u2"),
                       ("content_type", "<u2"), ("name_len", "<u2"), ("au", "u1"), ("repeat", "u1")])
MOT_COUNTERS = ("objects", "object_bytes", "groups", "headers", "segments", "crc_bad", "type_other", "no_tid", "grp_short", "hdr_bad",
                "seg_number_bad", "seg_duplicate", "resets", "obj_overflow", "pad_overrun", "progress_events", "progress_pct", "transport_id",
                "segments_stored")
MOT_STATS = np.dtype([(k, "<i8") for k in ("objects", "object_bytes", "objects_lost", "groups", "headers", "segments")] +
                     [(k, "<i4") for k in MOT_COUNTERS[5:] + ("active",)] + [("reserved", "<i4", 5)])
CHUNK_MOT = np.dtype([("first_object", "<i8"), ("n_objects", "<i4"), ("objects_lost", "<i4"), ("rec_off", "<u8"), ("bytes_off", "<u8"), ("n_bytes", "<i8")] +
                     [(k, "<i8") for k in ("objects", "object_bytes", "groups", "headers", "segments", "crc_bad", "grp_short", "hdr_bad", "obj_overflow",
                                           "resets", "progress_events")])
assert MOT_OBJECT.itemsize == 32 and MOT_STATS.itemsize == 128 and CHUNK_MOT.itemsize == 128


# MOT objects of a packet-mode carousel (include/dabx.h): the records are MOT_OBJECT -- `frame` is the last_frame of the data group that
# completed the object and `au` carries flags --, dabx_carousel_stats, and the slot's row of the slab's MOT section is a CHUNK_MOT
MOT_FLAG_DIR_ELEMENT = 1
CAROUSEL_DIR_OBJECTS_DEFAULT = 49
CAROUSEL_DIR_BYTES_DEFAULT = 65536
CAROUSEL_COUNTERS = ("objects", "object_bytes", "groups", "headers", "segments", "crc_bad", "type_other", "no_tid", "grp_short", "hdr_bad",
                     "seg_number_bad", "seg_duplicate", "resets", "obj_overflow", "hdr_known", "hdr_not_first", "from_body", "evictions",
                     "dirs_begun", "dirs_repeated", "dirs_refused", "dir_segments", "dir_objects", "dir_short", "dir_seg_bad", "dir_cut",
                     "dg_overrun")
CAROUSEL_STATS = np.dtype([(k, "<i8") for k in ("objects", "object_bytes", "objects_lost")] +
                          [(k, "<i4") for k in CAROUSEL_COUNTERS[2:] + ("active",)])
assert CAROUSEL_STATS.itemsize == 128


class CarouselConfig(C.Structure):
    """dabx_carousel_config."""
    _fields_ = [("size", C.c_uint32), ("max_object_bytes", C.c_uint32), ("max_dir_objects", C.c_uint32), ("max_dir_bytes", C.c_uint32),
                ("reserved", C.c_int32 * 4)]


# The data handlers of a packet-mode slot (include/dabx.h): dabx_data_item, one record per TDC frame, UDP payload or NML object, and
# dabx_data_stats: one int64 per decision and guard
DATA_HANDLERS = {"tdc": 1, "ip": 2, "journaline": 3}
DATA_HANDLER_MOT = 4
DATA_TDC_0, DATA_TDC_1, DATA_UDP, DATA_NML = 1, 2, 3, 4
DATA_CRC_OK, DATA_NEW_REVISION = 1, 2
DATA_ITEM = np.dtype([("byte_pos", "<i8"), ("frame", "<i8"), ("length", "<u2"), ("kind", "u1"), ("flags", "u1"), ("a", "<u2"), ("b", "<u2"),
                      ("group", "<u4"), ("reserved", "<u4")])
DATA_COUNTERS = ("groups", "items", "bytes", "dg_overrun", "walk_end", "tdc_cut", "tdc_len_bad", "tdc_hdr_crc_bad", "tdc_crc0_bad", "tdc_crc0_short",
                 "tdc_type_other", "ip_dg_crc_bad", "ip_len_bad", "ip_not_v4", "ip_checksum_bad", "ip_proto_other", "ip_short", "jl_hdr_short",
                 "jl_segmented", "jl_empty", "jl_len_bad", "jl_crc_bad", "jl_no_crc", "jl_type_other", "nml_too_long", "nml_short", "nml_type_bad",
                 "nml_repeat")
DATA_STATS = np.dtype([(k, "<i8") for k in DATA_COUNTERS[:3] + ("lost",) + DATA_COUNTERS[3:] + ("launches", "active", "handler")])
# ... in bulk: DELIVER_DATA = 524288 (opt-in like DELIVER_FIG; 1024, 4096, 16384 and 131072 stay refused), announced by a SECOND extension of
# the header at byte 192 (CHUNK_HEADER_EXT2; off_stream is then 256), one CHUNK_DATA per (stream, slot)
DELIVER_DATA = 524288
CHUNK_EXT2_MAGIC = 0x32584244                    # "DBX2"
CHUNK_HEADER_EXT2 = np.dtype([("magic", "<u4"), ("bytes", "<u4"), ("off_data", "<u8"), ("reserved", "<u8", 6)])
CHUNK_DATA = np.dtype([("first_item", "<i8"), ("n_items", "<i4"), ("items_lost", "<i4"), ("rec_off", "<u8"), ("bytes_off", "<u8"), ("n_bytes", "<i8")] +
                      [(k, "<i8") for k in ("groups", "items", "bytes")] + [("reserved", "<i8", 8)])
assert DATA_ITEM.itemsize == 32 and DATA_STATS.itemsize == 256 and CHUNK_HEADER_EXT2.itemsize == 64 and CHUNK_DATA.itemsize == 128


class DataConfig(C.Structure):
    """dabx_data_config."""
    _fields_ = [("size", C.c_uint32), ("handler", C.c_int32), ("only_new_revisions", C.c_int32), ("reserved", C.c_int32 * 5)]


def data_handler_for(dscty, app_type):
    """dabx_data_handler_for: DATA_HANDLERS' value, DATA_HANDLER_MOT or 0 for a packet-mode component (data_processor.cpp:53-101)."""
    return int(load().dabx_data_handler_for(int(dscty), int(app_type)))


def data_walk(handler, records, group_bytes, only_new_revisions=False, device=False, max_items=4096, out_cap=1 << 20):
    """One slot's crafted data groups through a handler without an engine (dabx_internal_data_walk_host / _device: test entries, not part of
    include/dabx.h): records [n] DATAGROUP_INFO with byte_pos into group_bytes.  device = False: the host build of the handlers, needs no
    device; True: k_data_batch, the body of the engine's k_data_handler.  Returns (items [k] DATA_ITEM, their bytes, stats dict)."""
    L = load()
    call = L.dabx_internal_data_walk_device if device else L.dabx_internal_data_walk_host
    call.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    records = np.ascontiguousarray(records, DATAGROUP_INFO)
    group_bytes = np.ascontiguousarray(group_bytes, np.uint8)
    items, out, st = np.zeros(max_items, DATA_ITEM), np.zeros(out_cap, np.uint8), np.zeros(1, DATA_STATS)
    k = check(call(DATA_HANDLERS[handler] if isinstance(handler, str) else int(handler), int(bool(only_new_revisions)), len(records),
                   _p(records) if len(records) else None, _p(group_bytes) if len(group_bytes) else None, len(group_bytes), max_items, _p(items), _p(out), out_cap,
                   _p(st)))
    items = items[:k].copy()
    return items, out[:int(items["length"].sum())].copy(), {n: int(st[0][n]) for n in DATA_STATS.names}


def data_timing(engine, on, max_launches=4096):
    """Measuring entry (dabx_internal_data_timing; not part of include/dabx.h): on = True, every k_data_handler launch from now on lies between
    two HIP events of its own; on = False: the times (ms, float32) of the launches made since, oldest first."""
    ms = np.zeros(max_launches, np.float32)
    L = load()
    L.dabx_internal_data_timing.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    n = check(L.dabx_internal_data_timing(engine._h, int(bool(on)), _p(ms), max_launches))
    return ms[:min(n, max_launches)].copy()


class MotConfig(C.Structure):
    """dabx_mot_config."""
    _fields_ = [("size", C.c_uint32), ("max_object_bytes", C.c_uint32), ("reserved", C.c_int32 * 6)]


class PadConfig(C.Structure):
    """dabx_pad_config."""
    _fields_ = [("size", C.c_uint32), ("source", C.c_int32), ("reserved", C.c_int32 * 6)]


class PacketConfig(C.Structure):
    """dabx_packet_config."""
    _fields_ = [("size", C.c_uint32), ("packet_address", C.c_int32), ("reserved", C.c_int32 * 6)]


class DeliveryConfig(C.Structure):
    _fields_ = [("host_slabs", C.c_int32), ("what", C.c_int32), ("copy_engine", C.c_int32), ("reserved", C.c_int32 * 5)]


class IngestConfig(C.Structure):
    _fields_ = [("host_slabs", C.c_int32), ("fmt", C.c_int32), ("max_frames", C.c_int32), ("copy_engine", C.c_int32), ("reserved", C.c_int32 * 4)]


class DeliveryInfo(C.Structure):
    _fields_ = [("chunks_closed", C.c_uint64), ("chunks_landed", C.c_uint64), ("bytes_copied", C.c_uint64), ("copy_seconds", C.c_double),
                ("copy_seconds_max", C.c_double), ("gather_wait_seconds", C.c_double), ("copy_engine", C.c_int32),
                ("sdma_engine_mask", C.c_uint32), ("calibration_GBps", C.c_double), ("reserved", C.c_uint64 * 3)]


class ChunkRef(C.Structure):
    _fields_ = [("seq", C.c_uint64), ("data", C.c_void_p), ("bytes", C.c_uint64)]


class Chunk:
    """One delivered slab, viewed in place (no copy): valid until release()."""

    def __init__(self, engine, ref):
        self._eng, self.seq, self.nbytes = engine, ref.seq, ref.bytes
        self.raw = np.ctypeslib.as_array(C.cast(ref.data, C.POINTER(C.c_uint8)), shape=(ref.bytes,))
        self.header = self.raw[:128].view(CHUNK_HEADER)[0]
        h = self.header
        assert h["magic"] == CHUNK_MAGIC and h["bytes"] == ref.bytes, (hex(int(h["magic"])), int(h["bytes"]), ref.bytes)
        S, M, F = int(h["n_streams"]), int(h["max_subch"]), int(h["max_frames"])
        self.S, self.M, self.F = S, M, F
        self.streams = self.raw[int(h["off_stream"]):int(h["off_stream"]) + S * 72].view(CHUNK_STREAM)
        self.subch = self.raw[int(h["off_subch"]):int(h["off_subch"]) + S * M * 144].view(CHUNK_SUBCH).reshape(S, M)
        if h["what"] & DELIVER_FIB:
            self.fibs = self.raw[int(h["off_fib"]):int(h["off_fib"]) + S * F * 384].reshape(S, F, 12, 32)
            self.crc = self.raw[int(h["off_crc"]):int(h["off_crc"]) + S * F * 12].reshape(S, F, 12)
            self.frames = self.raw[int(h["off_frame"]):int(h["off_frame"]) + S * F * 16].view(CHUNK_FRAME).reshape(S, F)
        self.dg = None                          # the data-group section: [S, M] CHUNK_DG, or None when the slab has none
        if int(h["off_dg"]):
            self.dg = self.raw[int(h["off_dg"]):int(h["off_dg"]) + S * M * 128].view(CHUNK_DG).reshape(S, M)
        self.pad = None                         # the PAD section: [S, M] CHUNK_PAD, or None when the slab has none
        if int(h["off_pad"]):
            self.pad = self.raw[int(h["off_pad"]):int(h["off_pad"]) + S * M * 128].view(CHUNK_PAD).reshape(S, M)
        self.mot = None                         # the MOT section: [S, M] CHUNK_MOT, or None when the slab has none
        if int(h["off_mot"]):
            self.mot = self.raw[int(h["off_mot"]):int(h["off_mot"]) + S * M * 128].view(CHUNK_MOT).reshape(S, M)
        self.header_ext = None                  # the header's extension (CHUNK_HEADER_EXT) when `what` has a bit >= 256, else None
        self.tii_table = None                   # the TII section: [S] CHUNK_TII, or None when the slab has none
        self.mp2_audio_table = None             # the MP2 audio section: [S, M] CHUNK_MP2_AUDIO, or None when the slab has none
        self.aac_table = None                   # the AAC section: [S, M] CHUNK_AAC, or None when the slab has none
        self.scope_table = None                 # the scope section: [S] CHUNK_SCOPE, or None when the slab has none
        self.cir_table = None                   # the CIR section: [S] CHUNK_CIR, or None when the slab has none
        self.spectrum_table = None              # the spectrum section: [S] CHUNK_SPECTRUM, or None when the slab has none
        self.fig_table = None                   # the FIG section: [S] CHUNK_FIG, or None when the slab has none
        if int(h["what"]) & ~255:
            self.header_ext = self.raw[128:192].view(CHUNK_HEADER_EXT)[0]
            if int(self.header_ext["magic"]) != CHUNK_EXT_MAGIC or int(self.header_ext["bytes"]) < 64:
                raise DabxError("chunk %d: bad header extension" % self.seq)
            if int(self.header_ext["off_tii"]):
                o = int(self.header_ext["off_tii"])
                self.tii_table = self.raw[o:o + S * 32].view(CHUNK_TII)
            if int(self.header_ext["off_mp2_audio"]):
                o = int(self.header_ext["off_mp2_audio"])
                self.mp2_audio_table = self.raw[o:o + S * M * 128].view(CHUNK_MP2_AUDIO).reshape(S, M)
            if int(self.header_ext["off_aac"]):
                o = int(self.header_ext["off_aac"])
                self.aac_table = self.raw[o:o + S * M * 128].view(CHUNK_AAC).reshape(S, M)
            if int(self.header_ext["off_scope"]):
                o = int(self.header_ext["off_scope"])
                self.scope_table = self.raw[o:o + S * 32].view(CHUNK_SCOPE)
            if int(self.header_ext["off_cir"]):
                o = int(self.header_ext["off_cir"])
                self.cir_table = self.raw[o:o + S * 32].view(CHUNK_CIR)
            if int(self.header_ext["off_spectrum"]):
                o = int(self.header_ext["off_spectrum"])
                self.spectrum_table = self.raw[o:o + S * 32].view(CHUNK_SPECTRUM)
            if int(self.header_ext["off_fig"]):
                o = int(self.header_ext["off_fig"])
                self.fig_table = self.raw[o:o + S * 32].view(CHUNK_FIG)
        self.header_ext2 = None                 # the second extension (CHUNK_HEADER_EXT2) when `what` has DELIVER_DATA, else None
        self.data_table = None                  # the data section: [S, M] CHUNK_DATA, or None when the slab has none
        if int(h["what"]) & DELIVER_DATA:
            self.header_ext2 = self.raw[192:256].view(CHUNK_HEADER_EXT2)[0]
            if int(self.header_ext2["magic"]) != CHUNK_EXT2_MAGIC or int(self.header_ext2["bytes"]) < 64:
                raise DabxError("chunk %d: bad second header extension" % self.seq)
            if int(self.header_ext2["off_data"]):
                o = int(self.header_ext2["off_data"])
                self.data_table = self.raw[o:o + S * M * 128].view(CHUNK_DATA).reshape(S, M)
        self.eti_table = None                  # the ETI section: [S] CHUNK_ETI, or None when the slab has none
        if int(h["off_eti"]):
            self.eti_table = self.raw[int(h["off_eti"]):int(h["off_eti"]) + S * 64].view(CHUNK_ETI)

    def tii(self, stream):
        """TII events of `stream` in this chunk, oldest first: a list of (TII_EVENT record, its results[:n_results] as TII_RESULT records),
        views.  Empty when the slab has no TII section."""
        if self.tii_table is None:
            return []
        r = self.tii_table[stream]
        out = []
        for k in range(int(r["n_events"])):
            o = int(r["ev_off"]) + k * TII_EVENT_SLOT_BYTES
            ev = self.raw[o:o + 32].view(TII_EVENT)[0]
            out.append((ev, self.raw[o + 32:o + 32 + 16 * int(ev["n_results"])].view(TII_RESULT)))
        return out

    @staticmethod
    def _record_slots(table, stream, slot_bytes):
        """Where the record slots of `stream` lie in the slab, oldest first, by its row of a scope / CIR / spectrum section's table (None: the
        slab has no such section)."""
        if table is None:
            return []
        r = table[stream]
        return [int(r["rec_off"]) + k * slot_bytes for k in range(int(r["n_records"]))]

    def scope(self, stream):
        """Scope records of `stream` in this chunk, oldest first: a list of (SCOPE_RECORD record, iq [1536] complex64, carr [1536] float32),
        views.  Empty when the slab has no scope section or the stream had the mode off when the delivery was opened."""
        return [(self.raw[o:o + 32].view(SCOPE_RECORD)[0], self.raw[o + 32:o + 32 + SCOPE_CARRIERS * 8].view(np.complex64),
                 self.raw[o + 32 + SCOPE_CARRIERS * 8:o + SCOPE_SLOT_BYTES].view(np.float32))
                for o in self._record_slots(self.scope_table, stream, SCOPE_SLOT_BYTES)]

    def cir(self, stream):
        """CIR / correlation records of `stream` in this chunk, oldest first: a list of (CIR_RECORD record, values[:n_values] float32,
        indices[:n_indices] int16), views.  Empty when the slab has no CIR section or the stream had the mode off when the delivery was opened."""
        out = []
        for o in self._record_slots(self.cir_table, stream, CIR_SLOT_BYTES):
            rec = self.raw[o:o + 32].view(CIR_RECORD)[0]
            out.append((rec, self.raw[o + 32:o + 32 + 4 * int(rec["n_values"])].view(np.float32),
                        self.raw[o + 32 + CIR_CORR_LAGS * 4:o + 32 + CIR_CORR_LAGS * 4 + 2 * int(rec["n_indices"])].view(np.int16)))
        return out

    def spectrum(self, stream):
        """Spectrum records of `stream` in this chunk, oldest first: a list of (SPECTRUM_RECORD record, SPECTRUM_LIMITS record, db [512]
        float32, row [512] uint8), views.  Empty when the slab has no spectrum section or the stream had the mode off when the delivery was opened."""
        return [(self.raw[o:o + 32].view(SPECTRUM_RECORD)[0], self.raw[o + 32:o + 64].view(SPECTRUM_LIMITS)[0],
                 self.raw[o + 64:o + 64 + 4 * SPECTRUM_BINS].view(np.float32), self.raw[o + 64 + 4 * SPECTRUM_BINS:o + SPECTRUM_SLOT_BYTES])
                for o in self._record_slots(self.spectrum_table, stream, SPECTRUM_SLOT_BYTES)]

    def fig(self, stream):
        """FIG change events of `stream` in this chunk, oldest first: a list of dicts (fig_event_dict).  Empty when the slab has no FIG section
        or the stream had the mode off when the delivery was opened."""
        return [fig_event_dict(self.raw[o:o + 64].view(FIG_EVENT)[0]) for o in self._record_slots(self.fig_table, stream, 64)]

    def eti(self, stream):
        """ETI(NI) frames of `stream` in this chunk: (its CHUNK_ETI record, [n_eti, 6144] uint8), views; the rows are contiguous and in CIF
        order -- rows.tobytes() is a piece of a raw ETI(NI) stream.  (None, empty) when the slab has no ETI section."""
        if self.eti_table is None:
            return None, np.zeros((0, ETI_FRAME_BYTES), np.uint8)
        r = self.eti_table[stream]
        o, n = int(r["rows_off"]), int(r["n_eti"])
        return r, self.raw[o:o + n * ETI_FRAME_BYTES].reshape(n, ETI_FRAME_BYTES)

    def msc(self, s, j):
        """Logical frames of slot (s, j) in this chunk: [n_cifs, 3 * kbps] uint8 (a view)."""
        r = self.subch[s, j]
        nb = 3 * int(r["kbps"])
        o = int(r["msc_off"])
        return self.raw[o:o + int(r["n_cifs"]) * nb].reshape(int(r["n_cifs"]), nb)

    def superframes(self, s, j):
        """Super frames of slot (s, j) in this chunk: [n_sf, 110 * kbps / 8] uint8 (a view)."""
        r = self.subch[s, j]
        nb, pitch, o = 110 * int(r["kbps"]) // 8, int(r["sf_pitch"]), int(r["sf_off"])
        return self.raw[o:o + int(r["n_sf"]) * pitch].reshape(int(r["n_sf"]), pitch)[:, :nb]

    def superframe_info(self, s, j):
        """Their records (AU table, per-AU CRC verdicts, corrections): [n_sf] SUPERFRAME_INFO (a view)."""
        r = self.subch[s, j]
        o = int(r["sfi_off"])
        return self.raw[o:o + int(r["n_sf"]) * 32].view(SUPERFRAME_INFO)

    def _ring_items(self, table, rec_off, count, dtype, s, j):
        """(records, bytes) of slot (s, j) in a section of the slab whose table record names them rec_off / count / bytes_off / n_bytes."""
        if table is None or not int(table[s, j][rec_off]):
            return np.zeros(0, dtype), np.zeros(0, np.uint8)
        r = table[s, j]
        ro, bo = int(r[rec_off]), int(r["bytes_off"])
        return self.raw[ro:ro + int(r[count]) * 32].view(dtype), self.raw[bo:bo + int(r["n_bytes"])]

    def datagroups(self, s, j):
        """MSC data groups of packet-mode slot (s, j) in this chunk: ([n_dg] DATAGROUP_INFO, their n_bytes bytes), views; group i is
        bytes[byte_pos[i] : byte_pos[i] + length[i]].  Empty when the slab has no data-group section or the slot is not in packet mode."""
        return self._ring_items(self.dg, "rec_off", "n_dg", DATAGROUP_INFO, s, j)

    def pad_items(self, s, j):
        """PAD items of slot (s, j) in this chunk: ([n_items] PAD_ITEM, their n_bytes bytes), views; item i is
        bytes[byte_pos[i] : byte_pos[i] + length[i]].  Empty when the slab has no PAD section or the slot has no PAD decoding."""
        return self._ring_items(self.pad, "item_off", "n_items", PAD_ITEM, s, j)

    def mot_objects(self, s, j):
        """MOT objects of slot (s, j) in this chunk: ([n_objects] MOT_OBJECT, their n_bytes bytes), views; object i is
        bytes[byte_pos[i] : byte_pos[i] + body_len[i] + name_len[i]], body first.  Empty when the slab has no MOT section or the slot has no
        MOT decoding."""
        return self._ring_items(self.mot, "rec_off", "n_objects", MOT_OBJECT, s, j)

    def mp2_audio(self, s, j):
        """Decoded MP2 frames of slot (s, j) in this chunk: ([n_frames] MP2_AUDIO_FRAME, their n_bytes = 4608 n_frames bytes of PCM), views;
        frame i's samples are bytes[4608 i : 4608 (i + 1)].view(int16).reshape(1152, 2), left and right.  Empty when the slab has no MP2
        audio section or the slot has not the mode on."""
        return self._ring_items(self.mp2_audio_table, "rec_off", "n_frames", MP2_AUDIO_FRAME, s, j)

    def aac(self, s, j):
        """The LOAS stream of slot (s, j) in this chunk: (its CHUNK_AAC record or None, [n_frames] AAC_FRAME, their n_bytes bytes), views;
        record i's frame is bytes[byte_pos[i] : byte_pos[i] + length[i]] and the bytes are the slot's stream as it is.  None and empty when
        the slab has no AAC section or the slot has not the mode on."""
        rec, by = self._ring_items(self.aac_table, "rec_off", "n_frames", AAC_FRAME, s, j)
        return (self.aac_table[s, j] if self.aac_table is not None and int(self.aac_table[s, j]["rec_off"]) else None), rec, by

    def data(self, s, j):
        """The handler items of slot (s, j) in this chunk: (its CHUNK_DATA record or None, [n_items] DATA_ITEM, their n_bytes bytes), views;
        item i is bytes[byte_pos[i] : byte_pos[i] + length[i]].  None and empty when the slab has no data section or the slot has no
        handler on."""
        rec, by = self._ring_items(self.data_table, "rec_off", "n_items", DATA_ITEM, s, j)
        return (self.data_table[s, j] if self.data_table is not None and int(self.data_table[s, j]["rec_off"]) else None), rec, by

    def release(self):
        if self._eng is not None:
            check(load().dabx_delivery_release(self._eng._h, C.c_uint64(self.seq)))
            self._eng = None


COUNTER_NAMES = ["frames", "samples", "fib_ok", "fib_total", "sync_lost", "streams_locked", "cifs_decoded", "sf_ok", "sf_fail",
                 "rs_corrected", "rs_failed", "fc_corrected", "au_ok", "au_bad", "msc_bytes", "reserved"]
TF = 196608


class CreateExt(C.Structure):
    """dabx_create_ext (include/dabx.h)."""
    _fields_ = [("size", C.c_uint32), ("ring_format", C.c_int32), ("reserved", C.c_int32 * 6)]


RING_CF32, RING_S16, RING_U8 = 0, 1, 2
RING_FORMATS = {"cf32": RING_CF32, "s16": RING_S16, "u8": RING_U8}


class Engine:
    """Stream-batched receiver (device-side DabProcessor::run for n_streams ensembles).

    ring_format: the IQ ring's element -- 0 / "cf32" (default), 1 / "s16", 2 / "u8" (DABX_RING_*): a native ring keeps the recording's own
    codes, takes pushes of its own dtype only and decodes the very same bits."""

    def __init__(self, n_streams=1, ring_frames=4, max_subch=18, out_frames=4, fic_only=False, capture_soft=False,
                 sync_threshold=3.0, soft_bit_type=1, sync_strongest=False, viterbi_tie_mode=0, dc_iq_correction=0,
                 schedule=0, msc_fast_min_jobs=0, msc_class_min_jobs=0, exact_level_tracker=False, acquire_mode=0, ring_format=0):
        L = load()
        if isinstance(ring_format, str):
            ring_format = RING_FORMATS[ring_format.lower()]
        cfg = Config()
        L.dabx_default_config(C.byref(cfg))
        cfg.n_streams, cfg.ring_frames, cfg.max_subch, cfg.out_frames = n_streams, ring_frames, max_subch, out_frames
        cfg.fic_only, cfg.capture_soft, cfg.sync_threshold = int(fic_only), int(capture_soft), sync_threshold
        cfg.soft_bit_type, cfg.sync_strongest = soft_bit_type, int(sync_strongest)
        cfg.viterbi_tie_mode = int(viterbi_tie_mode)
        cfg.dc_iq_correction = int(dc_iq_correction)
        cfg.schedule, cfg.msc_fast_min_jobs, cfg.msc_class_min_jobs = int(schedule), int(msc_fast_min_jobs), int(msc_class_min_jobs)
        cfg.exact_level_tracker = int(exact_level_tracker)
        cfg.acquire_mode = int(acquire_mode)
        self.cfg = cfg
        self.n_streams = n_streams
        self._h = C.c_void_p()
        if int(ring_format) == RING_CF32:
            check(L.dabx_create(C.byref(cfg), C.byref(self._h)))
        else:
            ext = CreateExt(size=C.sizeof(CreateExt), ring_format=int(ring_format))
            check(L.dabx_create_ex(C.byref(cfg), C.byref(ext), C.byref(self._h)))
        self.subch = []

    def close(self):
        if getattr(self, "_h", None) and _LIB is not None:
            _LIB.dabx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_subchannels(self, subch, stream=-1, dab_plus=True):
        arr = (SubchDesc * max(1, len(subch)))()
        for i, c in enumerate(subch):
            dp = getattr(c, "dab_plus", -1)      # discovered descriptors carry FIG 0/2's answer; -1 = not yet known
            arr[i] = SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, int(dab_plus) if dp < 0 else dp, 0)
        check(load().dabx_set_subchannels(self._h, stream, arr, len(subch)))
        self.subch = list(subch)

    def push_iq(self, stream, iq):
        iq = np.ascontiguousarray(iq)
        fmt = {np.dtype(np.complex64): 0, np.dtype(np.int16): 1, np.dtype(np.uint8): 2}[iq.dtype]
        n = iq.size if fmt == 0 else iq.size // 2
        check(load().dabx_push_iq(self._h, stream, _p(iq), fmt, n))

    def push_iq_async(self, stream, iq):
        """iq must stay alive and unchanged until push_wait() (see dabx_push_iq_async); it is pushed in place, so it has to be
        C-contiguous (a strided view cannot be copied here: the copy would not outlive the call)."""
        if not iq.flags.c_contiguous:
            raise ValueError("push_iq_async needs a C-contiguous array")
        fmt = {np.dtype(np.complex64): 0, np.dtype(np.int16): 1, np.dtype(np.uint8): 2}[iq.dtype]
        n = iq.size if fmt == 0 else iq.size // 2
        check(load().dabx_push_iq_async(self._h, stream, _p(iq), fmt, n))

    def push_wait(self):
        check(load().dabx_push_wait(self._h))

    def read_iq(self, stream, first, n):
        out = np.zeros(n, np.complex64)
        check(load().dabx_read_iq(self._h, stream, C.c_uint64(first), C.c_size_t(n), _p(out)))
        return out

    def ring_format(self):
        """(DABX_RING_* of the engine's IQ ring, bytes per sample): (0, 8), (1, 4) or (2, 2)."""
        fmt, bps = C.c_int32(), C.c_int32()
        check(load().dabx_get_ring_format(self._h, C.byref(fmt), C.byref(bps)))
        return fmt.value, bps.value

    def ring_ptr(self, stream):
        p, cap = C.c_void_p(), C.c_size_t()
        check(load().dabx_iq_ring_dev(self._h, stream, C.byref(p), C.byref(cap)))
        return p.value, cap.value

    def commit(self, n_samples, stream=-1):
        check(load().dabx_commit_iq(self._h, stream, n_samples))

    def announce_write(self, n_samples, stream=-1):
        if hasattr(load(), "dabx_announce_write"):
            check(load().dabx_announce_write(self._h, stream, n_samples))

    def process(self, max_frames, sync=True):
        return check(load().dabx_process(self._h, max_frames, int(sync)))

    def synchronize(self):
        check(load().dabx_synchronize(self._h))

    def hip_stream(self):
        load().dabx_hip_stream.restype = C.c_void_p
        return load().dabx_hip_stream(self._h)

    def read_fibs(self, stream, n_frames=1):
        fibs = np.zeros((n_frames, 12, 32), np.uint8)
        crc = np.zeros((n_frames, 12), np.uint8)
        n = check(load().dabx_read_fibs(self._h, stream, n_frames, _p(fibs), _p(crc)))
        return fibs[:n], crc[:n]

    def read_frame_info(self, stream, n_frames=1):
        """(sym0_pos int64[n], start_index int32[n]) of the newest frames, oldest first (dabx_read_frame_info)."""
        pos = np.zeros(n_frames, np.int64)
        st = np.zeros(n_frames, np.int32)
        n = check(load().dabx_read_frame_info(self._h, stream, n_frames, _p(pos), _p(st)))
        return pos[:n], st[:n]

    def discover_subchannels(self, stream, max_out=64):
        out = (SubchDesc * max_out)()
        n = check(load().dabx_discover_subchannels(self._h, stream, out, max_out))
        return [out[i] for i in range(n)]

    def set_fig_reference_quirks(self, on):
        check(load().dabx_set_fig_reference_quirks(self._h, int(on)))

    def set_lcd_statistics(self, on):
        check(load().dabx_set_lcd_statistics(self._h, int(on)))

    def follow_fic(self, stream):
        out = Reconf()
        check(load().dabx_follow_fic(self._h, stream, C.byref(out)))
        return {k: getattr(out, k) for k, _ in Reconf._fields_ if not k.startswith("reserved")}

    def next_subchannels(self, stream, max_out=64):
        out = (SubchDesc * max_out)()
        n = check(load().dabx_next_subchannels(self._h, stream, out, max_out))
        return [out[i] for i in range(n)]

    def set_subchannels_at(self, subch, stream, at_cif, dab_plus=True):
        arr = (SubchDesc * max(1, len(subch)))()
        for i, c in enumerate(subch):
            dp = getattr(c, "dab_plus", -1)
            arr[i] = SubchDesc(c.subch_id, c.cu_start, c.cu_size, c.kbps, c.prot_level, c.short_form, int(dab_plus) if dp < 0 else dp, 0)
        load().dabx_set_subchannels_at.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64]
        check(load().dabx_set_subchannels_at(self._h, stream, arr, len(subch), at_cif))
        self.subch = list(subch)

    def subch_stats(self, stream, j):
        st = SubchStats()
        check(load().dabx_get_subch_stats(self._h, stream, j, C.byref(st)))
        return {k: getattr(st, k) for k, _ in SubchStats._fields_}

    def read_tii(self, stream, min_frames=1, threshold_db=6, collisions=False, collision_sub_id=0, max_out=64):
        out = (TiiResult * max_out)()
        acc = C.c_int32(0)
        n = check(load().dabx_read_tii(self._h, stream, min_frames, threshold_db, int(collisions), collision_sub_id, out, max_out,
                                       C.byref(acc)))
        return [out[i].as_tuple() for i in range(n)], acc.value

    def set_tii_mode(self, stream, min_frames=5, threshold_db=8, collisions=False, sub_id=0, enable=True):
        """The stream's TII detector on the device (dabx_set_tii_mode; stream = -1: all streams): an event whenever `min_frames` TII null
        symbols are in the sum, read with read_tii_events or delivered in bulk (DELIVER_TII)."""
        cfg = TiiConfig(enable=int(bool(enable)), min_frames=min_frames, threshold_db=threshold_db, collisions=int(bool(collisions)),
                        collision_sub_id=sub_id)
        L = load()
        L.dabx_set_tii_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_set_tii_mode(self._h, stream, C.byref(cfg)))

    def read_tii_events(self, stream, max_events=8):
        """The events completed since the previous call: ([(TII_EVENT record, results[:n_results] as TII_RESULT records)], events lost)."""
        ev = np.zeros(max_events, TII_EVENT)
        res = np.zeros((max_events, TII_MAX_RESULTS), TII_RESULT)
        lost = C.c_int32(0)
        L = load()
        L.dabx_read_tii_events.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        n = check(L.dabx_read_tii_events(self._h, stream, max_events, _p(ev), _p(res), C.byref(lost)))
        return [(ev[k], res[k, :int(ev[k]["n_results"])]) for k in range(n)], lost.value

    def tii_stats(self, stream):
        st = np.zeros(1, TII_STATS)
        L = load()
        L.dabx_get_tii_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_get_tii_stats(self._h, stream, _p(st)))
        return {k: int(st[k][0]) for k in TII_STATS.names if k != "reserved"}

    def set_fig_mode(self, stream, enable=True, reference_quirks=False, service_info=False):
        """The stream's FIC followed on the device (dabx_set_fig_mode; stream = -1: all streams): FIG 0/0-0/3 and the labels of FIG 1 go into
        a database on the device (fig_info, fig_subchannels, fig_packet_components, fig_labels, fig_follow), changes are reported as events
        (read_fig_events, or in bulk with DELIVER_FIG).  service_info: FIG 0/5 .. 0/19 are followed too (fig_si_info, fig_user_apps,
        fig_global_defs, fig_languages, fig_programme_types, fig_fec_schemes, fig_clusters, fig_si_stats, fig_directory; events of kinds 6-9)."""
        cfg = FigConfig(enable=int(bool(enable)), reference_quirks=int(bool(reference_quirks)), service_info=int(bool(service_info)))
        L = load()
        L.dabx_set_fig_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_set_fig_mode(self._h, stream, C.byref(cfg)))

    def fig_info(self, stream):
        out = FibdecInfo()
        L = load()
        L.dabx_fig_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_fig_info(self._h, stream, C.byref(out)))
        return {k: getattr(out, k) for k, _ in FibdecInfo._fields_ if not k.startswith("reserved")}

    def fig_subchannels(self, stream, next=False, max_out=64):
        out = (SubchDesc * max_out)()
        L = load()
        L.dabx_fig_subchannels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        n = check(L.dabx_fig_subchannels(self._h, stream, int(next), out, max_out))
        return [out[i] for i in range(n)]

    def fig_packet_components(self, stream, next=False, max_out=FIG_MAX_PACKETS):
        out = np.zeros(max(1, max_out), PACKET_COMPONENT)
        L = load()
        L.dabx_fig_packet_components.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        n = check(L.dabx_fig_packet_components(self._h, stream, int(next), _p(out), max_out))
        return out[:n]

    def fig_follow(self, stream):
        out = Reconf()
        L = load()
        L.dabx_fig_follow.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_fig_follow(self._h, stream, C.byref(out)))
        return {k: getattr(out, k) for k, _ in Reconf._fields_ if not k.startswith("reserved")}

    def fig_labels(self, stream, max_out=4 * FIG_MAX_LABELS):
        """Every label filed so far, in order of filing: a list of dicts (fig_label_dict)."""
        out = np.zeros(max(1, max_out), FIG_LABEL)
        L = load()
        L.dabx_fig_labels.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        n = check(L.dabx_fig_labels(self._h, stream, _p(out), max_out))
        return [fig_label_dict(r) for r in out[:n]]

    def fig_stats(self, stream):
        st = np.zeros(1, FIG_STATS)
        L = load()
        L.dabx_get_fig_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_get_fig_stats(self._h, stream, _p(st)))
        return {k: int(st[k][0]) for k in FIG_COUNTERS}

    def fig_si_info(self, stream):
        """FIG 0/7 of both configurations, FIG 0/9, the newest FIG 0/10 and the SI tables' sizes (dabx_fig_si_info) as a dict."""
        out = np.zeros(1, FIG_SI_INFO)
        L = load()
        L.dabx_fig_si_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_fig_si_info(self._h, stream, _p(out)))
        return _rec_dict(out[0])

    def _fig_si_table(self, name, dtype, cap, stream, next=None):
        out = np.zeros(cap, dtype)
        fn = getattr(load(), name)
        if next is None:
            fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            n = check(fn(self._h, stream, _p(out), cap))
        else:
            fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
            n = check(fn(self._h, stream, int(next), _p(out), cap))
        return out[:n]

    def fig_user_apps(self, stream, next=False):
        """FIG 0/13 of the current (or next) configuration in order of filing: a list of dicts (fig_user_apps_dict)."""
        return [fig_user_apps_dict(r) for r in self._fig_si_table("dabx_fig_user_apps", FIG_USER_APPS, FIG_MAX_USER_APPS, stream, next)]

    def fig_global_defs(self, stream, next=False):
        return [_rec_dict(r) for r in self._fig_si_table("dabx_fig_global_defs", FIG_GLOBAL_DEF, FIG_MAX_GLOBAL_DEFS, stream, next)]

    def fig_fec_schemes(self, stream, next=False):
        """FIG 0/14: [(SubChId, FEC scheme)]."""
        return [(int(r["subch_id"]), int(r["scheme"])) for r in self._fig_si_table("dabx_fig_fec_schemes", FIG_FEC, 64, stream, next)]

    def fig_clusters(self, stream, next=False):
        return [fig_cluster_dict(r) for r in self._fig_si_table("dabx_fig_clusters", FIG_CLUSTER, FIG_MAX_CLUSTERS, stream, next)]

    def fig_languages(self, stream):
        """FIG 0/5: [(L/S, SubChId or SCId, language)]."""
        return [(int(r["ls"]), int(r["id"]), int(r["language"])) for r in self._fig_si_table("dabx_fig_languages", FIG_LANGUAGE, FIG_MAX_LANGUAGES, stream)]

    def fig_programme_types(self, stream):
        """FIG 0/17: [(SId, S/D, international code)]."""
        return [(int(r["sid"]), int(r["sd"]), int(r["code"])) for r in self._fig_si_table("dabx_fig_programme_types", FIG_PTY, FIG_MAX_PTYS, stream)]

    def fig_si_stats(self, stream):
        st = np.zeros(1, FIG_SI_STATS)
        L = load()
        L.dabx_get_fig_si_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_get_fig_si_stats(self._h, stream, _p(st)))
        return {k: int(st[k][0]) for k in FIG_SI_COUNTERS}

    def fig_directory(self, stream=-1, next=False, max_per_stream=FIG_MAX_COMPONENTS):
        """The service directory (dabx_fig_directory: one launch, one copy): every service component of the current (or next) configuration
        joined with its sub-channel, packet data, language, programme type, user applications and label -- a list of dicts (fig_service_dict)
        for one stream, a list of such lists for stream = -1.  Charset conversion and the short label stay with the caller."""
        n = self.n_streams if stream < 0 else 1
        out, cnt = np.zeros((n, max(1, max_per_stream)), FIG_SERVICE), np.zeros(n, np.int32)
        L = load()
        L.dabx_fig_directory.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_fig_directory(self._h, stream, int(next), _p(out), max_per_stream, _p(cnt)))
        rows = [[fig_service_dict(r) for r in out[s, :min(int(cnt[s]), max_per_stream)]] for s in range(n)]
        return rows if stream < 0 else rows[0]

    def read_fig_events(self, stream, max_events=FIG_MAX_EVENTS):
        """The events written since the previous call that the ring still holds, oldest first: ([fig_event_dict], events lost)."""
        ev = np.zeros(max(1, max_events), FIG_EVENT)
        lost = C.c_int32(0)
        L = load()
        L.dabx_read_fig_events.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        n = check(L.dabx_read_fig_events(self._h, stream, max_events, _p(ev), C.byref(lost)))
        return [fig_event_dict(e) for e in ev[:n]], lost.value

    def set_scope_mode(self, stream, iq_type=0, carrier_type=0, symbol=0, enable=True):
        """The stream's IQ scope and carrier plot on the device (dabx_set_scope_mode; stream = -1: all streams): a record whenever the
        reference would show a symbol (symbol = 0), or for OFDM symbol `symbol` (1..75) of every decoded frame; read with read_scope."""
        cfg = ScopeConfig(enable=int(bool(enable)), iq_type=iq_type, carrier_type=carrier_type, symbol=symbol)
        L = load()
        L.dabx_set_scope_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_set_scope_mode(self._h, stream, C.byref(cfg)))

    def read_scope(self, stream, max_records=8):
        """The records completed since the previous call: ([(SCOPE_RECORD record, iq [1536] complex64, carr [1536] float32)], records lost)."""
        recs = np.zeros(max_records, SCOPE_RECORD)
        iq = np.zeros((max_records, SCOPE_CARRIERS), np.complex64)
        carr = np.zeros((max_records, SCOPE_CARRIERS), np.float32)
        lost = C.c_int32(0)
        L = load()
        L.dabx_read_scope.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        n = check(L.dabx_read_scope(self._h, stream, max_records, _p(recs), _p(iq), _p(carr), C.byref(lost)))
        return [(recs[k], iq[k], carr[k]) for k in range(n)], lost.value

    def set_cir_mode(self, stream, cir=True, correlation=False, enable=True):
        """The stream's channel impulse response plot and / or correlation plot on the device (dabx_set_cir_mode; stream = -1: all streams):
        a CIR record per window of 97 x 2048 samples every six frames' worth of samples, a correlation record whenever the reference would
        show its plot; read with read_cir.  enable=False switches both off."""
        cfg = CirConfig(enable=int(bool(enable)), cir=int(bool(cir)), correlation=int(bool(correlation)))
        L = load()
        L.dabx_set_cir_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_set_cir_mode(self._h, stream, C.byref(cfg) if enable else None))

    def read_cir(self, stream, max_records=4):
        """The records completed since the previous call: ([(CIR_RECORD record, values[:n_values] float32, indices[:n_indices] int16)], records lost)."""
        recs = np.zeros(max_records, CIR_RECORD)
        val = np.zeros((max_records, CIR_CORR_LAGS), np.float32)
        idx = np.zeros((max_records, CIR_INDEX_ROOM), np.int16)
        lost = C.c_int32(0)
        L = load()
        L.dabx_read_cir.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        n = check(L.dabx_read_cir(self._h, stream, max_records, _p(recs), _p(val), _p(idx), C.byref(lost)))
        return [(recs[k], val[k, :int(recs[k]["n_values"])], idx[k, :int(recs[k]["n_indices"])]) for k in range(n)], lost.value

    def cir_stats(self, stream):
        st = np.zeros(1, CIR_STATS)
        L = load()
        L.dabx_get_cir_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_get_cir_stats(self._h, stream, _p(st)))
        return {"shows": [int(v) for v in st["shows"][0]], "lost": int(st["lost"][0]), "rows_untrusted": int(st["rows_untrusted"][0]),
                "launches": int(st["launches"][0])}

    def set_spectrum_mode(self, stream, averaging="medium", zoom=0, enable=True):
        """The stream's RF spectrum and waterfall rows on the device (dabx_set_spectrum_mode; stream = -1: all streams): a record per show of
        SpectrumViewer::show_spectrum, more than 512 000 consumed samples apart; read with read_spectrum.  averaging: "slow" / "medium" /
        "fast" (the filter of the display limits), zoom: 0..100 (the waterfall's scaling).  enable=False switches it off."""
        cfg = SpectrumConfig(enable=int(bool(enable)), averaging=SPECTRUM_AVERAGING.get(averaging, averaging), zoom_percent=int(zoom))
        L = load()
        L.dabx_set_spectrum_mode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_set_spectrum_mode(self._h, stream, C.byref(cfg) if enable else None))

    def read_spectrum(self, stream, max_records=8):
        """The records completed since the previous call: ([(SPECTRUM_RECORD record, SPECTRUM_LIMITS record, db [512] float32, row [512] uint8)],
        records lost)."""
        recs = np.zeros(max_records, SPECTRUM_RECORD)
        lim = np.zeros(max_records, SPECTRUM_LIMITS)
        db = np.zeros((max_records, SPECTRUM_BINS), np.float32)
        row = np.zeros((max_records, SPECTRUM_BINS), np.uint8)
        lost = C.c_int32(0)
        L = load()
        L.dabx_read_spectrum.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        n = check(L.dabx_read_spectrum(self._h, stream, max_records, _p(recs), _p(lim), _p(db), _p(row), C.byref(lost)))
        return [(recs[k], lim[k], db[k], row[k]) for k in range(n)], lost.value

    def spectrum_stats(self, stream):
        st = np.zeros(1, SPECTRUM_STATS)
        L = load()
        L.dabx_get_spectrum_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_get_spectrum_stats(self._h, stream, _p(st)))
        return {k: int(st[k][0]) for k in ("shows", "untrusted", "lost", "launches", "inexact")}

    def scope_stats(self, stream):
        st = np.zeros(1, SCOPE_STATS)
        L = load()
        L.dabx_get_scope_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        check(L.dabx_get_scope_stats(self._h, stream, _p(st)))
        return {k: int(st[k][0]) for k in SCOPE_STATS.names if k != "reserved"}

    def read_eti(self, stream, max_frames=32):
        out = np.zeros((max_frames, 6144), np.uint8)
        lost = C.c_int32(0)
        n = check(load().dabx_read_eti(self._h, stream, max_frames, _p(out), C.byref(lost)))
        return out[:n], lost.value

    def read_msc(self, stream, j, n_cifs=4):
        nb = 3 * self.subch[j].kbps
        out = np.zeros((n_cifs, nb), np.uint8)
        n = check(load().dabx_read_msc(self._h, stream, j, n_cifs, _p(out)))
        return out[:n]

    def read_superframes(self, stream, j, n=1):
        nb = 110 * self.subch[j].kbps // 8
        out = np.zeros((n, nb), np.uint8)
        k = check(load().dabx_read_superframes(self._h, stream, j, n, _p(out)))
        return out[:k]

    def read_superframe_info(self, stream, j, n=1):
        """Records of the newest n super frames of slot j, oldest first (row i belongs to row i of read_superframes(stream, j, n))."""
        out = np.zeros(n, SUPERFRAME_INFO)
        k = check(load().dabx_read_superframe_info(self._h, stream, j, n, _p(out)))
        return out[:k]

    def set_packet_mode(self, stream, j, packet_address):
        """Slot j of `stream` becomes a packet-mode data sub-channel with this packet address (dabx_set_packet_mode); None switches it
        back to plain logical frames."""
        L = load()
        if packet_address is None:
            check(L.dabx_set_packet_mode(self._h, int(stream), int(j), None))
        else:
            cfg = PacketConfig(size=C.sizeof(PacketConfig), packet_address=int(packet_address))
            check(L.dabx_set_packet_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def _read_ring(self, call, dtype, ring_bytes, stream, j, n, max_bytes, with_bytes):
        """dabx_read_datagroups / dabx_read_pad_items: (records [k], bytes); with_bytes = False passes bytes = NULL (records only, no bytes)."""
        info = np.zeros(max(1, n), dtype)
        if not with_bytes:
            return info[:check(call(self._h, int(stream), int(j), int(n), _p(info), None, 0))], np.zeros(0, np.uint8)
        if max_bytes is None:
            max_bytes = ring_bytes                        # no slot's byte ring holds more
        buf = np.zeros(max(1, int(max_bytes)), np.uint8)
        k = check(call(self._h, int(stream), int(j), int(n), _p(info), _p(buf), int(max_bytes)))
        info = info[:k]
        return info, buf[:int(info["length"].sum())].copy()

    def read_datagroups(self, stream, j, n=64, max_bytes=None, with_bytes=True):
        """(records [k] DATAGROUP_INFO, bytes uint8) of the newest k <= n completed data groups of slot j, oldest first; group i is
        bytes[byte_pos[i] : byte_pos[i] + length[i]].  with_bytes = False: the records alone."""
        return self._read_ring(load().dabx_read_datagroups, DATAGROUP_INFO, DG_RING_MAX_BYTES, stream, j, n, max_bytes, with_bytes)

    def packet_stats(self, stream, j):
        """dabx_packet_stats of slot j as a dict."""
        L = load()
        out = np.zeros(1, PACKET_STATS)
        check(L.dabx_get_packet_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in PACKET_STATS.names if k != "reserved"}

    def set_pad_mode(self, stream, j, on=True, source="dabplus"):
        """Switches the PAD decoding of slot j of `stream` on (restarting it when it is on already) or off (dabx_set_pad_mode).  source:
        "dabplus", the access units of a DAB+ slot, or "mp2", the MP2 frames of a DAB audio slot (an integer is passed on as it is)."""
        L = load()
        if not on:
            check(L.dabx_set_pad_mode(self._h, int(stream), int(j), None))
        else:
            cfg = PadConfig(size=C.sizeof(PadConfig), source=PAD_SOURCES[source] if isinstance(source, str) else int(source))
            check(L.dabx_set_pad_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def read_pad_items(self, stream, j, n=512, max_bytes=None, with_bytes=True):
        """(records [k] PAD_ITEM, bytes uint8) of the newest k <= n PAD items of slot j, oldest first, dynamic labels and X-PAD MSC data
        groups in emission order; item i is bytes[byte_pos[i] : byte_pos[i] + length[i]].  with_bytes = False: the records alone."""
        return self._read_ring(load().dabx_read_pad_items, PAD_ITEM, PAD_RING_BYTES, stream, j, n, max_bytes, with_bytes)

    def pad_stats(self, stream, j):
        """dabx_pad_stats of slot j as a dict."""
        L = load()
        out = np.zeros(1, PAD_STATS)
        check(L.dabx_get_pad_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in PAD_STATS.names if k != "reserved"}

    def set_mot_mode(self, stream, j, on=True, max_object_bytes=0):
        """Switches the MOT decoding of PAD slot j of `stream` on (restarting it when it is on already) or off (dabx_set_mot_mode).
        max_object_bytes: the bound of an object's stored segments, 0 = 65 536."""
        L = load()
        if not on:
            check(L.dabx_set_mot_mode(self._h, int(stream), int(j), None))
        else:
            cfg = MotConfig(size=C.sizeof(MotConfig), max_object_bytes=int(max_object_bytes))
            check(L.dabx_set_mot_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def read_mot_objects(self, stream, j, n=256, max_bytes=None, with_bytes=True):
        """(records [k] MOT_OBJECT, bytes uint8) of the newest k <= n MOT objects of slot j that are still in its rings, oldest first;
        object i is bytes[byte_pos[i] : byte_pos[i] + body_len[i] + name_len[i]], the body and then the name.  with_bytes = False: the
        records alone.  max_bytes None: as much as `n` objects of the default size can have."""
        call = load().dabx_read_mot_objects
        info = np.zeros(max(1, n), MOT_OBJECT)
        if not with_bytes:
            return info[:check(call(self._h, int(stream), int(j), int(n), _p(info), None, 0))], np.zeros(0, np.uint8)
        if max_bytes is None:
            max_bytes = 2 * (MOT_OBJECT_BYTES_DEFAULT + MOT_NAME_ROOM)
        buf = np.zeros(max(1, int(max_bytes)), np.uint8)
        k = check(call(self._h, int(stream), int(j), int(n), _p(info), _p(buf), int(max_bytes)))
        info = info[:k]
        return info, buf[:int(info["body_len"].sum()) + int(info["name_len"].sum())].copy()

    def mot_stats(self, stream, j):
        """dabx_mot_stats of slot j as a dict (all zero unless MOT decoding is on for the slot)."""
        out = np.zeros(1, MOT_STATS)
        check(load().dabx_get_mot_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in MOT_STATS.names if k != "reserved"}

    def set_carousel_mode(self, stream, j, on=True, max_object_bytes=0, max_dir_objects=0, max_dir_bytes=0):
        """Switches the carousel decoding (MotHandler / MotDirectory) of packet-mode slot j of `stream` on (restarting it when it is on
        already) or off (dabx_set_carousel_mode).  max_object_bytes: the bound of an object's stored segments, 0 = 65 536;
        max_dir_objects: the most objects a directory may announce, 0 = 49; max_dir_bytes: the largest directory, 0 = 65 536.  The objects
        are read with read_mot_objects."""
        L = load()
        if not on:
            check(L.dabx_set_carousel_mode(self._h, int(stream), int(j), None))
        else:
            cfg = CarouselConfig(size=C.sizeof(CarouselConfig), max_object_bytes=int(max_object_bytes), max_dir_objects=int(max_dir_objects),
                                 max_dir_bytes=int(max_dir_bytes))
            check(L.dabx_set_carousel_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def carousel_stats(self, stream, j):
        """dabx_carousel_stats of slot j as a dict (all zero unless carousel decoding is on for the slot)."""
        out = np.zeros(1, CAROUSEL_STATS)
        check(load().dabx_get_carousel_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in CAROUSEL_STATS.names}

    def set_data_mode(self, stream, j, handler="tdc", only_new_revisions=False, on=True):
        """Switches a data handler of packet-mode slot j of `stream` on (restarting it when one is on already) or off (dabx_set_data_mode).
        handler: "tdc", "ip" or "journaline" (an integer is passed on as it is); only_new_revisions: Journaline objects whose revision
        is the one filed are not emitted.  The items are read with read_data_items."""
        L = load()
        if not on:
            check(L.dabx_set_data_mode(self._h, int(stream), int(j), None))
        else:
            cfg = DataConfig(size=C.sizeof(DataConfig), handler=DATA_HANDLERS[handler] if isinstance(handler, str) else int(handler),
                             only_new_revisions=int(bool(only_new_revisions)))
            check(L.dabx_set_data_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def read_data_items(self, stream, j, n=256, max_bytes=None, with_bytes=True):
        """(records [k] DATA_ITEM, bytes uint8) of the newest k <= n items of slot j that are still in its rings, oldest first; item i is
        bytes[byte_pos[i] : byte_pos[i] + length[i]].  with_bytes = False: the records alone."""
        return self._read_ring(load().dabx_read_data_items, DATA_ITEM, DG_RING_MAX_BYTES, stream, j, n, max_bytes, with_bytes)

    def data_stats(self, stream, j):
        """dabx_data_stats of slot j as a dict (all zero but `launches` unless a handler is on for the slot)."""
        out = np.zeros(1, DATA_STATS)
        check(load().dabx_get_data_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in DATA_STATS.names}

    def set_mp2_audio_mode(self, stream, j, on=True):
        """Switches the MP2 audio decoding of DAB audio slot j of `stream` on (restarting it, as a fresh Mp2Processor, when it is on already)
        or off (dabx_set_mp2_audio_mode).  Independent of the slot's PAD mode."""
        L = load()
        if not on:
            check(L.dabx_set_mp2_audio_mode(self._h, int(stream), int(j), None))
        else:
            cfg = Mp2AudioConfig(size=C.sizeof(Mp2AudioConfig))
            check(L.dabx_set_mp2_audio_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def read_mp2_audio(self, stream, j, n=64, max_bytes=None, with_bytes=True):
        """(records [k] MP2_AUDIO_FRAME, bytes uint8 [k * 4608]) of the newest k <= n decoded MP2 frames of slot j, oldest first; frame i's
        PCM is bytes[4608 i : 4608 (i + 1)].view(int16).reshape(1152, 2), left and right.  with_bytes = False: the records alone."""
        call = load().dabx_read_mp2_audio
        info = np.zeros(max(1, n), MP2_AUDIO_FRAME)
        if not with_bytes:
            return info[:check(call(self._h, int(stream), int(j), int(n), _p(info), None, 0))], np.zeros(0, np.uint8)
        if max_bytes is None:
            max_bytes = min(MP2_AUDIO_RING_BYTES, n * MP2_PCM_BYTES)
        buf = np.zeros(max(1, int(max_bytes)), np.uint8)
        k = check(call(self._h, int(stream), int(j), int(n), _p(info), _p(buf), int(max_bytes)))
        return info[:k], buf[:k * MP2_PCM_BYTES].copy()

    def mp2_audio_stats(self, stream, j):
        """dabx_mp2_audio_stats of slot j as a dict (all zero but `launches` unless the mode is on); pcm_bytes = 4608 * frames_out."""
        out = np.zeros(1, MP2_AUDIO_STATS)
        check(load().dabx_get_mp2_audio_stats(self._h, int(stream), int(j), _p(out)))
        st = {k: int(out[0][k]) for k in MP2_AUDIO_STATS.names}
        st["pcm_bytes"] = MP2_PCM_BYTES * st["frames_out"]
        return st

    def set_aac_stream_mode(self, stream, j, on=True):
        """Switches the LOAS framing of DAB+ slot j of `stream` on (restarting it with empty rings when it is on already) or off
        (dabx_set_aac_stream_mode).  Independent of the slot's PAD and MOT modes."""
        L = load()
        if not on:
            check(L.dabx_set_aac_stream_mode(self._h, int(stream), int(j), None))
        else:
            cfg = AacStreamConfig(size=C.sizeof(AacStreamConfig), format=0)
            check(L.dabx_set_aac_stream_mode(self._h, int(stream), int(j), C.byref(cfg)))

    def read_aac_frames(self, stream, j, n=128, max_bytes=None):
        """(records [k] AAC_FRAME, bytes uint8) of the newest k <= n access units of slot j, oldest first; record i's LOAS frame is
        bytes[byte_pos[i] : byte_pos[i] + length[i]] (length 0: a lost access unit), and `bytes` is that stretch of the slot's stream."""
        info = np.zeros(max(1, n), AAC_FRAME)
        if max_bytes is None:
            max_bytes = n * AAC_MAX_FRAME_BYTES
        buf = np.zeros(max(1, int(max_bytes)), np.uint8)
        k = check(load().dabx_read_aac_frames(self._h, int(stream), int(j), int(n), _p(info), _p(buf), int(max_bytes)))
        info = info[:k]
        total = int(info["byte_pos"][-1]) + int(info["length"][-1]) if k else 0
        return info, buf[:total].copy()

    def aac_stream_stats(self, stream, j):
        """dabx_aac_stream_stats of slot j as a dict (all zero but `launches` unless the mode is on)."""
        out = np.zeros(1, AAC_STREAM_STATS)
        check(load().dabx_get_aac_stream_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in AAC_STREAM_STATS.names}

    def mp2_sync_stats(self, stream, j):
        """dabx_mp2_sync_stats of slot j as a dict (all zero unless the slot is a PAD slot with source "mp2")."""
        out = np.zeros(1, MP2_SYNC_STATS)
        check(load().dabx_get_mp2_sync_stats(self._h, int(stream), int(j), _p(out)))
        return {k: int(out[0][k]) for k in MP2_SYNC_STATS.names if k != "reserved"}

    def read_soft(self, stream):
        out = np.zeros((75, 3072), np.int16)
        check(load().dabx_read_soft(self._h, stream, _p(out)))
        return out

    def ingest_open(self, fmt, slabs=2, max_frames=0, copy_engine=0):
        """fmt: numpy dtype (complex64 / int16 / uint8) or 0..2.  Returns the page-locked slabs as numpy arrays [n_streams * max_frames * TF (* 2)]."""
        code = fmt if isinstance(fmt, int) else {np.dtype(np.complex64): 0, np.dtype(np.int16): 1, np.dtype(np.uint8): 2}[np.dtype(fmt)]
        cfg = IngestConfig(host_slabs=slabs, fmt=code, max_frames=max_frames, copy_engine=copy_engine)
        L = load()
        L.dabx_ingest_submit.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        check(L.dabx_ingest_open(self._h, C.byref(cfg)))
        out = []
        for k in range(slabs):
            p, cap = C.c_void_p(), C.c_size_t()
            check(L.dabx_ingest_slab(self._h, k, C.byref(p), C.byref(cap)))
            dt = (np.complex64, np.int16, np.uint8)[code]
            out.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cap.value,)).view(dt))
        return out

    def ingest_open_formats(self, formats, slabs=2, max_frames=0, copy_engine=0):
        """The general form: formats[s] = IqFormat of stream s.  Returns (slabs as uint8 arrays [n_streams, pitch], pitch)."""
        assert len(formats) == self.n_streams
        cfg = IngestConfig(host_slabs=slabs, fmt=0, max_frames=max_frames, copy_engine=copy_engine)
        arr = (IqFormat * len(formats))(*formats)
        L = load()
        L.dabx_ingest_pitch.restype = C.c_longlong
        check(L.dabx_ingest_open_formats(self._h, C.byref(cfg), arr))
        pitch = check(L.dabx_ingest_pitch(self._h))
        out = []
        for k in range(slabs):
            p, cap = C.c_void_p(), C.c_size_t()
            check(L.dabx_ingest_slab(self._h, k, C.byref(p), C.byref(cap)))
            assert cap.value == pitch * self.n_streams
            out.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(cap.value,)).reshape(self.n_streams, pitch))
        return out, pitch

    def ingest_submit_bytes(self, k, n_bytes):
        arr = (C.c_size_t * self.n_streams)(*[int(v) for v in n_bytes])
        check(load().dabx_ingest_submit_bytes(self._h, k, arr))

    def ingest_submit(self, k, n_samples):
        check(load().dabx_ingest_submit(self._h, k, n_samples))

    def ingest_commit(self, k):
        check(load().dabx_ingest_commit(self._h, k))

    def ingest_close(self):
        check(load().dabx_ingest_close(self._h))

    def delivery_open(self, slots=4, what=0, copy_engine=0):
        cfg = DeliveryConfig(host_slabs=slots, what=what, copy_engine=copy_engine)
        check(load().dabx_delivery_open(self._h, C.byref(cfg)))

    def delivery_close(self):
        check(load().dabx_delivery_close(self._h))

    def delivery_slab_bytes(self):
        load().dabx_delivery_slab_bytes.restype = C.c_longlong
        return check(load().dabx_delivery_slab_bytes(self._h))

    def delivery_info(self):
        out = DeliveryInfo()
        load().dabx_delivery_get_info.argtypes = [C.c_void_p, C.c_void_p]
        check(load().dabx_delivery_get_info(self._h, C.byref(out)))
        return {k: getattr(out, k) for k, _ in DeliveryInfo._fields_ if not k.startswith("reserved")}

    def delivery_wait_free(self, n=1, timeout_ms=-1):
        return check(load().dabx_delivery_wait_free(self._h, int(n), int(timeout_ms)))

    def delivery_next(self, wait=False):
        """The oldest chunk not yet fetched as a Chunk (views into the page-locked host slab), or None."""
        ref = ChunkRef()
        if check(load().dabx_delivery_next(self._h, int(wait), C.byref(ref))) == 0:
            return None
        return Chunk(self, ref)

    def stats(self, stream):
        st = Stats()
        check(load().dabx_get_stats_sized(self._h, stream, C.byref(st), C.c_size_t(C.sizeof(st))))
        return {k: getattr(st, k) for k, _ in Stats._fields_ if not k.startswith("reserved")}

    def counters(self):
        out = (C.c_int64 * 16)()
        check(load().dabx_get_counters(self._h, out))
        return dict(zip(COUNTER_NAMES, list(out)))


def eti_frame(cif_hi, cif_lo, minor, subch, fic96, msc):
    """Host only: one 6144-byte ETI(NI) frame; subch = SubchDesc list (FIC order), msc = list of byte arrays."""
    arr = (SubchDesc * max(1, len(subch)))(*subch)
    bufs = [np.ascontiguousarray(m, np.uint8) for m in msc]
    ptrs = (C.c_void_p * max(1, len(bufs)))(*[b.ctypes.data for b in bufs])
    fic96 = np.ascontiguousarray(fic96, np.uint8)
    out = np.zeros(6144, np.uint8)
    used = check(load().dabx_eti_frame(cif_hi, cif_lo, minor, arr, len(subch), _p(fic96), ptrs, _p(out)))
    return out, used


def eti_frames_device(cif_hi, cif_lo, minor, subch, fic96, msc):
    """The same assembly on the device, n frames of one layout (a wavefront each, the kernel body of the delivery's ETI stage): cif_hi /
    cif_lo / minor [n], subch = SubchDesc list, fic96 [n, 96], msc [n, sum of 3 * kbps] -> ([n, 6144] uint8, used [n] int32)."""
    hi = np.ascontiguousarray(cif_hi, np.int32).reshape(-1)
    lo = np.ascontiguousarray(cif_lo, np.int32).reshape(-1)
    mi = np.ascontiguousarray(minor, np.int32).reshape(-1)
    n = hi.size
    if lo.size != n or mi.size != n:
        raise ValueError("eti_frames_device needs one (cif_hi, cif_lo, minor) per frame")
    arr = (SubchDesc * max(1, len(subch)))(*subch)
    fic96 = np.ascontiguousarray(fic96, np.uint8).reshape(n, 96)
    msc = np.ascontiguousarray(msc, np.uint8).reshape(n, -1)
    out = np.zeros((n, ETI_FRAME_BYTES), np.uint8)
    used = np.zeros(n, np.int32)
    L = load()
    L.dabx_eti_frames_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.dabx_eti_frames_device(n, _p(hi), _p(lo), _p(mi), arr, len(subch), _p(fic96), _p(msc) if msc.size else None, _p(out), _p(used)))
    return out, used


def tii_process_device(sums, pairs, cfgs, out=None, n_results=None, n_found=None):
    """The TII detector on the device, n independent detectors in one call (a block each, the device function of the engine's k_tii): sums
    [n, 2048] complex64, pairs [n, 768] complex64 (the detectors' state: a copy is advanced and returned), cfgs = n dicts / TiiConfig
    (threshold_db, collisions, collision_sub_id, enable) -> (pairs, results [n, 32] TII_RESULT, n_results [n], n_found [n]).  out /
    n_results / n_found: what a detector with enable = 0 leaves in its rows."""
    sums = np.ascontiguousarray(sums, np.complex64).reshape(-1, 2048)
    n = sums.shape[0]
    pairs = np.array(pairs, np.complex64).reshape(n, 768)
    arr = (TiiConfig * max(1, n))(*[c if isinstance(c, TiiConfig) else TiiConfig(**dict({"enable": 1}, **c)) for c in cfgs])
    if len(cfgs) != n:
        raise ValueError("tii_process_device needs one configuration per detector")
    res = np.zeros((n, TII_MAX_RESULTS), TII_RESULT)
    if out is not None:
        res[...] = np.asarray(out, TII_RESULT).reshape(n, TII_MAX_RESULTS)
    nr = np.zeros(n, np.int32) if n_results is None else np.array(n_results, np.int32).reshape(n)
    nf = np.zeros(n, np.int32) if n_found is None else np.array(n_found, np.int32).reshape(n)
    L = load()
    L.dabx_tii_process_device.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    check(L.dabx_tii_process_device(n, _p(sums), _p(pairs), arr, _p(res), _p(nr), _p(nf)))
    return pairs, res, nr, nf


def host_register(a):
    """Page-locks a numpy array's memory (hipHostRegister) so that pushes from it are DMA; returns the array."""
    check(load().dabx_host_register(_p(a), a.nbytes))
    return a


def host_unregister(a):
    check(load().dabx_host_unregister(_p(a)))


def probe_iq_file(path):
    """Host only: container / sample format of a recorded-IQ file (.raw/.iq, .sdr/.wav, .uff)."""
    fmt = IqFormat()
    check(load().dabx_probe_iq_file(os.fsencode(path), C.byref(fmt)))
    return fmt


def convert_iq_bytes(fmt, payload):
    """One-shot GPU decode (+ resample) of payload bytes -> complex64 at 2.048 MS/s."""
    payload = np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8)
    n_in = payload.size // fmt.sample_bytes()
    cap = n_in if fmt.sample_rate == 2048000 else (n_in // (fmt.sample_rate // 1000) + 1) * 2048
    out = np.zeros(max(cap, 1), np.complex64)
    n = check(load().dabx_convert_iq_bytes(C.byref(fmt), _p(payload), payload.size, _p(out), out.size))
    return out[:n]


class Feed:
    """Streaming file feed into one stream's IQ ring (dabx_feed_*)."""

    def __init__(self, engine, stream, fmt):
        self._h = C.c_void_p()
        self.fmt = fmt
        check(load().dabx_feed_open(engine._h, stream, C.byref(fmt), C.byref(self._h)))

    def push(self, payload):
        payload = np.frombuffer(payload, np.uint8) if not isinstance(payload, np.ndarray) else np.ascontiguousarray(payload, np.uint8)
        return check(load().dabx_feed_bytes(self._h, _p(payload), payload.size))

    def bound(self, n_bytes):
        return check(load().dabx_feed_bound(self._h, n_bytes))

    def close(self):
        if self._h and _LIB is not None:
            _LIB.dabx_feed_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def play_file(engine, stream, path, block_frames=4, on_block=None):
    """Un-paced replay of a recorded file through one stream: probe, feed in blocks, process as frames become
    available.  Like the reference's readers (raw_reader.cpp:140-150, wav_reader.cpp:164-177) the final partial
    32768-unit read block is dropped.  Returns the number of frames processed."""
    fmt = probe_iq_file(path)
    unit = 32768 if fmt.family == 0 else 32768 * fmt.sample_bytes()      # raw: bytes, wav: frames
    if fmt.family == 2:
        unit = (fmt.sample_rate // 1000) * fmt.sample_bytes()            # uff: 1-ms reads, xml_reader.cpp:224-226
    n_units = fmt.data_bytes // unit
    feed = Feed(engine, stream, fmt)
    frames = 0
    per_block = max(1, (block_frames * 196608 * fmt.sample_bytes() * (fmt.sample_rate // 1000) // 2048) // unit)
    with open(path, "rb") as fh:
        fh.seek(fmt.data_offset)
        done = 0
        while done < n_units:
            take = min(per_block, n_units - done)
            feed.push(fh.read(take * unit))
            done += take
            before = engine.stats(stream)["frames"]
            engine.process(block_frames + 1)
            frames += engine.stats(stream)["frames"] - before
            if on_block:
                on_block(engine)
    feed.close()
    return frames


class FibdecInfo(C.Structure):
    _fields_ = [("fibs_processed", C.c_int64), ("fig00_fib", C.c_int64), ("last_change_fib", C.c_int64), ("cif_count", C.c_int32),
                ("cif_count_hi", C.c_int32), ("cif_count_lo", C.c_int32), ("change_flags", C.c_int32), ("occurrence_change", C.c_int32),
                ("n_changes", C.c_int32), ("n_restarts", C.c_int32), ("reserved", C.c_int32 * 3)]


class Reconf(C.Structure):
    _fields_ = [("pending", C.c_int32), ("n_changes", C.c_int32), ("frames_missed", C.c_int32), ("reserved", C.c_int32),
                ("at_cif", C.c_int64), ("last_change_cif", C.c_int64), ("frames_fed", C.c_int64)]


class FibDecoder:
    """dabx_fibdec_*: FibDecoder's FIG 0/0-0/2 walk with a current and a next configuration (host only)."""

    def __init__(self, reference_quirks=False):
        self._h = C.c_void_p()
        check(load().dabx_fibdec_create(C.byref(self._h)))
        if reference_quirks:
            check(load().dabx_fibdec_set_reference_quirks(self._h, 1))

    def process(self, fibs, crc_ok):
        fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
        crc_ok = np.ascontiguousarray(crc_ok, np.uint8).reshape(-1)
        return check(load().dabx_fibdec_process(self._h, _p(fibs), _p(crc_ok), fibs.shape[0]))

    def info(self):
        out = FibdecInfo()
        check(load().dabx_fibdec_get_info(self._h, C.byref(out)))
        return {k: getattr(out, k) for k, _ in FibdecInfo._fields_ if not k.startswith("reserved")}

    def subchannels(self, next=False, max_out=64):
        out = (SubchDesc * max_out)()
        n = check(load().dabx_fibdec_subchannels(self._h, int(next), out, max_out))
        return [out[i] for i in range(n)]

    def packet_components(self, next=False, max_out=64):
        """FIG 0/3 (+ the SId of the FIG 0/2 TMId-3 component that names the SCId): [n] PACKET_COMPONENT."""
        L = load()
        out = np.zeros(max(1, max_out), PACKET_COMPONENT)
        n = check(L.dabx_fibdec_packet_components(self._h, int(next), _p(out), max_out))
        return out[:n]

    def reset(self):
        check(load().dabx_fibdec_reset(self._h))

    def close(self):
        if self._h and _LIB is not None:
            _LIB.dabx_fibdec_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_fibs(fibs, crc_ok, max_out=64):
    """FIB/FIG subset (host only): -> (list of SubchDesc, cif_count)."""
    fibs = np.ascontiguousarray(fibs, np.uint8).reshape(-1, 32)
    crc_ok = np.ascontiguousarray(crc_ok, np.uint8).reshape(-1)
    out = (SubchDesc * max_out)()
    cif = C.c_int32(-1)
    n = check(load().dabx_parse_fibs(_p(fibs), _p(crc_ok), fibs.shape[0], out, max_out, C.byref(cif)))
    return [out[i] for i in range(n)], cif.value


def fic_decode(soft):
    """soft: [batch, 3*3072] int16 (OFDM symbols 1..3) -> (fibs [batch,12,32], crc_ok [batch,12])."""
    soft = np.ascontiguousarray(soft, np.int16).reshape(-1, 9216)
    fibs = np.zeros((soft.shape[0], 12, 32), np.uint8)
    crc = np.zeros((soft.shape[0], 12), np.uint8)
    check(load().dabx_fic_decode(_p(soft), soft.shape[0], _p(fibs), _p(crc)))
    return fibs, crc
