// engine_facade.cpp -- dabx_fic_decode, the per-symbol facades dabx_fic_* and dabx_msc_*, and the dabx_internal_* test entries of the demapper,
// the FIC and the MSC stages.
#include "engine.h"
#include "viterbi_core.h"
#include <cstring>
#include <vector>

// The light engine of dabx_fic_decode and dabx_fic_create: FIC only, `batch` streams, without the IQ ring (large for a big batch) -- control
// records with frame_ok = 1, FIC symbols, FIB outputs and Viterbi scratch.  On failure the caller destroys *out (null: nothing was created).
static int fic_engine_create(int batch, dabx_engine **out)
{
  auto *e = *out = new dabx_engine();
  (void)hipGetDevice(&e->device);
  if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; *out = nullptr; return DABX_E_HIP; }
  e->ss.a = e->stream;
  EngineDev &d = e->dev;
  d.n_streams = batch; d.max_subch = 0; d.out_frames = 1; d.fic_only = 1;
  d.vit_stride = (int)vit_scratch_words(FIC_OUT);
  int rc;
  if ((rc = e->alloc(&d.ctl, batch)) || (rc = e->alloc(&d.fic_sym, (size_t)batch * 3 * K2)) || (rc = e->alloc(&d.fib_out, (size_t)batch * 384)) ||
      (rc = e->alloc(&d.fib_crc, (size_t)batch * 12)) || (rc = e->alloc(&d.vit_scratch, (size_t)batch * 4 * d.vit_stride, false))) return rc;
  std::vector<StreamCtl> ctl(batch);
  for (auto &c : ctl) { memset(&c, 0, sizeof(c)); c.frame_ok = 1; }
  DABX_HIP(hipMemcpyAsync(d.ctl, ctl.data(), sizeof(StreamCtl) * batch, hipMemcpyHostToDevice, e->stream));
  DABX_HIP(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" {

// ---- stage-level FIC decode through the pipeline kernel (FicDecoder::process_block x 3) ------------
int dabx_fic_decode(const int16_t *soft, int batch, uint8_t *fibs, uint8_t *crc_ok)
{
  if (!soft || !fibs || !crc_ok || batch <= 0) { set_error("dabx_fic_decode: bad argument"); return DABX_E_ARG; }
  int rc = need_device_e();
  if (rc) return rc;
  dabx_engine *e = nullptr;
  if ((rc = fic_engine_create(batch, &e))) { dabx_destroy(e); return rc; }
  EngineDev &d = e->dev;
#define A(x) if ((rc = (x))) { dabx_destroy(e); return rc; }
  int16_t *dsoft = nullptr;
  A(e->alloc(&dsoft, (size_t)batch * 3 * K2, false));
  DABX_HIP(hipMemcpyAsync(dsoft, soft, sizeof(int16_t) * (size_t)batch * 3 * K2, hipMemcpyHostToDevice, e->stream));
  A(launch_i16_to_sym(dsoft, d.fic_sym, (size_t)batch * 3 * K2, e->stream));
  A(launch_fic_only(d, e->stream, 0, 4));
#undef A
  DABX_HIP(hipStreamSynchronize(e->stream));
  DABX_HIP(hipMemcpy(fibs, d.fib_out, (size_t)batch * 384, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(crc_ok, d.fib_crc, (size_t)batch * 12, hipMemcpyDeviceToHost));
  dabx_destroy(e);
  return 0;
}

}  // extern "C"

// ====================================================================================================================
// Per-symbol, stateful stage entries: the GPU side of the reference's FicDecoder and MscHandler CLASS surface
// (fic_decoder.h:42-58, msc_handler.h:36-47).  Both reuse the engine's kernels on the state of a one-stream engine: what
// the frame-batched path does for 512 ensembles at once these do for one ensemble, one OFDM symbol per call.
// ====================================================================================================================
struct dabx_fic {
  dabx_engine *eng = nullptr;        // light-weight: control record, FIC symbols, FIB outputs, Viterbi scratch only
  int16_t *soft_dev = nullptr;       // staging of one symbol's soft bits
  bool running = true;               // mIsRunning (the shim calls restart() from DabProcessor::start like the reference)
  int index = 0, fic_idx = 0;        // mIndex / mFicIdx: soft bits collected of the current FIC block, next block
};

extern "C" {

int dabx_fic_create(dabx_fic **out)
{
  if (!out) { set_error("dabx_fic_create: bad argument"); return DABX_E_ARG; }
  int rc = need_device_e();
  if (rc) return rc;
  auto *f = new dabx_fic();
  if ((rc = fic_engine_create(1, &f->eng)) || (rc = f->eng->alloc(&f->soft_dev, (size_t)K2, false))) { dabx_fic_destroy(f); return rc; }
  *out = f;
  return 0;
}

void dabx_fic_destroy(dabx_fic *f)
{
  if (!f) return;
  dabx_destroy(f->eng);
  delete f;
}

int dabx_fic_process_block(dabx_fic *f, const int16_t *soft, int sym_idx, int *first_fic)
{
  if (!f || !soft || sym_idx < 1 || sym_idx > 3) { set_error("dabx_fic_process_block: bad argument"); return DABX_E_ARG; }
  dabx_engine *e = f->eng;
  if (int rc = use_device(e)) return rc;
  if (sym_idx == 1) { f->index = 0; f->fic_idx = 0; }            // fic_decoder.cpp:148-152
  // the 3072 soft bits continue the running FIC block; blocks complete at 2304-bit boundaries (:154-165)
  const int pos0 = f->fic_idx * FIC_IN + f->index;               // position in the frame's 9216 FIC soft bits
  if (pos0 + K2 > 3 * K2) { set_error("dabx_fic_process_block: symbols out of order"); return DABX_E_STATE; }
  const int done_before = f->fic_idx;
  const int total = f->index + K2;
  const int completed = total / FIC_IN;
  f->index = total % FIC_IN;
  f->fic_idx += completed;
  if (first_fic) *first_fic = done_before;
  if (!f->running) return 0;                                     // :182-185: _process_fic_input returns at once
  DABX_HIP(hipMemcpyAsync(f->soft_dev, soft, sizeof(int16_t) * K2, hipMemcpyHostToDevice, e->stream));
  int rc = launch_i16_to_sym(f->soft_dev, e->dev.fic_sym + pos0, (size_t)K2, e->stream);
  if (rc) return rc;
  if (completed > 0 && (rc = launch_fic_only(e->dev, e->stream, done_before, completed))) return rc;
  DABX_HIP(hipStreamSynchronize(e->stream));
  return completed;
}

int dabx_fic_get_fibs(dabx_fic *f, int fic_idx, uint8_t fibs[96], uint8_t crc_ok[3])
{
  if (!f || fic_idx < 0 || fic_idx > 3 || !fibs || !crc_ok) return DABX_E_ARG;
  if (int rc = sync_all(f->eng)) return rc;
  DABX_HIP(hipMemcpy(fibs, f->eng->dev.fib_out + 96 * fic_idx, 96, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(crc_ok, f->eng->dev.fib_crc + 3 * fic_idx, 3, hipMemcpyDeviceToHost));
  return 0;
}

int dabx_fic_get_fib_bits(dabx_fic *f, uint8_t *bits, uint8_t *valid)
{
  if (!f || !bits || !valid) return DABX_E_ARG;
  if (int rc = sync_all(f->eng)) return rc;
  uint8_t packed[384], crc[12];
  DABX_HIP(hipMemcpy(packed, f->eng->dev.fib_out, 384, hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(crc, f->eng->dev.fib_crc, 12, hipMemcpyDeviceToHost));
  for (int i = 0; i < 3072; i++) bits[i] = (uint8_t)((packed[i >> 3] >> (7 - (i & 7))) & 1);
  for (int g = 0; g < 4; g++) valid[g] = (uint8_t)(crc[3 * g] && crc[3 * g + 1] && crc[3 * g + 2]);
  return 0;
}

static int fic_ctl(dabx_fic *f, StreamCtl *c)
{
  if (int rc = sync_all(f->eng)) return rc;
  DABX_HIP(hipMemcpy(c, f->eng->dev.ctl, sizeof(StreamCtl), hipMemcpyDeviceToHost));
  return 0;
}
int dabx_fic_get_decode_ratio_percent(dabx_fic *f)
{
  if (!f) return DABX_E_ARG;
  StreamCtl c;
  if (int rc = fic_ctl(f, &c)) return rc;
  return c.fic_ratio * 10;
}
int dabx_fic_get_cif_count(dabx_fic *f)
{
  if (!f) return DABX_E_ARG;
  StreamCtl c;
  if (int rc = fic_ctl(f, &c)) return rc;
  return c.cif_count;
}
int dabx_fic_get_ber(dabx_fic *f, dabx_fic_ber *out)
{
  if (!f || !out) return DABX_E_ARG;
  StreamCtl c;
  if (int rc = fic_ctl(f, &c)) return rc;
  memset(out, 0, sizeof(*out));
  out->bits = c.fic_bits; out->errors = c.fic_errors; out->status_bits = c.fic_status_bits; out->status_errors = c.fic_status_errors;
  out->blocks = c.fic_block;
  return 0;
}
int dabx_fic_reset_decode_success_ratio(dabx_fic *f)
{
  if (!f) return DABX_E_ARG;
  StreamCtl c;
  if (int rc = fic_ctl(f, &c)) return rc;
  c.fic_ratio = 0;
  DABX_HIP(hipMemcpy(f->eng->dev.ctl, &c, sizeof(StreamCtl), hipMemcpyHostToDevice));
  return 0;
}
int dabx_fic_stop(dabx_fic *f) { if (!f) return DABX_E_ARG; f->running = false; return 0; }
int dabx_fic_restart(dabx_fic *f)
{
  if (!f) return DABX_E_ARG;
  if (int rc = dabx_fic_reset_decode_success_ratio(f)) return rc;
  f->running = true;
  return 0;
}

}  // extern "C"

// ---- test entries of the batched MSC decoder (tests/test_gpu_msc_decoder.py; not part of include/dabx.h) ---------------------------
// Soft bits go straight into the time-de-interleaver ring and k_msc_prep / k_msc_vitT (or k_msc_frame) decode them exactly as
// dabx_process launches them: no IQ, no front-end kernel.  Between two decodes the ring holds the 16 CIFs of history in front of a
// stream's CIF counter and at most one batch of new CIFs behind it: that is what `first + n_cifs` is checked against, so that no
// call can overwrite history the next batch reads (TDI_SLOTS = 64 >= 16 + 4 * MSC_BATCH_FRAMES).
extern "C" {

// soft: [n_cifs][55296] int16, the whole CIFs cif_no + first .. cif_no + first + n_cifs - 1 of `stream` (cif_no: the stream's CIF counter,
// which only dabx_internal_msc_decode moves), converted with the engine's viterbi_tie_mode as the demapper's output is.
int dabx_internal_msc_inject(dabx_engine *e, int stream, const int16_t *soft, int n_cifs, int first)
{
  constexpr int HOLD = 4 * MSC_BATCH_FRAMES;
  if (!e || !soft || stream < 0 || stream >= e->dev.n_streams || n_cifs < 1 || n_cifs > HOLD || first < 0 || first > HOLD - n_cifs || !e->dev.tdi) {
    set_error("dabx_internal_msc_inject: bad argument (stream %d, CIFs %d + %d of at most %d)", stream, first, n_cifs, HOLD);
    return DABX_E_ARG;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  int16_t *soft_dev = nullptr;
  const size_t bytes = (size_t)n_cifs * CIF_BITS * sizeof(int16_t);
  DABX_HIP(hipMalloc(&soft_dev, bytes));
  int rc = 0;
  if (hipMemcpy(soft_dev, soft, bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_internal_msc_inject: copy failed"); rc = DABX_E_HIP; }
  if (!rc) rc = launch_msc_inject(e->dev, stream, soft_dev, n_cifs, first, e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess && !rc) { set_error("dabx_internal_msc_inject: HIP error"); rc = DABX_E_HIP; }
  (void)hipFree(soft_dev);
  return rc;
}

// cifs_per_stream: [n_streams], how many of the injected CIFs every stream counts as received (0 .. batch_cifs); then one MSC batch of
// batch_cifs CIFs, launched as dabx_process launches it, and a full synchronisation.  Results: dabx_read_msc, dabx_get_subch_stats.
int dabx_internal_msc_decode(dabx_engine *e, const int32_t *cifs_per_stream, int batch_cifs)
{
  if (!e || !cifs_per_stream || batch_cifs < 1 || batch_cifs > 4 * MSC_BATCH_FRAMES) {
    set_error("dabx_internal_msc_decode: bad argument (batch of %d CIFs, at most %d)", batch_cifs, 4 * MSC_BATCH_FRAMES);
    return DABX_E_ARG;
  }
  for (int s = 0; s < e->dev.n_streams; s++)
    if (cifs_per_stream[s] < 0 || cifs_per_stream[s] > batch_cifs) {
      set_error("dabx_internal_msc_decode: %d CIFs for stream %d in a batch of %d", (int)cifs_per_stream[s], s, batch_cifs);
      return DABX_E_ARG;
    }
  if (e->dl.open || e->pending_frames != 0) {
    set_error("dabx_internal_msc_decode: the engine has a delivery open or front-end frames pending");
    return DABX_E_STATE;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  if (e->classes_dirty) {
    if (int rc = e->build_msc_classes()) return rc;
    e->classes_dirty = false;
  }
  int32_t *counts_dev = nullptr;
  const size_t bytes = sizeof(int32_t) * (size_t)e->dev.n_streams;
  DABX_HIP(hipMalloc(&counts_dev, bytes));
  int rc = 0;
  if (hipMemcpy(counts_dev, cifs_per_stream, bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_internal_msc_decode: copy failed"); rc = DABX_E_HIP; }
  if (!rc) rc = launch_msc_advance(e->dev, counts_dev, e->stream);
  if (!rc) {
    e->dev.snap = e->snap_buf[e->ss.batch_parity];
    rc = launch_msc_batch(e->dev, batch_cifs, e->have_fast ? &e->fast : nullptr, e->ss, e->mk, nullptr, nullptr, e->pkt.dev.n > 0 ? &e->pkt.dev : nullptr,
                          e->pad.dev.n > 0 ? &e->pad.dev : nullptr, e->mot.dev.n > 0 ? &e->mot.dev : nullptr, e->car.dev.n > 0 ? &e->car.dev : nullptr,
                          nullptr, e->mpa.dev.n > 0 ? &e->mpa.dev : nullptr, &e->mpa_launches, e->aac.dev.n > 0 ? &e->aac.dev : nullptr, &e->aac_launches,
                          e->dat.dev.n > 0 ? &e->dat.dev : nullptr, &e->dat_ctl);
  }
  const int rc2 = sync_all(e);
  (void)hipFree(counts_dev);
  return rc ? rc : rc2;
}

// ---- test entries of the FIC stage (tests/test_gpu_fic_stage.py; not part of include/dabx.h) ----------------------------------------
// soft: [9216] int16, the FIC soft bits of the next frame of `stream` (OFDM symbols 1..3), converted with the engine's viterbi_tie_mode
// as the demapper's output is.  Nothing is decoded or counted before dabx_internal_fic_decode.
int dabx_internal_fic_inject(dabx_engine *e, int stream, const int16_t *soft)
{
  if (!e || !soft || stream < 0 || stream >= e->dev.n_streams || !e->dev.fic_sym) {
    set_error("dabx_internal_fic_inject: bad argument (stream %d)", stream);
    return DABX_E_ARG;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  int16_t *soft_dev = nullptr;
  const size_t bytes = (size_t)3 * K2 * sizeof(int16_t);
  DABX_HIP(hipMalloc(&soft_dev, bytes));
  int rc = 0;
  if (hipMemcpy(soft_dev, soft, bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_internal_fic_inject: copy failed"); rc = DABX_E_HIP; }
  if (!rc) rc = launch_fic_inject(e->dev, stream, soft_dev, e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess && !rc) { set_error("dabx_internal_fic_inject: HIP error"); rc = DABX_E_HIP; }
  (void)hipFree(soft_dev);
  return rc;
}

// present: [n_streams], 1 = the stream has a frame (frame_ok), 0 = it has none: k_fic_frame must leave everything of that stream as it
// is.  One launch of k_fic_frame over all streams (first = 0, count = 4, no sequence-number wait), then the present streams count the
// frame (the slot ring of out_frames turns), and a full synchronisation.  Results: dabx_read_fibs, dabx_get_stats.
int dabx_internal_fic_decode(dabx_engine *e, const int32_t *present)
{
  if (!e || !present || !e->dev.fic_sym) { set_error("dabx_internal_fic_decode: bad argument"); return DABX_E_ARG; }
  for (int s = 0; s < e->dev.n_streams; s++)
    if (present[s] != 0 && present[s] != 1) {
      set_error("dabx_internal_fic_decode: present[%d] = %d (0 or 1)", s, (int)present[s]);
      return DABX_E_ARG;
    }
  if (e->dl.open || e->pending_frames != 0) {
    set_error("dabx_internal_fic_decode: the engine has a delivery open or front-end frames pending");
    return DABX_E_STATE;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  int32_t *present_dev = nullptr;
  const size_t bytes = sizeof(int32_t) * (size_t)e->dev.n_streams;
  DABX_HIP(hipMalloc(&present_dev, bytes));
  int rc = 0;
  if (hipMemcpy(present_dev, present, bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_internal_fic_decode: copy failed"); rc = DABX_E_HIP; }
  if (!rc) rc = launch_fic_decode(e->dev, present_dev, e->stream);
  if (!rc) rc = fig_step(e);
  const int rc2 = sync_all(e);
  (void)hipFree(present_dev);
  return rc ? rc : rc2;
}

// ---- test entries of the engine's demapper (tests/test_gpu_demap_stage.py; not part of include/dabx.h) -------------------------------
// spectra: [76][2048] cf32 in FFT bin order, symbols 0..75 of the next frame of `stream`: symbol 0 becomes the stream's phase reference,
// symbols 1..75 go into the engine's spectra buffer of the next step's parity, in carrier order, as k_symbols_persistent stores them.
// null_fft: [2048] cf32 or NULL: advances the noise-power buffer that np_sel selects (the library's own update, null_power_next).
// clock_err and np_sel (0 or 1) go into the stream's control record.  Nothing is demapped before dabx_internal_demap_frame.
int dabx_internal_demap_inject(dabx_engine *e, int stream, const float *spectra, const float *null_fft, float clock_err, int np_sel)
{
  if (!e || !spectra || stream < 0 || stream >= e->dev.n_streams || (np_sel != 0 && np_sel != 1) || !e->dev.spectra) {
    set_error("dabx_internal_demap_inject: bad argument (stream %d, np_sel %d)", stream, np_sel);
    return DABX_E_ARG;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  float2 *buf = nullptr;
  const size_t n_spec = (size_t)76 * TU, n_all = n_spec + TU;
  DABX_HIP(hipMalloc(&buf, n_all * sizeof(float2)));
  int rc = 0;
  if (hipMemcpy(buf, spectra, n_spec * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_internal_demap_inject: copy failed"); rc = DABX_E_HIP; }
  if (!rc && null_fft && hipMemcpy(buf + n_spec, null_fft, TU * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("dabx_internal_demap_inject: copy failed");
    rc = DABX_E_HIP;
  }
  if (!rc) rc = launch_demap_inject(e->dev, (int)(e->ss.step_count & 1u), stream, buf, null_fft ? buf + n_spec : nullptr, clock_err, np_sel, e->stream);
  if (hipStreamSynchronize(e->stream) != hipSuccess && !rc) { set_error("dabx_internal_demap_inject: HIP error"); rc = DABX_E_HIP; }
  (void)hipFree(buf);
  return rc;
}

// present: [n_streams], 1 = the stream has a frame (frame_ok), 0 = it has none: the demapper must leave everything of that stream as it is.
// schedule 0: one k_demap_frame6(0, 75); 1: k_demap_fic, then k_demap_frame6(3, 75); 2: k_demap_whole -- the launches of launch_front_step's
// three schedules, picked by soft-bit type, tie mode and LCD statistics through the same dispatch, without the sequence-number hand-over;
// then a full synchronisation.  Neither the CIF counter nor the frame count moves: dabx_internal_fic_decode and dabx_internal_msc_decode do
// that afterwards.  Results: dabx_read_soft (capture_soft), dabx_get_stats, and what those two decode.
int dabx_internal_demap_frame(dabx_engine *e, const int32_t *present, int schedule)
{
  if (!e || !present || schedule < 0 || schedule > 2 || !e->dev.spectra || !e->dev.fic_sym || !e->dev.tdi) {
    set_error("dabx_internal_demap_frame: bad argument (schedule %d)", schedule);
    return DABX_E_ARG;
  }
  for (int s = 0; s < e->dev.n_streams; s++)
    if (present[s] != 0 && present[s] != 1) {
      set_error("dabx_internal_demap_frame: present[%d] = %d (0 or 1)", s, (int)present[s]);
      return DABX_E_ARG;
    }
  if (e->dl.open || e->pending_frames != 0) {
    set_error("dabx_internal_demap_frame: the engine has a delivery open or front-end frames pending");
    return DABX_E_STATE;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  int32_t *present_dev = nullptr;
  const size_t bytes = sizeof(int32_t) * (size_t)e->dev.n_streams;
  DABX_HIP(hipMalloc(&present_dev, bytes));
  int rc = 0;
  if (hipMemcpy(present_dev, present, bytes, hipMemcpyHostToDevice) != hipSuccess) { set_error("dabx_internal_demap_frame: copy failed"); rc = DABX_E_HIP; }
  const bool scope_on = e->scope.n_on > 0;
  if (!rc) rc = launch_demap_frame(e->dev, e->ss.step_count, present_dev, schedule, e->stream, scope_on ? &e->scope.dev : nullptr);
  if (!rc && scope_on) e->scope.launches++;
  const int rc2 = sync_all(e);
  (void)hipFree(present_dev);
  return rc ? rc : rc2;
}

// ---- test entry of the frame chain (tests/test_gpu_front_stage.py; not part of include/dabx.h) ----------------------------------------
// What k_frame_head, k_symbols_persistent and k_frame_tail of the LAST step left for `stream` of a drained engine, copied out with plain
// hipMemcpy behind a full synchronisation (no kernel).  sc: the record below; phase_ref [2048] cf32 in bin order; spectra [75][1536] cf32 in
// carrier order, from the buffer of the parity that step used; cp_part [75] cf32; abs_part [75]; null_power [2][2048] (DemapDev::null_power,
// then null_power2; sc->np_sel tells which is current); tii_acc [2048] cf32 (left alone when the engine has no TII sum: sc->has_tii = 0).
// Any of the array pointers may be NULL.
struct dabx_front_scalars {
  int32_t frame_ok, np_sel, start_index, correction, f_frame, phase_sym1, nco_phase, has_tii;
  long long frames;
  unsigned long long sym0_pos, rd;
  float f_sync, f_bb, phase_offs, clock_err;
  int32_t tii_cnt[2], parity, pad_;
};
static_assert(sizeof(dabx_front_scalars) == 88, "dabx_front_scalars: dabstar_amd/lib.py reads it as a packed record of 88 bytes");

int dabx_internal_front_read(dabx_engine *e, int stream, dabx_front_scalars *sc, float *phase_ref, float *spectra, float *cp_part, float *abs_part,
                             float *null_power, float *tii_acc)
{
  if (!e || !sc || stream < 0 || stream >= e->dev.n_streams || !e->dev.spectra || !e->dev.cp_part || !e->dev.abs_part || !e->dev.demap.phase_ref) {
    set_error("dabx_internal_front_read: bad argument (stream %d)", stream);
    return DABX_E_ARG;
  }
  if (e->dl.open || e->pending_frames != 0) {
    set_error("dabx_internal_front_read: the engine has a delivery open or front-end frames pending");
    return DABX_E_STATE;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  const EngineDev &d = e->dev;
  const size_t s = (size_t)stream;
  StreamCtl c;
  DABX_HIP(hipMemcpy(&c, d.ctl + s, sizeof(StreamCtl), hipMemcpyDeviceToHost));
  memset(sc, 0, sizeof(*sc));
  sc->frame_ok = c.frame_ok; sc->np_sel = c.np_sel; sc->start_index = c.start_index; sc->correction = c.correction; sc->f_frame = c.f_frame;
  sc->phase_sym1 = c.phase_sym1; sc->nco_phase = c.nco_phase; sc->frames = c.frames; sc->sym0_pos = c.sym0_pos; sc->rd = c.rd;
  sc->f_sync = c.f_sync; sc->f_bb = c.f_bb; sc->phase_offs = c.phase_offs; sc->clock_err = c.clock_err;
  sc->parity = e->ss.step_count ? (int)((e->ss.step_count - 1) & 1u) : 0;            // launch_front_step: parity = step_count++ & 1
  sc->has_tii = d.tii_acc && d.tii_cnt;
  if (sc->has_tii) DABX_HIP(hipMemcpy(sc->tii_cnt, d.tii_cnt + 2 * s, 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (phase_ref) DABX_HIP(hipMemcpy(phase_ref, d.demap.phase_ref + s * TU, TU * sizeof(float2), hipMemcpyDeviceToHost));
  if (spectra)
    DABX_HIP(hipMemcpy(spectra, d.spectra + ((size_t)sc->parity * d.n_streams + s) * 75 * K, (size_t)75 * K * sizeof(float2), hipMemcpyDeviceToHost));
  if (cp_part) DABX_HIP(hipMemcpy(cp_part, d.cp_part + s * 75, 75 * sizeof(float2), hipMemcpyDeviceToHost));
  if (abs_part) DABX_HIP(hipMemcpy(abs_part, d.abs_part + s * 76, 75 * sizeof(float), hipMemcpyDeviceToHost));
  if (null_power) {
    DABX_HIP(hipMemcpy(null_power, d.demap.null_power + s * TU, TU * sizeof(float), hipMemcpyDeviceToHost));
    DABX_HIP(hipMemcpy(null_power + TU, d.demap.null_power2 + s * TU, TU * sizeof(float), hipMemcpyDeviceToHost));
  }
  if (tii_acc && sc->has_tii) DABX_HIP(hipMemcpy(tii_acc, d.tii_acc + s * TU, TU * sizeof(float2), hipMemcpyDeviceToHost));
  return 0;
}

// ---- test entry of the DC / IQ correction (tests/test_gpu_dciq_stage.py; not part of include/dabx.h) -----------------------------------
// What k_dciq carries from launch to launch for `stream`: state = meanI, meanQ, meanII, meanQQ, meanIQ (EngineDev::dciq_state, the first
// five of the stream's eight floats) and *done = the absolute index of the first sample not yet corrected (EngineDev::dciq_done), copied
// out with plain hipMemcpy behind a full synchronisation (no kernel).  An engine without the correction has the initial values.
int dabx_internal_dciq_read(dabx_engine *e, int stream, float *state, uint64_t *done)
{
  if (!e || !state || !done || stream < 0 || stream >= e->dev.n_streams || !e->dev.dciq_state || !e->dev.dciq_done) {
    set_error("dabx_internal_dciq_read: bad argument (stream %d)", stream);
    return DABX_E_ARG;
  }
  if (int rc = use_device(e)) return rc;
  if (int rc = sync_all(e)) return rc;
  unsigned long long upto = 0;
  DABX_HIP(hipMemcpy(state, e->dev.dciq_state + (size_t)stream * 8, 5 * sizeof(float), hipMemcpyDeviceToHost));
  DABX_HIP(hipMemcpy(&upto, e->dev.dciq_done + stream, sizeof(upto), hipMemcpyDeviceToHost));
  *done = (uint64_t)upto;
  return 0;
}

}  // extern "C"

struct dabx_msc {
  dabx_engine *eng = nullptr;              // one-stream engine: TDI ring, sub-channel slots, output rings, DAB+ stage
  int16_t *soft_dev = nullptr;
  std::vector<dabx_subch_desc> slots;      // kbps == 0: free
  std::vector<long long> frames_seen, sf_seen;   // per slot: logical / super frames that existed before the CIF just closed
  std::vector<long long> frames_now, sf_now;
};

static int msc_apply(dabx_msc *m)
{
  return dabx_set_subchannels(m->eng, 0, m->slots.data(), (int)m->slots.size());
}

extern "C" {

int dabx_msc_create(int max_services, dabx_msc **out)
{
  if (!out || max_services < 1 || max_services > MAX_SUBCH) { set_error("dabx_msc_create: bad argument"); return DABX_E_ARG; }
  dabx_config cfg;
  dabx_default_config(&cfg);
  cfg.n_streams = 1; cfg.ring_frames = 2; cfg.max_subch = max_services; cfg.out_frames = 1;
  auto *m = new dabx_msc();
  int rc = dabx_create(&cfg, &m->eng);
  if (rc) { delete m; return rc; }
  if ((rc = m->eng->alloc(&m->soft_dev, (size_t)K2, false))) { dabx_msc_destroy(m); return rc; }
  m->slots.assign((size_t)max_services, dabx_subch_desc{});
  m->frames_seen.assign((size_t)max_services, 0); m->sf_seen.assign((size_t)max_services, 0);
  m->frames_now.assign((size_t)max_services, 0); m->sf_now.assign((size_t)max_services, 0);
  *out = m;
  return 0;
}

void dabx_msc_destroy(dabx_msc *m)
{
  if (!m) return;
  dabx_destroy(m->eng);
  delete m;
}

int dabx_msc_set_channel(dabx_msc *m, const dabx_subch_desc *d)
{
  if (!m || !d || d->kbps <= 0) { set_error("dabx_msc_set_channel: bad argument"); return DABX_E_ARG; }
  int slot = -1;
  for (size_t j = 0; j < m->slots.size() && slot < 0; j++) if (!m->slots[j].kbps) slot = (int)j;
  if (slot < 0) { set_error("dabx_msc_set_channel: all %zu service slots in use", m->slots.size()); return DABX_E_STATE; }
  m->slots[(size_t)slot] = *d;
  if (m->slots[(size_t)slot].dab_plus < 0) m->slots[(size_t)slot].dab_plus = (d->kbps <= 384 && d->kbps % 8 == 0) ? 1 : 0;
  const int rc = msc_apply(m);
  if (rc) { m->slots[(size_t)slot] = dabx_subch_desc{}; return rc; }
  m->frames_seen[(size_t)slot] = m->sf_seen[(size_t)slot] = m->frames_now[(size_t)slot] = m->sf_now[(size_t)slot] = 0;
  return slot;
}

int dabx_msc_stop_service(dabx_msc *m, int slot)
{
  if (!m || slot < 0 || slot >= (int)m->slots.size()) return DABX_E_ARG;
  m->slots[(size_t)slot] = dabx_subch_desc{};
  return msc_apply(m);
}

int dabx_msc_stop_all_services(dabx_msc *m)
{
  if (!m) return DABX_E_ARG;
  for (auto &s : m->slots) s = dabx_subch_desc{};
  return msc_apply(m);
}

int dabx_msc_is_service_running(dabx_msc *m, int slot)
{
  if (!m || slot < 0 || slot >= (int)m->slots.size()) return DABX_E_ARG;
  return m->slots[(size_t)slot].kbps != 0;
}

int dabx_msc_process_block(dabx_msc *m, const int16_t *soft, int blk_nr)
{
  if (!m || !soft || blk_nr < 4 || blk_nr >= L) { set_error("dabx_msc_process_block: bad argument"); return DABX_E_ARG; }
  dabx_engine *e = m->eng;
  if (int rc = use_device(e)) return rc;
  if (e->classes_dirty) {                       // one stream never reaches the lane-per-trellis path, but the slots' class tags must be current
    if (int rc = e->build_msc_classes()) return rc;
    e->classes_dirty = false;
  }
  const int cur = (blk_nr - 4) % 18;            // msc_handler.cpp:145
  const bool closes = cur == 17;
  DABX_HIP(hipMemcpyAsync(m->soft_dev, soft, sizeof(int16_t) * K2, hipMemcpyHostToDevice, e->stream));
  int rc = launch_stage_msc_block(e->dev, m->soft_dev, cur, closes, e->stream);
  if (rc) return rc;
  if (!closes) { DABX_HIP(hipStreamSynchronize(e->stream)); return 0; }
  // a full CIF: every back end runs (msc_handler.cpp:155-167)
  e->dev.snap = e->snap_buf[e->ss.batch_parity];
  if ((rc = launch_msc_batch(e->dev, 1, nullptr, e->ss, e->mk))) return rc;
  if ((rc = sync_all(e))) return rc;
  std::vector<SubchDev> sc(m->slots.size());
  DABX_HIP(hipMemcpy(sc.data(), e->dev.subch, sizeof(SubchDev) * sc.size(), hipMemcpyDeviceToHost));
  for (size_t j = 0; j < sc.size(); j++) {
    m->frames_seen[j] = m->frames_now[j]; m->sf_seen[j] = m->sf_now[j];
    m->frames_now[j] = sc[j].active ? sc[j].cif_out : 0;
    m->sf_now[j] = sc[j].active ? sc[j].sf_count : 0;
  }
  return 1;
}

int dabx_msc_get_frame(dabx_msc *m, int slot, uint8_t *bytes, int max_bytes)
{
  if (!m || slot < 0 || slot >= (int)m->slots.size() || !bytes) return DABX_E_ARG;
  const size_t j = (size_t)slot;
  if (!m->slots[j].kbps || m->frames_now[j] == m->frames_seen[j]) return 0;       // de-interleaver still filling / no new CIF
  const int nb = 3 * m->slots[j].kbps;
  if (max_bytes < nb) { set_error("dabx_msc_get_frame: %d bytes needed", nb); return DABX_E_ARG; }
  const int got = dabx_read_msc(m->eng, 0, slot, 1, bytes);
  return got < 0 ? got : (got == 1 ? nb : 0);
}

int dabx_msc_get_superframe(dabx_msc *m, int slot, uint8_t *bytes, int max_bytes)
{
  if (!m || slot < 0 || slot >= (int)m->slots.size() || !bytes) return DABX_E_ARG;
  const size_t j = (size_t)slot;
  if (!m->slots[j].kbps || m->sf_now[j] == m->sf_seen[j]) return 0;
  const int nb = 110 * m->slots[j].kbps / 8;
  if (max_bytes < nb) { set_error("dabx_msc_get_superframe: %d bytes needed", nb); return DABX_E_ARG; }
  const int got = dabx_read_superframes(m->eng, 0, slot, 1, bytes);
  return got < 0 ? got : (got == 1 ? nb : 0);
}

int dabx_msc_get_superframe_info(dabx_msc *m, int slot, dabx_superframe_info *out)
{
  if (!m || slot < 0 || slot >= (int)m->slots.size() || !out) return DABX_E_ARG;
  const size_t j = (size_t)slot;
  if (!m->slots[j].kbps || m->sf_now[j] == m->sf_seen[j]) return 0;
  const int got = dabx_read_superframe_info(m->eng, 0, slot, 1, out);
  return got < 0 ? got : (got == 1 ? 1 : 0);
}

int dabx_msc_get_stats(dabx_msc *m, int slot, dabx_subch_stats *out)
{
  if (!m) return DABX_E_ARG;
  return dabx_get_subch_stats(m->eng, 0, slot, out);
}

}  // extern "C"
