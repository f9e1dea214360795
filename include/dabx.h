/*
 * dabx.h -- C ABI of libdabx: MI355X-native OFDM-demodulation + FEC back end for DAB/DAB+ Mode I.
 *
 * Drop-in boundary for the one hot path of tomneda/DABstar (reference tree /root/reference, paths
 * below relative to its src/).  The reference has no FFI seam: the seam is the C++ class surface
 * OfdmDecoder / FicDecoder / MscHandler selected at compile time (base/main/dab_processor.h:53-57
 * picks ofdm_decoder_simd.h or ofdm_decoder.h).  A HIP back end enters as a third alternative; the
 * functions below are what that alternative binds to (see INTEGRATION.md for the C++ stub).
 *
 * Conventions: extern "C", plain pointers and sizes, int return codes (0 = ok, <0 = dabx_err),
 * caller-allocated buffers, no exceptions cross the boundary, one caller thread per handle.
 * Functions ending in _dev take DEVICE pointers (HBM-resident batches); all others take HOST
 * pointers and stage through the device themselves.  There is no CPU fallback: every entry point
 * fails with DABX_E_NODEVICE when no HIP device is usable.
 */
#ifndef DABX_H
#define DABX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DABX_ABI_VERSION 6

typedef enum {
  DABX_OK = 0,
  DABX_E_NODEVICE = -1,   /* no usable HIP device / kernel image not loadable */
  DABX_E_ARG = -2,        /* bad argument */
  DABX_E_PROFILE = -3,    /* illegal (bit rate, protection level) combination */
  DABX_E_HIP = -4,        /* HIP runtime error (see dabx_last_error) */
  DABX_E_STATE = -5,      /* call not valid in this state */
  DABX_E_NOMEM = -6
} dabx_err;

/* Mode-I constants, common/glob_defs.h:40-55 */
enum { DABX_L = 76, DABX_K = 1536, DABX_TN = 2656, DABX_TF = 196608, DABX_TS = 2552, DABX_TU = 2048,
       DABX_TG = 504, DABX_2K = 3072, DABX_FIC_IN = 2304, DABX_FIC_OUT = 768, DABX_CIF_BITS = 55296 };

typedef struct { float re, im; } dabx_cf32;

const char *dabx_last_error(void);
int dabx_abi_version(void);
/* Selects the HIP device for the calling thread's subsequent dabx calls (default 0). */
int dabx_set_device(int device);
int dabx_device_count(void);

/* ===================================================================================== stage level
 * Each entry mirrors one reference function; batch = number of independent problems.           */

/* ViterbiSpiral::deconvolve (base/support/viterbi_spiral/viterbi_spiral.h:20, .cpp:95-126):
 * soft  : batch x 4*(nbits+6) int16 mother-code soft bits (0 at punctured positions)
 * bits  : batch x nbits bytes, one decoded bit per byte.  Canonical scalar tie rule. */
int dabx_viterbi(const int16_t *soft, int nbits, int batch, uint8_t *bits);
/* The same with the decoder arithmetic selected: tie_mode 0 = the canonical scalar body (viterbi_scalar.h: int32 metrics, a
 * tie keeps predecessor i); 1 = the reference's VITERBI_AVX2 build (viterbi_16way.h:9-58: uint16 saturating metrics,
 * renormalisation above 60000, a tie goes to predecessor i + 32); 2 = its VITERBI_SSE2 / NEON builds (viterbi_8way.h:9-53:
 * signed int16 metrics saturating at 32767, renormalisation above 30000, ties as in the scalar body).  Each is bit-identical
 * to the respective object code of the reference. */
int dabx_viterbi_mode(const int16_t *soft, int nbits, int batch, int tie_mode, uint8_t *bits);

/* Protection::deconvolve for EEP/UEP (base/protection/protection.h:44; eep_protection.cpp:43-167,
 * uep_protection.cpp:52-212): in = batch x cu_size*64 punctured soft bits; out = batch x 24*kbps bits
 * (one per byte, NOT yet de-dispersed).  short_form != 0 selects the UEP table. */
int dabx_deconvolve(const int16_t *in, int in_stride, int kbps, int prot_level, int short_form, int batch,
                    uint8_t *bits);
/* Size in soft bits (cu_size*64) of a legal profile, or DABX_E_PROFILE. */
int dabx_profile_input_bits(int kbps, int prot_level, int short_form);
/* Host only: the depuncture index list of a profile (96*kbps + 24 entries: mother-code bit i comes from transmitted bit
 * map[i], 0xFFFF = punctured) -- EepProtection / UepProtection constructors, eep_protection.cpp:43-150,
 * uep_protection.cpp:136-196.  Returns the number of transmitted bits. */
int dabx_profile_map(int kbps, int prot_level, int short_form, uint16_t *map, int max_entries);

/* FicDecoder::process_block x3 (base/decoder/fic_decoder.h:49, .cpp:143-262): soft = batch x 9216
 * int16 (OFDM symbols 1..3); fibs = batch x 12 x 32 bytes (packed, de-dispersed);
 * crc_ok = batch x 12 flags. */
int dabx_fic_decode(const int16_t *soft, int batch, uint8_t *fibs, uint8_t *crc_ok);

/* ---- FicDecoder, per OFDM symbol and stateful (base/decoder/fic_decoder.h:42-58) -------------------------------------
 * The handle is the GPU-side FicDecoder of ONE ensemble: what the `FicDecoder` class of the HIP build of the reference
 * (shim/fic_decoder_hip.h) binds to.  dabx_fic_process_block == FicDecoder::process_block(iOfdmSoftBits, iOfdmSymbIdx)
 * (.cpp:143-167): sym_idx = 1, 2, 3; soft = the 3072 int16 soft bits of that symbol.  A FIC block is decoded as soon as
 * its 2304 soft bits are complete, exactly when the reference calls _process_fic_input: block 0 during symbol 1, block 1
 * during symbol 2, blocks 2 and 3 during symbol 3.  Returns the number of FIC blocks this call completed (0..2; 0 also
 * while stopped); *first_fic (optional) = index of the first of them.  Their FIBs -- what the reference hands to
 * IFibDecoder::process_FIB for every FIB whose CRC holds (.cpp:234-261) -- are read with dabx_fic_get_fibs.          */
typedef struct dabx_fic dabx_fic;
int  dabx_fic_create(dabx_fic **out);
void dabx_fic_destroy(dabx_fic *f);
int  dabx_fic_process_block(dabx_fic *f, const int16_t *soft /* 3072 */, int sym_idx, int *first_fic);
/* FIC block fic_idx (0..3) of the current frame: 3 FIBs x 32 packed bytes (de-dispersed) + 3 CRC flags. */
int  dabx_fic_get_fibs(dabx_fic *f, int fic_idx, uint8_t fibs[96], uint8_t crc_ok[3]);
/* FicDecoder::get_fib_bits(u8 *, bool *) (.cpp:310-321): mFibBitsEntireFrame as 3072 bytes holding one bit each and
 * mFicValid[4] (all three FIBs of the block passed their CRC). */
int  dabx_fic_get_fib_bits(dabx_fic *f, uint8_t *bits /* 3072 */, uint8_t *valid /* 4 */);
int  dabx_fic_get_decode_ratio_percent(dabx_fic *f);        /* get_fic_decode_ratio_percent, .cpp:323-326 */
int  dabx_fic_reset_decode_success_ratio(dabx_fic *f);      /* fic_decoder.h:53 */
int  dabx_fic_stop(dabx_fic *f);                            /* stop(): process_block becomes a no-op, .cpp:182-185, 264-268 */
int  dabx_fic_restart(dabx_fic *f);                         /* restart(): ratio = 0, running, .cpp:270-275 */
/* FibDecoder::get_cif_count as the FIG 0/0 walk of the decoded FIBs left it (fib_decoder_fig0.cpp:89-101): hi * 250 + lo; 0 before the
 * first FIG 0/0.  The rule and its limits: dabx_stats.cif_count. */
int  dabx_fic_get_cif_count(dabx_fic *f);
/* The channel BER of the FIC (ViterbiSpiral::calculate_BER, viterbi_spiral.cpp:128-164, driven from fic_decoder.cpp:199-210): the decoded
 * bits re-encoded and compared with the signs of the 2304 transmitted soft bits of every block; both counters are halved after every
 * 40th block.  status_* = the pair as it stood at the newest 40th block BEFORE halving: errors / bits of it is the value the reference
 * hands to signal_fic_status (fic_decoder.cpp:205); blocks = FIC blocks since the last such report (mFicBlock). */
typedef struct { int32_t bits, errors, status_bits, status_errors, blocks, reserved[3]; } dabx_fic_ber;
int  dabx_fic_get_ber(dabx_fic *f, dabx_fic_ber *out);

/* ---- MscHandler, per OFDM symbol and stateful (base/backend/msc_handler.h:36-47, backend.cpp:60-161) --------------
 * The handle is the GPU-side MscHandler of ONE ensemble with up to max_services back ends: the CIF buffer, every back
 * end's 16-CIF time de-interleaver history, depuncture + Viterbi + energy de-dispersal and (for DAB+ services) the
 * Mp4Processor's super-frame synchronisation + RS(120,110) live on the device.
 * dabx_msc_set_channel == MscHandler::set_channel (msc_handler.cpp:123-135): adds a back end for the sub-channel; its
 * de-interleaver starts filling with the next CIF (Backend ctor, backend.cpp:60-84).  Returns the service slot (>= 0).
 * dabx_msc_process_block == MscHandler::process_block(iSoftBits, iBlockNr) (msc_handler.cpp:140-168): blk_nr = 4..75;
 * the block that completes a CIF ((blk_nr - 4) % 18 == 17) runs every back end and returns 1, the others return 0.
 * dabx_msc_get_frame: the logical frame Backend::_process_segment hands to BackendDriver::add_to_frame for that CIF
 * (backend.cpp:140-160) as 3 * kbps PACKED bytes (the reference's outV holds the same 24 * kbps bits one per byte, MSB of
 * byte 0 first); returns the byte count, or 0 while the service's de-interleaver is still filling (first 16 CIFs).
 * dabx_msc_get_superframe: the RS-corrected DAB+ super frame completed by that CIF, if any (110 * kbps / 8 bytes, else 0);
 * dabx_msc_get_superframe_info: its dabx_superframe_info record (returns 1, else 0). */
typedef struct dabx_msc dabx_msc;
struct dabx_subch_desc_s;
int  dabx_msc_create(int max_services, dabx_msc **out);
void dabx_msc_destroy(dabx_msc *m);
int  dabx_msc_set_channel(dabx_msc *m, const struct dabx_subch_desc_s *d);
int  dabx_msc_stop_service(dabx_msc *m, int slot);          /* stop_service, msc_handler.cpp:77-103 (the shim maps SubChId + flag to the slot) */
int  dabx_msc_stop_all_services(dabx_msc *m);               /* msc_handler.cpp:105-118 */
int  dabx_msc_is_service_running(dabx_msc *m, int slot);
int  dabx_msc_process_block(dabx_msc *m, const int16_t *soft /* 3072 */, int blk_nr);
int  dabx_msc_get_frame(dabx_msc *m, int slot, uint8_t *bytes, int max_bytes);
int  dabx_msc_get_superframe(dabx_msc *m, int slot, uint8_t *bytes, int max_bytes);
struct dabx_superframe_info_s;
int  dabx_msc_get_superframe_info(dabx_msc *m, int slot, struct dabx_superframe_info_s *out);
struct dabx_subch_stats_s;
int  dabx_msc_get_stats(dabx_msc *m, int slot, struct dabx_subch_stats_s *out);

/* ReedSolomon::dec(in, out, 135) with (8,0435,0,1,10) (base/backend/reed_solomon.h:28, mp4processor.cpp:63,203):
 * in = batch x 120, out = batch x 110, ret = batch x int16 (#corrected | 0 | -1). */
int dabx_rs_decode(const uint8_t *in, int batch, uint8_t *out, int16_t *ret);

/* FirecodeChecker::check / check_and_correct_6bits (base/backend/firecode_checker.h:42-43):
 * x = batch x 12 bytes (11 used; byte 11 may be touched exactly as in the reference), ok = batch flags */
int dabx_firecode_check(const uint8_t *x, int batch, uint8_t *ok);
int dabx_firecode_check_and_correct(uint8_t *x, int batch, uint8_t *ok);

/* check_crc_bytes (base/backend/crc.cpp:88-96): msgs = batch x stride bytes, CRC follows len bytes */
int dabx_crc16_check(const uint8_t *msgs, int stride, int len, int batch, uint8_t *ok);

/* fftwf_execute of the 2048-point forward/backward plan (base/main/dab_processor.cpp:63,201;
 * ofdm/phasereference.cpp:51-52): unnormalised DFT, batch x 2048 cf32. */
int dabx_fft2048(const dabx_cf32 *in, int batch, int inverse, dabx_cf32 *out);

/* OfdmDecoder (base/ofdm/ofdm_decoder.h:46-73) -- opaque per-stream demapper state on the device. */
typedef struct dabx_demap dabx_demap;
int dabx_demap_create(int batch, dabx_demap **out);
void dabx_demap_destroy(dabx_demap *d);
int dabx_demap_reset(dabx_demap *d);                                              /* reset()  :90-101  */
int dabx_demap_store_reference_symbol_0(dabx_demap *d, const dabx_cf32 *fft);     /* :132-145 batch x 2048 */
int dabx_demap_store_null_symbol_without_tii(dabx_demap *d, const dabx_cf32 *fft);/* :114-130 */
/* decode_symbol :147-355 for n_sym consecutive symbols: fft = batch x n_sym x 2048,
 * clock_err = batch floats, soft = batch x n_sym x 3072 int16. */
int dabx_demap_decode_symbols(dabx_demap *d, const dabx_cf32 *fft, int n_sym, const float *clock_err, int16_t *soft);
int dabx_demap_set_soft_bit_gen_type(dabx_demap *d, int type /*1..3*/);
/* SLcdData::SNR as decode_symbol computes it for the LCD statistics (:326-343 with _compute_noise_Power :358-371) from the
 * state as it stands: 10 log10((mMeanPowerOvrAll - noise) / noise); snr_db = batch floats. */
int dabx_demap_get_snr_db(dabx_demap *d, float *snr_db);
/* The device-side numbers of the LCD record (OfdmDecoder::SLcdData, ofdm_decoder.h:53-61; filled at ofdm_decoder.cpp:326-345) from the state
 * as it stands, batch floats each, any pointer may be NULL: SNR as above; MER = 10 log10((pi/4)^2 / mean over the carriers of
 * mStdDevSqPhaseVector) (:204-208, :331-340: the per-carrier IIR of the squared phase distance from the diagonal); mean_value = mMeanValue
 * (:294), which the record carries as TestData1. */
int dabx_demap_get_lcd_data(dabx_demap *d, float *snr_db, float *mer_db, float *mean_value);

/* PhaseReference::correlate_with_phase_ref_and_find_max_peak (base/ofdm/phasereference.cpp:87-213):
 * v = batch x 2048 cf32, returns start index per problem (or -1). */
int dabx_prs_correlate(const dabx_cf32 *v, int batch, float threshold, int strongest, int32_t *start_index);
/* PhaseReference::estimate_carrier_offset_from_sync_symbol_0 (:223-280): fft = batch x 2048 */
int dabx_coarse_cfo(const dabx_cf32 *fft_sym0, int batch, int32_t *hz);

/* FIB/FIG subset (host side, no device needed): sub-channel organisation FIG 0/1, service components FIG 0/2,
 * CIF counter FIG 0/0 -- base/decoder/fib_decoder.cpp:59-110, fib_decoder_fig0.cpp:89-101, 142-224, 230-293,
 * getters fib_decoder.cpp:547-557, 673-691.  fibs = n x 32 bytes as delivered by dabx_read_fibs / dabx_fic_decode.
 * Returns the number of sub-channels found (in order of first appearance, as FibDecoder::get_sub_channel_id_list
 * lists them); dab_plus = 1 / 0 / -1 (ASCTy 63 / other / unknown). */
struct dabx_subch_desc_s;
int dabx_parse_fibs(const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs, struct dabx_subch_desc_s *out, int max_out,
                    int32_t *cif_count);
/* The same as a running decoder (FibDecoder::process_FIB, fib_decoder.cpp:59-106, fed FIB by FIB in transmission order): it keeps
 * the CURRENT and the NEXT multiplex configuration -- FIG 0/1 and 0/2 are filed under _get_config_ptr(C/N flag),
 * fib_decoder.h:97, fib_decoder_fig0.cpp:149, 240 -- and swaps them when the change flags of FIG 0/0 go back to 0
 * (fib_decoder_fig0.cpp:102-111: std::swap(curr, next); next->reset(); see dabx_fibdec_set_reference_quirks for "from which value").  A sub-channel that reaches beyond the CIF or overlaps a
 * known one restarts the collection (fib_decoder.cpp:131-141), as in the reference. */
typedef struct dabx_fibdec dabx_fibdec;
typedef struct {
  int64_t fibs_processed;     /* FIBs handed to dabx_fibdec_process so far (those with a failed CRC are counted and skipped) */
  int64_t fig00_fib;          /* index, counted like fibs_processed, of the FIB that carried the newest FIG 0/0; -1: none yet */
  int64_t last_change_fib;    /* ... of the FIB whose FIG 0/0 made the newest swap; -1: none yet */
  int32_t cif_count;          /* newest FIG 0/0: CIFCountHi * 250 + CIFCountLo (mCifCount); -1: none yet */
  int32_t cif_count_hi, cif_count_lo;
  int32_t change_flags;       /* its ChangeFlags (EN 300 401 6.4.1: 0 none, 1 sub-channel, 2 service organisation, 3 both) */
  int32_t occurrence_change;  /* its OccurrenceChange: low byte (0..249) of the CIF count from which the next configuration applies;
                                 meaningful while change_flags != 0 */
  int32_t n_changes;          /* swaps so far */
  int32_t n_restarts;         /* _restart_fib_decoding calls so far */
  int32_t reserved[3];
} dabx_fibdec_info;
int  dabx_fibdec_create(dabx_fibdec **out);
void dabx_fibdec_destroy(dabx_fibdec *d);
int  dabx_fibdec_reset(dabx_fibdec *d);                              /* FibDecoder::connect_channel, fib_decoder.cpp:143-150 */
/* When the two configurations are swapped.  0 (default): whenever an announcement ends -- the change flags of FIG 0/0 go from ANY non-zero
 * value back to 0 (EN 300 401 6.4.1: 1 = sub-channel organisation, 2 = service organisation, 3 = both) -- and a table the announcement
 * never filled (no FIG 0/1 resp. 0/2 with C/N = 1 seen) is carried over from the current configuration.  1: the reference's rule, bit for
 * bit: only after flags 3 (fib_decoder_fig0.cpp:103); after flags 1 or 2 its next table is neither swapped nor reset, and the stale
 * entries take part in the reconfiguration after that. */
int  dabx_fibdec_set_reference_quirks(dabx_fibdec *d, int on);
/* n_fibs x 32 bytes + CRC flags (what dabx_read_fibs / dabx_fic_decode deliver); returns the number of swaps made in this call */
int  dabx_fibdec_process(dabx_fibdec *d, const uint8_t *fibs, const uint8_t *crc_ok, int n_fibs);
int  dabx_fibdec_get_info(const dabx_fibdec *d, dabx_fibdec_info *out);
/* sub-channel table of the current (next = 0) or the next (next = 1) configuration, like dabx_parse_fibs */
int  dabx_fibdec_subchannels(const dabx_fibdec *d, int next, struct dabx_subch_desc_s *out, int max_out);
/* Service components in packet mode (FIG 0/3, fib_decoder_fig0.cpp:294-330) of the current (next = 0) or the next configuration, in order of
 * first appearance; the first description of an SCId wins (:303-321).  What a host needs to bind a packet-mode sub-channel
 * (dabx_set_packet_mode): the sub-channel, the packet address, the data service component type and the DG flag (0 = data groups are used:
 * the one combination DataProcessor::add_to_frame does NOT walk as packets is dscty 5 with dg_flag 1, data_processor.cpp:111).  sid is the SId
 * of the FIG 0/2 service whose TMId-3 component names this SCId, as fib_decoder.cpp:362-411 joins the two; 0 while no such FIG 0/2 has been
 * seen.  Returns the number of components written. */
typedef struct {
  int32_t  scid;             /* 12 bits */
  int32_t  subch_id;
  int32_t  packet_address;   /* 10 bits */
  int32_t  dscty;
  int32_t  dg_flag;
  uint32_t sid;
} dabx_packet_component;
int  dabx_fibdec_packet_components(const dabx_fibdec *d, int next, dabx_packet_component *out, int max_out);

/* ===================================================================================== engine level
 * Stream-batched receiver: the device-side equivalent of DabProcessor::run
 * (base/main/dab_processor.cpp:110-442) for n_streams independent ensembles.                   */
typedef struct dabx_engine dabx_engine;

typedef struct {
  int32_t n_streams;        /* independent ensembles resident on this GPU */
  int32_t ring_frames;      /* IQ ring capacity per stream in units of T_F samples (>= 2) */
  int32_t max_subch;        /* sub-channels decoded per stream (<= 64) */
  int32_t out_frames;       /* output ring depth in frames (>= 1) */
  float   sync_threshold;   /* ProcessParams::threshold, main/dabradio.cpp:92 (3.0) */
  int32_t sync_strongest;   /* configuration.cpp:65 default 0 */
  int32_t soft_bit_type;    /* glob_enums.h:49-56, default 1 (SOFTDEC1) */
  int32_t fic_only;         /* 1: BASELINE config 2 (FIC Viterbi only) */
  int32_t capture_soft;     /* 1: keep int16 soft bits of the last frame (debug / parity tests) */
  int32_t viterbi_tie_mode; /* 0: canonical scalar Viterbi (CMake default); 1 / 2: arithmetic of the VITERBI_AVX2 / VITERBI_SSE2 builds,
                               see dabx_viterbi_mode */
  int32_t dc_iq_correction; /* SampleReader::set_dc_and_iq_correction (sample_reader.cpp:218-243, 334-346; configuration.cpp:75-76
                               default off): 0 off, 1 DC removal, 2 DC removal + IQ-imbalance correction, applied to every
                               committed sample in place in the ring (dabx_read_iq then returns corrected samples) */
  int32_t schedule;         /* 0 (default): overlapped -- the batched MSC decode and the demapping of a frame's MSC symbols run on
                               their own HIP streams next to the front end of the following frames; 1: serial -- every kernel on
                               ONE HIP stream in program order (debugging aid, deterministic per-kernel profiles; same bytes) */
  int32_t msc_fast_min_jobs;  /* trellises per 7-frame MSC batch (all streams together) from which the MSC runs on the
                                 lane-per-trellis kernels; below it the wave-per-trellis kernel decodes everything.  0 = default
                                 20480 (measured break-even, about 41 streams x 18 sub-channels) */
  int32_t msc_class_min_jobs; /* smallest protection-profile class (trellises per batch, all streams together) that gets its own
                                 lane-per-trellis class; smaller ones stay on the wave-per-trellis kernel.  0 = default 256 */
  int32_t exact_level_tracker;/* SampleReader's signal-level IIR (sample_reader.cpp:246-248).  Out of lock -- where the null-symbol
                                 search compares against it -- it is always the reference's recurrence, sample by sample.  In lock,
                                 where nothing reads it:
                                 0 (default): advanced chunk by chunk (relative error ~1e-5: what dabx_stats.signal_level shows in
                                   lock), and when a stream falls out of lock, walked exactly from the point and value at which the
                                   search had handed it over -- so the search continues from the reference's value, provided the
                                   samples read since then are still in the ring (pushes through dabx_push_iq* and the file
                                   readers are tracked; a zero-copy producer's are if it uses dabx_announce_write; a lock that outlasts
                                   the ring has lost them).  Then two walks are started a little below and above the chunk-wise
                                   value of the oldest frame boundary still in the ring; the recurrence forgets, and once they have
                                   merged into the same float (5 - 9 frames) that float is the exact value (level_healed_events).
                                   Failing that too, the level continues from the chunk-wise value: level_unanchored_events; the
                                   returns walked from the anchor itself are counted in level_rewalk_events;
                                 1: exact in lock too (a second pass over every sample on a HIP stream of its own: -27 % throughput
                                   at 512 streams, docs/history/r01-r04_design_notebook.md 6);
                                 2: chunk-wise only, the search continues from that value (the behaviour before round 4). */
  int32_t acquire_mode;       /* streams OUT of lock (null-symbol search + candidate correlations, k_acquire): 0 (default) -- searched on a HIP
                                 stream of their own next to the steps of the streams in lock, which never wait for them (a stream joins the
                                 first step after its search has finished); dabx_process(sync != 0) waits for the frames it issued, not for a
                                 search pass beside them.  While fewer than half of the streams are in lock -- start-up, a lone stream that
                                 lost its lock -- the search runs in step: every step first gives every such stream a frame's worth of
                                 search, exactly DabProcessor's order of events per stream.  1: always in step; 2: always asynchronous.
                                 While the device's count of streams in lock equals n_streams no search is launched at all (it would
                                 return at once for every stream): a stream that then loses its lock is searched from the first step ISSUED
                                 after the loss -- with sync = 0 the host may have queued steps ahead, which the stream sits out.
                                 Same samples, same decisions, same frames either way -- only WHEN differs.  (With dc_iq_correction the
                                 search always runs in step: the correction of newly committed samples is ordered on the front-end stream.) */
} dabx_config;

/* SDescriptorType subset (common/dab_constants.h:119-135) */
typedef struct dabx_subch_desc_s {
  int32_t subch_id, cu_start, cu_size, kbps, prot_level /* +4 => EEP-B */, short_form /* 1 = UEP */;
  int32_t dab_plus;          /* 1: run super-frame sync + RS(120,110) (Mp4Processor) */
  int32_t reserved;
} dabx_subch_desc;

typedef struct {
  int64_t frames;            /* frames demodulated since open */
  int64_t samples_consumed;
  int32_t state;             /* 0 wait-for-dip, 1 eval-sync, 2 in-frame */
  int32_t fic_ratio_percent; /* FicDecoder::get_fic_decode_ratio_percent */
  float   freq_offs_bb_hz, clock_err_hz;
  float   snr_db_est;        /* OfdmDecoder's LCD SNR (ofdm_decoder.cpp:326-343) after the newest frame's last symbol */
  int32_t last_start_index, cif_count;
  /* cif_count: CIFCountHi * 250 + CIFCountLo of the last FIG 0/0 in the last FIB with a good CRC that carries one (mCifCount); 0 before the
   * first.  The rule is the reference's walk (fib_decoder.cpp:74-100, fib_decoder_fig0.cpp:95-101): FIG after FIG by the header's length
   * field, stopped by the end marker alone, no length checked anywhere -- every FIG of type 0 with extension 0 sets the counter from the
   * bytes 4 and 5 behind its header, whatever its length field says (with the header at byte 25 or 26 those are the FIB's CRC bytes).  The
   * ETI frames of dabx_read_eti carry the same counter (one walk for both).  Three limits:
   *  - a FIG 0/0 header at byte 27 or later of the FIB is ignored (the reference reads bits of whatever follows the FIB in its buffer);
   *  - the reference's break after a FIG 0/1 with impossible content (mRestartFibDecoding) is not modelled: a FIG 0/0 behind it counts;
   *  - dabx_fibdec / dabx_parse_fibs walk more strictly (they stop at a FIG that runs past byte 30 and take a FIG 0/0 of length >= 5
   *    only): on a non-conformant FIB with a good CRC dabx_fibdec_info.cif_count can differ from this one. */
  int64_t fib_ok, fib_total, sf_ok, sf_fail, rs_corrected, rs_failed, au_ok, au_bad, cifs_decoded;
  float   signal_level;      /* SampleReader::sLevel (sample_reader.h:70,95; .cpp:245-248) after the newest frame */
  float   peak_level;        /* SampleReader::peakLevel (.cpp:247); tracked out of lock and, with exact_level_tracker, in lock */
  /* -- ABI 4 (everything above is the ABI-3 record) -- */
  int64_t level_margin_events; /* null-symbol search: comparisons level/50 <> 0.55 / 0.75 sLevel (timesyncer.cpp:58, 74) that fell within
                                1e-4 (relative) of their threshold, i.e. that the default (chunk-wise, ~1e-5) in-lock level tracker
                                could conceivably have decided differently from the sample-serial one; 0 = the approximation never mattered */
  int64_t level_rewalk_events;     /* losses of lock after which the level was re-walked exactly from its anchor (exact_level_tracker 0) */
  int64_t level_unanchored_events; /* ... after which it had to continue from the chunk-wise value (samples no longer in the ring) */
  int64_t level_healed_events;     /* ... after which the anchor was gone but two walks started 2^-9 either side of a frame boundary's
                                      chunk-wise value, four or more frames back in the ring, had merged into one float: exact all the same */
  /* -- ABI 5 -- */
  int64_t fic_ber_bits;      /* FicDecoder::mFicBits / mFicErrors (fic_decoder.h:74-75): transmitted FIC bits compared with the re-encoded */
  int64_t fic_ber_errors;    /* decoder output and those that differed (ViterbiSpiral::calculate_BER, viterbi_spiral.cpp:128-164), both halved
                                every 40 FIC blocks (fic_decoder.cpp:201-210); the channel BER the reference displays is errors / bits.
                                The hard decision is taken on the Viterbi symbol: with viterbi_tie_mode 0 a soft bit >= 32641 counts as
                                negative, because the scalar build's `soft + 127` wraps there (viterbi_scalar.h:34-40) */
  /* -- ABI 6 (in the place of the first reserved word: the record's size is unchanged) -- */
  float   mer_db_est;        /* OfdmDecoder's LCD MER (ofdm_decoder.cpp:204-208, 331-340) after the newest frame's last symbol; 0 unless
                                dabx_set_lcd_statistics switched its per-carrier IIR on */
  float   reserved_f;
  int64_t reserved[1];       /* zero; later fields go here without changing the record's size */
} dabx_stats;

void dabx_default_config(dabx_config *cfg);
int  dabx_create(const dabx_config *cfg, dabx_engine **out);
void dabx_destroy(dabx_engine *e);
/* The element of the IQ ring.  The reference's file devices turn the recording's codes into floats as they read them -- uint8 pairs
 * ((x - 127.38) / 128, raw_reader.cpp:66-70), int16 pairs (x / 32768, wav_reader.cpp:164) -- and SampleReader sees cf32 only; so does a
 * DABX_RING_CF32 engine (dabx_create), 8 bytes per sample.  A NATIVE ring keeps the codes themselves, 4 (S16) or 2 (U8) bytes per sample,
 * and the kernels that read the ring apply the same map at the load: both maps are exact in float, every decoded bit, every statistic
 * and dabx_read_iq are those of a cf32 engine fed the same codes.
 *   DABX_RING_S16  interleaved I, Q int16 in the machine's byte order, value (float)c / 32768
 *   DABX_RING_U8   interleaved I, Q uint8, value ((float)c - 127.38f) / 128.0f
 * What a native ring refuses (DABX_E_ARG, nothing written, dabx_last_error names the format and the ring):
 *   - dabx_push_iq / dabx_push_iq_async / dabx_ingest_open with a fmt other than the ring's (cf32 included): codes are copied, never
 *     converted;
 *   - file feeds and dabx_ingest_open_formats streams whose samples are not the ring's codes: any rate but 2.048 MS/s (the 1-ms
 *     interpolation produces floats), reference_quirks, int24 / int32 / float / int8 containers, int16 with Bits != 16, and in a U8
 *     ring the WAV family's uint8, whose map is (x - 128) / 128.  Accepted: RAW / UFF uint8 in a U8 ring; 16-bit int16 of either byte
 *     order and either I/Q order in an S16 ring (stored in machine order, I first);
 *   - dabx_config.dc_iq_correction != 0 at create: it rewrites samples in place and its output is not a code;
 *   - a ring of 4 GiB or more per stream (ring_frames > 5461 for S16).
 * The per-symbol handles (dabx_fic_*, dabx_msc_*) create cf32 engines. */
enum { DABX_RING_CF32 = 0, DABX_RING_S16 = 1, DABX_RING_U8 = 2 };   /* numbered like dabx_push_iq's fmt */
typedef struct {
  uint32_t size;            /* sizeof(dabx_create_ext) of the caller; fields beyond it take their defaults */
  int32_t  ring_format;     /* DABX_RING_* */
  int32_t  reserved[6];     /* zero */
} dabx_create_ext;
/* dabx_create with extensions (dabx_config and DABX_ABI_VERSION stay as they are).  ext == NULL: exactly dabx_create.  DABX_E_ARG: ext->size
 * smaller than the first two fields, an unknown ring_format, a native ring with dc_iq_correction. */
int  dabx_create_ex(const dabx_config *cfg, const dabx_create_ext *ext, dabx_engine **out);
/* The engine's ring element and its size: (0, 8), (1, 4) or (2, 2).  Either pointer may be NULL. */
int  dabx_get_ring_format(dabx_engine *e, int32_t *ring_format, int32_t *bytes_per_sample);
/* MscHandler::set_channel / stop_service equivalent for stream (or all streams when stream < 0): d[j] describes slot j
 * (kbps == 0: empty slot).  A slot whose description is unchanged keeps decoding without interruption, and so does one whose
 * sub-channel only moves to other capacity units (same SubChId, size, bit rate, protection: a multiplex reconfiguration; its
 * de-interleaver reads the CIFs before the change at the old address); new or otherwise changed
 * slots start their 16-CIF de-interleaver fill at the current CIF; a new largest bit rate re-strides the output rings in
 * place, running services are not disturbed.
 * Streams may carry different layouts: the decoder groups the slots of all streams by protection profile (rebuilt by the
 * next dabx_process after a series of calls).  At most DABX_MSC_FAST_CLASSES (16) profiles -- those with the most decoder
 * work, sub-channels x bit rate -- run on the lane-per-trellis kernels; every further profile, and classes smaller than
 * dabx_config.msc_class_min_jobs, are decoded by the wave-per-trellis kernel in the same batch.  That is a throughput
 * distinction only: there is NO limit on the number of different profiles per engine and no error code for exceeding 16
 * (tests/test_gpu_engine.py::test_more_profiles_than_decoder_classes runs 26). */
#define DABX_MSC_FAST_CLASSES 16
int  dabx_set_subchannels(dabx_engine *e, int stream, const dabx_subch_desc *d, int n);
/* Host IQ -> device ring (IDeviceHandler::getSamples contract, common/device_handler_if.h:47-48).
 * fmt: 0 = cf32, 1 = int16 IQ (/32768, wav_reader.cpp:164), 2 = uint8 IQ ((x-127.38)/128, raw_reader.cpp:66-70).
 * Returns when the caller's buffer is free again; copy and conversion run on their own HIP stream next to frames still
 * being decoded (the receiver is drained only if the ring looks full).
 * Native ring (dabx_create_ex): fmt must be the ring's format -- the codes are copied; any other fmt is DABX_E_ARG, nothing is written. */
int  dabx_push_iq(dabx_engine *e, int stream, const void *iq, int fmt, size_t n_samples);   /* DABX_E_STATE: would overwrite unread samples */
/* The same without waiting for the copy: the caller keeps `iq` alive and unchanged until dabx_push_wait returns.  Meant
 * for producers that cycle through a few page-locked buffers (hipHostMalloc, or their own memory passed once through
 * dabx_host_register): consecutive pushes then run back to back as DMA at PCIe rate next to the decode.  With pageable
 * memory the call behaves like dabx_push_iq. */
int  dabx_push_iq_async(dabx_engine *e, int stream, const void *iq, int fmt, size_t n_samples);
int  dabx_push_wait(dabx_engine *e);
int  dabx_host_register(void *p, size_t bytes);     /* hipHostRegister: page-lock a producer's buffer */
int  dabx_host_unregister(void *p);
/* Device-resident producers: ring base (capacity ring_frames*T_F SAMPLES) and commit of n new samples.  The ring is in the engine's own
 * element -- cf32 after dabx_create, int16 / uint8 pairs in a native ring: dabx_get_ring_format gives the bytes per sample. */
int  dabx_iq_ring_dev(dabx_engine *e, int stream, void **ring, size_t *capacity_samples);
int  dabx_commit_iq(dabx_engine *e, int stream /* <0: all */, size_t n_samples);
/* Optional, for device-resident producers that want the level tracker's anchor kept (dabx_config.exact_level_tracker = 0): the library
 * cannot see their writes, so after a plain dabx_commit_iq it must assume that anything behind the read cursor may have been
 * overwritten.  dabx_announce_write says, BEFORE the producer writes: "everything I have written so far, and everything I am going to
 * write until my next announcement, lies below committed + n_samples".  From its first announcement on the producer is taken at
 * its word (a commit no longer means "unknown writes"): announce before every write -- or once, with the ring's capacity, for a ring that
 * is filled once and only read again (periodic test signals). */
int  dabx_announce_write(dabx_engine *e, int stream /* <0: all */, size_t n_samples);
/* Host copy of ring samples [first, first + n) counted from the first sample ever committed (scopes, tests);
 * they must still be in the ring.  Always cf32: from a native ring, the values its codes stand for. */
int  dabx_read_iq(dabx_engine *e, int stream, uint64_t first, size_t n, float *iq_out);
/* Advance every stream by up to max_frames frames (bounded by available samples); returns the number of
 * batch steps executed.  Asynchronous on the engine's HIP stream unless sync != 0. */
int  dabx_process(dabx_engine *e, int max_frames, int sync);
int  dabx_synchronize(dabx_engine *e);
void *dabx_hip_stream(dabx_engine *e);
/* Results of the most recent frames (host copies). fibs: n x 12 x 32, crc: n x 12 */
int  dabx_read_fibs(dabx_engine *e, int stream, int n_frames, uint8_t *fibs, uint8_t *crc_ok);
/* Where the newest n_frames frames (n_frames <= out_frames, oldest first, the frames dabx_read_fibs returns) sit in the stream's
 * sample sequence: sym0_pos = index, counted from the first sample ever committed, of the first sample of the useful part of the
 * frame's phase reference symbol; start_index = the PRS correlation peak that placed it (DabProcessor's startIndex,
 * dab_processor.cpp:394-411).  Either array may be NULL.  Returns the number of frames written.  Time-stamps frames for a host
 * that knows when it committed which samples; lets a test compare the receiver's walk through the samples frame by frame. */
int  dabx_read_frame_info(dabx_engine *e, int stream, int n_frames, int64_t *sym0_pos, int32_t *start_index);
/* Sub-channel table announced in the FIBs of the newest frames of `stream` (dabx_parse_fibs over the FIB ring);
 * feed the result to dabx_set_subchannels to decode "everything found in the FIC" like EtiGenerator does. */
int  dabx_discover_subchannels(dabx_engine *e, int stream, dabx_subch_desc *out, int max_out);
/* Multiplex reconfiguration (EN 300 401 6.4.1, 6.5; FibDecoder's current / next tables).  The engine keeps one dabx_fibdec per
 * stream; dabx_follow_fic feeds it the FIBs of the frames decoded since the last call (in order; frames that have already left
 * the FIB ring of out_frames frames are reported in frames_missed) and says where the stream stands:
 *   pending      the newest FIG 0/0 carries change flags != 0: a reconfiguration is announced;
 *   at_cif       ... and takes effect from this CIF on, counted like the engine counts CIFs (4 per frame from the first frame
 *                decoded: CIF 4 f + k is the k-th of frame f) -- the CIF whose counter's low byte equals OccurrenceChange, at or
 *                after the CIF that carried the announcement;
 *   n_changes / last_change_cif   swaps the decoder has made (change flags 3 -> 0) and the engine CIF of the FIB group that made the
 *                newest one, i.e. the first CIF of the new configuration as the reference sees it.
 * dabx_next_subchannels returns the announced (next) table.  To follow a reconfiguration: call dabx_process up to the frame that
 * holds at_cif (frames = at_cif / 4 - frames decoded), then dabx_set_subchannels_at(..., at_cif) with the table wanted from then
 * on, and go on -- slots whose description does not change keep running, new ones start their 16-CIF de-interleaver fill at at_cif,
 * slots that end stop with the call: their last logical frame is that of the last CIF of the frame decoded before it, also when
 * at_cif lies inside the coming frame (tests/test_gpu_reconfig.py, cif_in_frame = 2). */
typedef struct {
  int32_t pending, n_changes, frames_missed, reserved;
  int64_t at_cif, last_change_cif, frames_fed;
} dabx_reconf;
int  dabx_follow_fic(dabx_engine *e, int stream, dabx_reconf *out);
/* The FIB decoders behind dabx_follow_fic / dabx_next_subchannels / dabx_current_subchannels swap their tables after ANY announcement by
 * default; on != 0 makes them (those that exist and those created later) follow the reference's rule to the bit -- only after change flags 3
 * (fib_decoder_fig0.cpp:103), dabx_fibdec_set_reference_quirks -- so that an engine-level reconfiguration can be compared with the reference's
 * own behaviour for flags 1 and 2 as well. */
int  dabx_set_fig_reference_quirks(dabx_engine *e, int on);
/* OfdmDecoder's LCD record (SLcdData, ofdm_decoder.h:53-61) carries, next to the SNR the engine always estimates (dabx_stats.snr_db_est), the MER:
 * 10 log10((pi/4)^2 / mean_k mStdDevSqPhaseVector[k]), a per-carrier IIR of the squared phase distance from the constellation's diagonal
 * (ofdm_decoder.cpp:204-208, 331-340) that feeds no soft bit.  on != 0 advances that IIR in the demapper too (a few instructions per carrier and
 * symbol; off by default: a display statistic of one receiver, not of 512) and dabx_stats.mer_db_est / dabx_chunk_stream.mer_db_est report it
 * after every frame; switched on in mid-stream the IIR starts from what it last held (zero after a reset / loss of lock, like the reference's).
 * Drains the engine. */
int  dabx_set_lcd_statistics(dabx_engine *e, int on);
int  dabx_next_subchannels(dabx_engine *e, int stream, dabx_subch_desc *out, int max_out);
/* ... and the CURRENT table of the same decoder (after a swap: the former next table plus whatever the new configuration's own FIGs,
 * C/N = 0, have added since -- first description wins). */
int  dabx_current_subchannels(dabx_engine *e, int stream, dabx_subch_desc *out, int max_out);
/* dabx_set_subchannels whose new and changed slots start at CIF at_cif instead of at the next CIF to be demodulated:
 * next CIF <= at_cif <= next CIF + 3 (a reconfiguration inside the coming frame).  stream >= 0. */
int  dabx_set_subchannels_at(dabx_engine *e, int stream, const dabx_subch_desc *d, int n, int64_t at_cif);
/* Decoded logical frames of a sub-channel: n_cifs x 3*kbps bytes, newest last; returns #CIFs valid. */
int  dabx_read_msc(dabx_engine *e, int stream, int subch_idx, int n_cifs, uint8_t *bytes);
/* RS-corrected DAB+ super frames (110*kbps/8 bytes each), newest last; returns count copied. */
int  dabx_read_superframes(dabx_engine *e, int stream, int subch_idx, int n, uint8_t *bytes);
/* What Mp4Processor::_process_super_frame (base/backend/audio/mp4processor.cpp:249-333) knows about a super frame when it hands the
 * access units to the AAC decoder: the stream parameters (:258-262), numAUs and mAuStartArr (:272-304), the verdict of the length check
 * (:311) and of check_crc_bytes (:321) for every access unit, and what the RS decoder / the fire code corrected on the way
 * (:184-241).  One record per super frame in the super-frame ring, written by the device stage that ran all of it (k_dabplus): a host
 * that feeds an AAC decoder slices the super frame at au_start[] and looks at the masks -- it re-parses no header and re-runs no CRC:
 *     for (a = 0; a < r.num_aus; a++)
 *       if (r.au_crc_ok >> a & 1) decoder.decode(sf + r.au_start[a], r.au_start[a + 1] - r.au_start[a] - 2);   // the 2 CRC bytes excluded, :306
 *       else                      decoder.conceal();                                                         // :316, :339
 * 32 bytes, little-endian, no padding holes. */
typedef struct dabx_superframe_info_s {
  uint8_t  num_aus;        /* 2, 3, 4 or 6 */
  uint8_t  au_crc_ok;      /* bit a: access unit a passed its CRC */
  uint8_t  au_len_bad;     /* bit a: access unit a failed the length check (aacFrameLen > 960, < 0, or beyond the super frame); no CRC run */
  uint8_t  stream_parms;   /* mOutVec[2] & 0x7F: dacRate 0x40, sbrFlag 0x20, aacChannelMode 0x10, psFlag 0x08, mpegSurround 0x07 */
  uint16_t au_start[7];    /* mAuStartArr[0 .. num_aus]; au_start[num_aus] = 110 * kbps / 8 */
  uint16_t rs_corrected;   /* byte corrections of the RS decoder in this super frame (sum of its returns >= 0) */
  uint8_t  rs_failed;      /* code words the RS decoder gave up on (the fire code passed all the same) */
  uint8_t  fc_corrected;   /* 1: check_and_correct_6bits changed the 11-byte header (mSumFcCorrections) */
  uint16_t reserved;
  int64_t  first_frame;    /* index, in the slot's sequence of logical frames, of the first of the super frame's five */
} dabx_superframe_info;
/* the records of the newest n super frames, oldest first: row i describes row i of dabx_read_superframes(..., n, ...) */
int  dabx_read_superframe_info(dabx_engine *e, int stream, int subch_idx, int n, dabx_superframe_info *out);
int  dabx_read_soft(dabx_engine *e, int stream, int16_t *soft /* 75*3072 */);
/* dabx_get_stats_sized fills the first `size` bytes of a dabx_stats.  dabx_get_stats is that call with the caller's own
 * sizeof -- as a macro, so that a binary and the library never disagree about how much is written; the exported function of the
 * same name is what binaries built against ABI 3 call and writes the ABI-3 record only.  Hosts that load the library at run time
 * compare dabx_abi_version() with the DABX_ABI_VERSION they were built against (shim/dabx_shim_env.h does). */
int  dabx_get_stats_sized(dabx_engine *e, int stream, void *out, size_t size);
int  dabx_get_stats(dabx_engine *e, int stream, dabx_stats *out);
#define dabx_get_stats(e, stream, out) dabx_get_stats_sized((e), (stream), (out), sizeof(*(out)))
/* Per-slot counters (Backend / Mp4Processor members: backend.cpp:146-150 warm-up, mp4processor.h:106-112 signals). */
typedef struct dabx_subch_stats_s {
  int64_t start_cif;         /* CIF index (since open) at which the slot was configured */
  int64_t cifs_decoded;      /* logical frames produced so far; frame i belongs to CIF start_cif + 16 + i */
  int64_t sf_count;          /* super frames written to the super-frame ring */
  int64_t sf_ok, sf_fail, rs_corrected, rs_failed, fc_corrected, au_ok, au_bad;
  int32_t active, subch_id;
} dabx_subch_stats;
int  dabx_get_subch_stats(dabx_engine *e, int stream, int subch_idx, dabx_subch_stats *out);
/* Sum of the counters over all streams of this engine (the values one RCCL all-reduce combines). */
int  dabx_get_counters(dabx_engine *e, int64_t out[16]);
/* ------------------------------------------------------------------------------------------------------------
 * Packet-mode data sub-channels: DataProcessor (base/backend/data/data_processor.cpp:106-254), the third FrameProcessor of the
 * reference's back end, on the device (k_packet, behind the MSC decoder of every batch, one wave per packet-mode slot).  For every
 * logical frame of the slot, in order: the packet walk (:123-150: packet length (bits 0..1 + 1) * 24 bytes, stop when fewer bytes remain),
 * per packet the address filter, the continuity index -- a mismatch sets the expected index to 0 and drops the packet (:170-178); the
 * expected index advances before the CRC is looked at (:181) --, check_CRC_bits over the whole packet (:184), and the assembly of the MSC
 * data groups from first / intermediate / last / single packets (:191-253; a single packet inside a series abandons the series and is
 * NOT emitted, :248-252).  The payload of a packet is its `useful length` bytes from byte 3; groups are kept as packed bytes.
 * Two guards, where the reference is undefined or unbounded:
 *   - useful length > packet length - 5: the reference copies `useful length` bytes from byte 3 whatever follows (:199, :224).  While those
 *     bytes lie inside the logical frame the device does the same; when they would pass the end of the logical frame (the reference reads
 *     out of bounds) the packet is dropped like one with a failed CRC, the assembly state unchanged, and counted in len_bad;
 *   - a series is bounded at DABX_DG_MAX_BYTES (the largest legal MSC data group is below 8.3 KB; the reference's mSeriesVec grows without
 *     limit): an append that would exceed it abandons the series (back to "waiting for a start") and is counted in dg_overflow.
 * Every completed group goes, bytes and one dabx_datagroup_info record, into per-slot rings sized from the bit rate (two full batches, 56
 * logical frames, of single-packet groups fit); the assembly state lives on the device and survives batch boundaries.  A host hands
 * bytes[byte_pos .. byte_pos + length) to its data handler and looks at crc_ok: it walks no packet and runs no CRC.
 * Out of scope: packet-mode FEC (EN 300 401 5.3.5), the TDC asynchronous stream (:257-278), the data handlers themselves. */
#define DABX_DG_MAX_BYTES 16384
typedef struct {
  uint32_t size;             /* sizeof(dabx_packet_config) of the caller */
  int32_t  packet_address;   /* 0 .. 1023: DataProcessor::mPacketAddress (FIG 0/3, dabx_packet_component.packet_address) */
  int32_t  reserved[6];      /* zero */
} dabx_packet_config;
typedef struct dabx_datagroup_info_s {
  int64_t  byte_pos;         /* position of the group's first byte in the slot's sequence of data-group bytes */
  int64_t  first_frame;      /* logical-frame index, as in dabx_superframe_info, of the packet that started the group */
  int64_t  last_frame;       /* ... of the packet that completed it */
  uint16_t length;           /* bytes */
  uint8_t  crc_flag;         /* bit 6 of byte 0 of the group: a data-group CRC is present (what ip_datahandler.cpp:48 reads); 0 for an empty group */
  uint8_t  crc_ok;           /* crc_flag set, length >= 2 and the CCITT check over the whole group passed (ip_datahandler.cpp:59); 0 otherwise */
  uint32_t reserved;
} dabx_datagroup_info;       /* 32 bytes, little-endian, no holes */
typedef struct {
  int64_t frames;            /* logical frames walked */
  int64_t packets;           /* packets the walk handed on (_handle_packet calls) */
  int64_t addr_match;        /* ... whose address was the slot's */
  int64_t continuity_err;    /* ... dropped for their continuity index */
  int64_t crc_bad;           /* ... dropped for their CRC */
  int64_t len_bad;           /* ... dropped because their useful length reaches beyond the logical frame (guard) */
  int64_t walk_short;        /* frames whose walk ended at a length code that overruns the frame (:129-133) */
  int64_t dg_count;          /* groups completed */
  int64_t dg_bytes;          /* ... and their bytes */
  int64_t dg_crc_bad;        /* ... of them, with the CRC flag set and crc_ok == 0 */
  int64_t dg_overflow;       /* series abandoned at DABX_DG_MAX_BYTES (guard) */
  int64_t dg_lost;           /* groups that had left the rings before a dabx_read_datagroups call could return them */
  int32_t active;            /* 1: the slot is in packet mode (all else is zero otherwise) */
  int32_t packet_address;
  int64_t reserved[3];
} dabx_packet_stats;         /* 128 bytes */
/* Switches slot subch_idx of `stream` to packet mode (cfg != NULL) or back to plain logical frames (NULL).  Only an active slot with
 * dab_plus == 0 and a bit rate that is a multiple of 8 up to 384 kbit/s; DABX_E_ARG otherwise.  The slot's logical frames are produced and
 * delivered exactly as before; the walk starts with the next logical frame decoded.  Calling it again for a slot in packet mode restarts
 * the assembly with the new address and empty rings.  The setting and the assembly state stay with the slot wherever dabx_set_subchannels
 * says it "keeps decoding without interruption", a move to other capacity units included; a new or changed slot loses them.  An engine
 * without a packet-mode slot allocates and launches nothing for this stage.  Drains the engine. */
int  dabx_set_packet_mode(dabx_engine *e, int stream, int subch_idx, const dabx_packet_config *cfg);
/* The newest n completed groups still in the rings, oldest first: their records into info[], their bytes back to back into bytes[];
 * byte_pos is rebased to the returned buffer (info[0].byte_pos == 0).  When the bytes of n groups exceed max_bytes the newest groups that
 * fit are returned (bytes == NULL: records only, byte_pos rebased all the same).  Returns the number of groups.  Groups older than
 * the ones returned count as seen; groups that left the rings unseen are counted in dabx_packet_stats.dg_lost.  Drains the engine like
 * the other dabx_read_* calls. */
int  dabx_read_datagroups(dabx_engine *e, int stream, int subch_idx, int n, dabx_datagroup_info *info, uint8_t *bytes, size_t max_bytes);
int  dabx_get_packet_stats(dabx_engine *e, int stream, int subch_idx, dabx_packet_stats *out);
/* ------------------------------------------------------------------------------------------------------------
 * Programme-associated data of DAB+ access units: the one piece of Mp4Processor::_process_super_frame that is neither audio decoding nor
 * GUI, on the device (k_pad, behind k_dabplus on the MSC batch's stream, one wave per PAD-enabled slot).  For every access unit of an
 * accepted super frame that passed its CRC (au_crc_ok set, au_len_bad clear), in AU order, super frames in order
 * (base/backend/audio/mp4processor.cpp:320-353): when its first syntactic element is a data stream element (id 4, :345), count = AU[1],
 * the PAD is AU[2 .. 2 + count), its last two bytes are the F-PAD (:347-352) and the rest the X-PAD, stored reversed, which goes through
 * PadHandler::process_PAD (base/backend/data/pad_handler.cpp:67-97): F-PAD type and X-PAD indicator dispatch, the short X-PAD with and
 * without contents indicator (:111-200), the variable X-PAD with and without (:208-330; mXPadLength counts the CI bytes and the end
 * marker too, :268-273, and that is how long a no-CI continuation is taken to be, :224), the dynamic label (:335-455), the data-group
 * length indicator with its CRC (:291-300) and the assembly of the X-PAD MSC data groups (:460-519).  Two hand-over points:
 *   - every `emit signal_show_label` (:144, :193, :416, :452) is one DABX_PAD_LABEL item: the bytes of mDynamicLabelTextUnConverted at that
 *     moment and mCharSet; the conversion to_QString_using_charset stays with the host;
 *   - every _build_MSC_segment call (:478, :514) with size = min(iData.size(), mDataGroupLength) >= 2 (:528-534) is one DABX_PAD_DATAGROUP
 *     item: iData[0 .. size), crc_flag = bit 6 of byte 0 (the CrcFlag bit-field, :524, :539), crc_ok = check_crc_bytes(iData, size - 2)
 *     (:541).  A group with a bad CRC is delivered with crc_ok == 0 and counted (the reference drops it, :543); the MOT parsing from :553 on
 *     is the host's, or k_mot's ("MOT objects of the X-PAD" below).
 * The state in between (pad_handler.h:68-86) lives on the device per slot and survives batch boundaries.  Four guards, where the
 * reference is undefined or unbounded; each is counted:
 *   G1 (mp4processor.cpp:347-352): the reference reads AU[2 .. 2 + count), buffer[count - 1] and buffer[count - 2] whatever they are.
 *      count < 2, or a byte it reads beyond the end of the super frame (au_start[a] + 2 + count > 110 * kbps / 8, or au_start[a] + 2 itself
 *      beyond it): the AU's PAD is skipped, state unchanged, counted in pad_bad.  Bytes inside the super frame but beyond the AU are read
 *      as the reference reads them.
 *   G2 (pad_handler.cpp:119-122, :151): a short X-PAD (X-PAD indicator 1) with fewer than 4 X-PAD bytes (iLast < 3) indexes below 0:
 *      skipped, state unchanged, pad_bad.
 *   G3 (:254-262, :284-287): a variable X-PAD whose CI list (up to four bytes, ending early at application type 0) would be read below
 *      index 0 is skipped before any state is touched, pad_bad.  A sub-field whose `length` bytes would reach below index 0 stops the walk
 *      in front of that sub-field: mXPadLength is set as the reference sets it, mLastAppType is as the previous sub-field left it, pad_bad.
 *      (The no-CI form has the reference's own check, :219.)
 *   G4 (:163, :183; applied to every append, :407 and :446 too): mDynamicLabelTextUnConverted is bounded at DABX_DL_MAX_BYTES (the legal
 *      maximum is 8 segments of 16 bytes): an append that would exceed it is dropped whole, text unchanged, counted in dl_overflow.
 * The data-group buffer needs no guard: mMscDataGroupBuffer is handed on as soon as it reaches mDataGroupLength <= 16 383 (:512), so it
 * never holds more than 16 382 bytes plus one sub-field (at most 196 bytes, a no-CI continuation of mXPadLength bytes).
 *
 * PAD of DAB (MP2) audio frames (source DABX_PAD_SOURCE_MP2): for a classic DAB audio sub-channel the same PadHandler is fed by the one
 * piece of Mp2Processor that is neither audio decoding nor GUI (base/backend/audio/mp2processor.cpp:611-747 with :250-285), on the device
 * (k_pad_mp2, beside k_pad on the MSC batch's stream, one wave per such slot).  Mp2Processor::add_to_frame (:678-747) runs over the bits of
 * every logical frame (24 * kbps of them, MP2framesize): SearchingForSync counts ones until the 12th (:715-733; the run may straddle a
 * logical-frame boundary), GetSampleRate collects 12 more header bits (:735-744; they may straddle one too), GetData counts bits until
 * MP2bitCount reaches lf = MP2framesize at 48 kHz, twice that at 24 kHz (:680, :741), and then searches again.  Quirks kept:
 *   - the header check (:277-279) evaluates (iFrame[2] - 0x10) >= 0xE0 in int: only bit-rate index 15 is refused, index 0 passes; a
 *     refused header and the rates 44 100, 32 000, 22 050, 16 000 and 0 leave sampleRate as it was (:257-261; it starts at 48 000);
 *   - when an MP2 frame completes (:691), _process_pad_data takes the PAD from the end of the CURRENT logical frame, wherever in it the MP2
 *     frame ended (:695); at 24 kHz that is every second logical frame.
 * _process_pad_data (:611-674): vLen = 3 * kbps - (kbps >= 56 ? 4 : 2) - 2 bytes in front of the ScF-CRC and the F-PAD; L0 is the logical
 * frame's last byte, L1 the one in front of it; F-PAD type != 0 and X-PAD indicator 0 and 3 return (counted as for DAB+); indicator 1 hands
 * on the four bytes frame[vLen - 4 .. vLen) with iLast = 3, indicator 2 frame[0 .. vLen) with iLast = vLen - 1.  The device stages the
 * newest min(vLen, 254) of them: PadHandler reads at most 196 bytes below iLast (four contents indicators, sub-fields of together at
 * most 4 * 48 bytes, or a no-CI continuation of mXPadLength <= 196 bytes), so no decision changes.  Guards G1 and G2 have no counterpart
 * (vLen >= 20 and the short form always has its four bytes); G3 and the check of :219 do bite at small rates, G4 is as above.
 * Parity of this path with the reference is unpinned: mp2processor.cpp cannot be compiled without the GUI's headers, so the tests compare
 * the device with a line-by-line restatement (tests/mp2_pad_cases.py), not with the reference's object code.
 * Out of scope: MotHandler of the X-PAD (the handler's one MotObject is "MOT objects of the X-PAD" below; the packet-mode MotHandler is
 * "MOT objects of a packet-mode carousel"), the charset conversion, DL Plus, F-PAD types
 * other than 0, handing out assembled MP2 frames.  (MP2 audio decoding is "MP2 audio" at the end of this file.) */
#define DABX_DL_MAX_BYTES 256
enum { DABX_PAD_LABEL = 1, DABX_PAD_DATAGROUP = 2 };
enum { DABX_PAD_SOURCE_DABPLUS = 0,    /* the access units of a DAB+ slot (dab_plus == 1) */
       DABX_PAD_SOURCE_MP2 = 1 };      /* the MP2 frames of a DAB audio slot (dab_plus == 0, not in packet mode, a multiple of 8 kbit/s up to 384) */
typedef struct {
  uint32_t size;             /* sizeof(dabx_pad_config) of the caller */
  int32_t  source;           /* DABX_PAD_SOURCE_*; read only when size >= 8 (a shorter configuration means DABX_PAD_SOURCE_DABPLUS) */
  int32_t  reserved[6];      /* zero */
} dabx_pad_config;
typedef struct dabx_pad_item_s {
  int64_t  byte_pos;         /* position of the item's first byte in the slot's sequence of item bytes */
  int64_t  frame;            /* dabx_superframe_info.first_frame of the super frame whose access unit completed the item; MP2 source: the
                                index of the logical frame that supplied the PAD, in the numbering of dabx_datagroup_info.last_frame */
  uint16_t length;           /* bytes */
  uint8_t  kind;             /* DABX_PAD_LABEL or DABX_PAD_DATAGROUP */
  uint8_t  au;               /* ... and that access unit's index in the super frame (MP2 source: 0) */
  uint8_t  charset;          /* labels: mCharSet (pad_handler.cpp:122, :353) */
  uint8_t  crc_flag;         /* groups: bit 6 of byte 0 (:539) */
  uint8_t  crc_ok;           /* groups: check_crc_bytes(iData, length - 2) (:541) */
  uint8_t  reserved[9];
} dabx_pad_item;             /* 32 bytes, little-endian, no holes */
typedef struct {
  int64_t superframes;       /* super frames walked (MP2 source: logical frames walked) */
  int64_t aus;               /* access units taken (au_crc_ok set, au_len_bad clear) (MP2 source: _process_pad_data calls, as pad_aus) */
  int64_t pad_aus;           /* ... that start with a data stream element (id 4, mp4processor.cpp:345) */
  int64_t fpad_other;        /* ... whose F-PAD type is not 0 (pad_handler.cpp:71) */
  int64_t xpad_short, xpad_variable, xpad_other;      /* X-PAD indicator 1 / 2 / 0 or 3 (:81-96), counted in front of the guards */
  int64_t pad_bad;           /* guards G1, G2, G3 */
  int64_t labels, label_bytes;      /* DABX_PAD_LABEL items and their bytes */
  int64_t groups, group_bytes;      /* DABX_PAD_DATAGROUP items and their bytes */
  int64_t items_lost;        /* items that had left the rings before a dabx_read_pad_items call could return them */
  int32_t li_bad;            /* data-group length indicators refused: CRC, or a length other than 4 (:292-299) */
  int32_t dl_overflow;       /* guard G4 */
  int32_t dg_crc_bad;        /* groups with crc_flag set and crc_ok == 0 */
  int32_t dg_small;          /* _build_MSC_segment calls with size < 2 (:530) */
  int32_t active;            /* 1: PAD decoding is on for the slot (all else is zero otherwise) */
  int32_t reserved;
} dabx_pad_stats;            /* 128 bytes */
/* Switches PAD decoding of slot subch_idx of `stream` on (cfg != NULL) or off (NULL).  Source DABX_PAD_SOURCE_DABPLUS: only an active
 * slot with dab_plus == 1; source DABX_PAD_SOURCE_MP2: only an active slot with dab_plus == 0 that is not in packet mode; DABX_E_ARG
 * otherwise, and for an unknown source.  NULL: a slot whose PAD decoding is on, or a DAB+ slot.  The slot's logical frames, super frames and records are produced and delivered exactly as before; the walk starts with the
 * next super frame completed.  Calling it again for a PAD slot restarts the state with empty rings.  The setting and the state stay with
 * the slot wherever dabx_set_subchannels says it "keeps decoding without interruption", a move to other capacity units included; a new or
 * changed slot loses them.  An engine without a PAD slot allocates and launches nothing for this stage.  Drains the engine. */
int  dabx_set_pad_mode(dabx_engine *e, int stream, int subch_idx, const dabx_pad_config *cfg);
/* The newest n items still in the rings, oldest first, labels and groups in emission order: their records into info[], their bytes back
 * to back into bytes[]; byte_pos is rebased to the returned buffer (info[0].byte_pos == 0).  When the bytes of n items exceed max_bytes
 * the newest items that fit are returned (bytes == NULL: records only).  Returns the number of items.  Items older than the ones returned
 * count as seen; items that left the rings unseen are counted in dabx_pad_stats.items_lost.  The rings hold what two full batches can
 * emit (512 items, 128 KiB; pad_core.h has the derivation).  Drains the engine like the other dabx_read_* calls. */
int  dabx_read_pad_items(dabx_engine *e, int stream, int subch_idx, int n, dabx_pad_item *info, uint8_t *bytes, size_t max_bytes);
int  dabx_get_pad_stats(dabx_engine *e, int stream, int subch_idx, dabx_pad_stats *out);
/* Where Mp2Processor's frame sync of a PAD slot with source DABX_PAD_SOURCE_MP2 stands: a host MP2 decoder learns from it where the MP2
 * frames start in the logical frames it reads.  All zero for any other slot.  Drains the engine. */
typedef struct {
  int64_t syncs;             /* sync words found: 12 ones in a row (mp2processor.cpp:720) */
  int64_t frames;            /* MP2 frames completed (:691) = _process_pad_data calls */
  int64_t hdr_refused;       /* headers _get_mp2_sample_rate refused (:277-279): ID / layer bits, or bit-rate index 15 */
  int64_t rate_unsupported;  /* headers that passed with a rate _set_sample_rate refuses (:257-261): 44 100, 32 000, 22 050, 16 000, 0 */
  int32_t sample_rate;       /* sampleRate: 48 000 or 24 000 */
  int32_t state;             /* MP2SyncState: 0 SearchingForSync, 1 GetSampleRate, 2 GetData */
  int32_t bit_count;         /* MP2bitCount */
  int32_t header_count;      /* MP2headerCount */
  int32_t last_sync_bit;     /* bit index in its logical frame of the 12th one of the last sync word (the MP2 frame starts 11 bits in
                                front of it); -1: none yet */
  int32_t active;            /* 1: the slot is a PAD slot with source DABX_PAD_SOURCE_MP2 (all else is zero otherwise) */
  int32_t reserved[2];
} dabx_mp2_sync_stats;       /* 64 bytes */
int  dabx_get_mp2_sync_stats(dabx_engine *e, int stream, int subch_idx, dabx_mp2_sync_stats *out);
/* ------------------------------------------------------------------------------------------------------------
 * MOT objects of the X-PAD: what PadHandler does with a data group behind the hand-over of dabx_pad_item -- the tail of
 * _build_MSC_segment (base/backend/data/pad_handler.cpp:539-622) and the handler's one MotObject (pad_handler.cpp:54: no directory
 * element, a PAD element; base/backend/data/mot/mot_object.cpp:71-323) -- on the device (k_mot, behind k_pad / k_pad_mp2 on the MSC
 * batch's stream, one wave per MOT-enabled PAD slot, for both PAD sources).  Every `emit signal_new_mot_object` (:300) is one
 * dabx_mot_object plus its bytes: the finished slideshow picture with its name and content type.  Per DABX_PAD_DATAGROUP item, in emission
 * order; the item's `length` is the reference's `size` (:528):
 *   1 crc_flag && !crc_ok: return (:539-545, crc_bad).  No flag: go on (:548-551).
 *   2 DataGroupType (byte 0, bits 0-3) other than 3 / 4: return (:556-560, type_other).
 *   3 index = ExtensionFlag (bit 7) ? 4 : 2.  SegmentFlag (bit 5): lastFlag and the 15-bit segment number, index += 2 (:567-573); without it
 *     the number is -1.  UserAccessFlag (bit 4): lengthIndicator = low nibble, the transport id from the two bytes behind the length byte
 *     whenever bit 4 of that byte is set, WHATEVER lengthIndicator says (:583-588); index moves by 1 + lengthIndicator only (:589).  No
 *     transport id: return (:593-597, no_tid).
 *   4 segmentSize = 13 bits at index, the segment starts at index + 2 (:605-616).
 *   5 type 3, set_header (mot_object.cpp:71-115): a transport-id change resets the object first (:75-79, resets); the 7-byte header core
 *     (:84-95); the extension walk `while pointer < headerSize` (:99-104, :210-238): PLI 0 / 1 / 2 advance by 1 / 2 / 5, PLI 3 has the 7- or
 *     15-bit length.  ContentName (0x0C) replaces the name with bytes [pointer + 1, pointer + length) (:181-189).  Parameters 0x02-0x08,
 *     0x0A, 0x0B and 0x0F do NOT advance the pointer by their length (:191-201): the bytes of their value are walked as parameters.  Kept.
 *     Then _check_if_complete and the emit (:111-114).
 *   6 type 4, add_body_segment (:117-175): a number < 0 or >= 8192: return (:119-123, seg_number_bad); a transport-id change resets the
 *     object, header core included (:125-130); a number already stored: return (:139-143, seg_duplicate); else the segment is stored and
 *     the sum grows; a last flag sets mNumOfSegments = number + 1, a later one overwrites it (:145-148); signal_pad_mot_progress for base
 *     type image with bodySize > 0, clamped at 100 (:160-169: progress_pct, progress_events); _check_if_complete (:240-278: header core
 *     seen, number of segments known, stored count >= that number, every index below it present) and the emit (:281-301): ALL stored
 *     segments in key order, those numbered at or above mNumOfSegments too.
 *   7 Nothing is cleared after an emit; only a transport-id change resets (:313-323).  Every repeated header of a complete object
 *     therefore emits it again (:111-114): `repeat` counts that.
 * Three guards, where the reference reads outside the bytes it was given or grows without bound; each is counted:
 *   M1 (pad_handler.cpp:569-616): a header field, the segmentation header or the segment itself (index + 2 + segmentSize) would reach
 *      beyond the item's `length` bytes: the group is ignored, state unchanged, grp_short.  Bytes inside the item, the two CRC bytes
 *      included, are read as the reference reads them.  The reference's buffer can be longer than `size` (mMscDataGroupBuffer beyond
 *      mDataGroupLength, :528), where its reads are defined; the item does not carry those bytes, so the guard covers that case too.
 *   M2 (mot_object.cpp:84-87, :212-230, :185): a type-3 segment shorter than the 7 bytes of the header core is ignored, state unchanged.  An
 *      extension read -- the parameter byte, its length bytes, a name byte -- at an index >= segmentSize ends the walk: that parameter is
 *      not applied and the completeness check follows.  A header longer than its segment (a segmented header) ends there too.  hdr_bad.
 *   M3 (:135-137): a body segment that would take the stored sum beyond max_object_bytes resets the object; the transport id just set
 *      stays.  obj_overflow.  (The reference's map grows without limit.)
 * The name needs no guard: it lies inside a header segment, fewer than 8192 bytes.
 * Parity of this path with the reference's object code is unpinned: mot_object.cpp cannot be compiled without the GUI's headers
 * (dabradio.h), so the tests compare the device with a line-by-line restatement (tests/mot_cases.py).
 * Out of scope: image decoding, the charset of the object name, and the default name "trid_<n>",
 * which the host forms from transport_id when name_len == 0 (:293-297). */
typedef struct {
  uint32_t size;             /* sizeof(dabx_mot_config) of the caller */
  uint32_t max_object_bytes; /* guard M3; 0 = 65 536; below 256 or above 4 MiB: DABX_E_ARG.  Read only when size >= 8 */
  int32_t  reserved[6];      /* zero */
} dabx_mot_config;           /* 32 bytes */
typedef struct dabx_mot_object_s {
  int64_t  byte_pos;         /* position of the object's first byte in the slot's sequence of object bytes */
  int64_t  frame;            /* dabx_pad_item.frame of the item whose group completed the object */
  uint32_t body_len;         /* bytes handed on: the sum of all stored segments (mot_object.cpp:286-291) */
  uint32_t body_size;        /* the header core's bodySize (:84) */
  uint16_t transport_id;
  uint16_t content_type;     /* get_content_type(): ((contentType << 8) & 0x3f00) | (contentSubType & 0xff), mot_object.h:71-75 */
  uint16_t name_len;         /* 0: the host forms "trid_<transport_id>" */
  uint8_t  au;               /* dabx_pad_item.au of that item (a carousel slot: flags, DABX_MOT_FLAG_DIR_ELEMENT) */
  uint8_t  repeat;           /* emissions of this object since the last reset(), minus one, saturating at 255: a host skips repeat != 0
                                without comparing bytes */
} dabx_mot_object;           /* 32 bytes, little-endian, no holes; the object's bytes: body_len of body (the stored segments in key order),
                                then name_len of name */
typedef struct {
  int64_t objects, object_bytes;    /* dabx_mot_object records emitted and their bytes */
  int64_t objects_lost;      /* objects that had left the rings before a dabx_read_mot_objects call could return them */
  int64_t groups;            /* DABX_PAD_DATAGROUP items walked */
  int64_t headers;           /* set_header calls that read a header core */
  int64_t segments;          /* body segments stored (:135-137) */
  int32_t crc_bad;           /* 1 */
  int32_t type_other;        /* 2 */
  int32_t no_tid;            /* 3 */
  int32_t grp_short;         /* guard M1 */
  int32_t hdr_bad;           /* guard M2 */
  int32_t seg_number_bad;    /* 6: :119-123 */
  int32_t seg_duplicate;     /* 6: :139-143 */
  int32_t resets;            /* reset() calls: transport-id changes (the first id after -1 included) and guard M3 */
  int32_t obj_overflow;      /* guard M3 */
  int32_t pad_overrun;       /* PAD items that had left the PAD rings before k_mot reached them (the rings hold two batches: always 0) */
  int32_t progress_events;   /* signal_pad_mot_progress (:168) */
  int32_t progress_pct;      /* ... and its last value */
  int32_t transport_id;      /* mTransportId, -1 at the start */
  int32_t segments_stored;   /* mMotMap.size() */
  int32_t active;            /* 1: MOT decoding is on for the slot (all else is zero otherwise) */
  int32_t reserved[5];
} dabx_mot_stats;            /* 128 bytes */
/* Switches the MOT decoding of slot subch_idx of `stream` on (cfg != NULL) or off (NULL).  On only for a slot whose PAD decoding is on, of
 * either source; DABX_E_ARG otherwise.  It starts with an empty object at the next PAD item emitted; calling it again restarts it.
 * Calling dabx_set_pad_mode for the slot, on or off, ends its MOT decoding: PAD restarts with empty rings.  The setting and the state stay
 * with the slot wherever dabx_set_subchannels says it "keeps decoding without interruption", a move to other capacity units included; a
 * new or changed slot loses them.  The PAD items of the slot are produced and delivered exactly as before.  An engine without a MOT slot
 * allocates and launches nothing for this stage.  Drains the engine. */
int  dabx_set_mot_mode(dabx_engine *e, int stream, int subch_idx, const dabx_mot_config *cfg);
/* The newest n objects still intact in the rings, oldest first: their records into info[], their bytes back to back into bytes[];
 * byte_pos is rebased to the returned buffer (info[0].byte_pos == 0).  When the bytes of n objects exceed max_bytes the newest objects that
 * fit are returned (bytes == NULL: records only).  Returns the number of objects.  Older unseen ones that left the rings are counted in
 * dabx_mot_stats.objects_lost.  The rings hold 256 records and at least two largest objects (max_object_bytes + 8 192 bytes each, as a
 * power of two).  Drains the engine like the other dabx_read_* calls. */
int  dabx_read_mot_objects(dabx_engine *e, int stream, int subch_idx, int n, dabx_mot_object *info, uint8_t *bytes, size_t max_bytes);
int  dabx_get_mot_stats(dabx_engine *e, int stream, int subch_idx, dabx_mot_stats *out);
/* ------------------------------------------------------------------------------------------------------------
 * MOT objects of a packet-mode carousel: what DataProcessor does with the MSC data groups of a packet-mode sub-channel with DSCTy 60
 * (data_processor.cpp:92-95, :209, :236; the DSCTy is dabx_packet_component's) behind the hand-over of dabx_datagroup_info --
 * MotHandler::add_MSC_data_group with its object cache (base/backend/data/mot/mot_handler.cpp:69-259, mh:), MotDirectory
 * (base/backend/data/mot/mot_dir.cpp:28-156, md:) and a MotObject per transport id (mot_object.cpp:71-323, mo:, as in "MOT objects of the
 * X-PAD" but no PAD element: no progress signal, mo:160) -- on the device (k_carousel, behind k_packet on the MSC batch's stream, one wave
 * per carousel-enabled packet-mode slot).  Every `emit signal_new_mot_object` (mo:300) is one dabx_mot_object plus its bytes.  Per
 * dabx_datagroup_info, in emission order:
 *   1 an empty group: return (mh:86-89).  crc_flag && !crc_ok: return (mh:91-94, crc_bad; the record's verdict, the CRC is not run again).
 *   2 next = ExtensionFlag ? 4 : 2 bytes.  SegmentFlag: lastFlag and the 15-bit segment number, next += 2 (mh:101-106); without it the number
 *     is 0.  UserAccessFlag: lengthInd = low nibble, the transport id from the two bytes behind the length byte whenever bit 4 of that byte
 *     is set, WHATEVER lengthInd says (mh:110-116); next moves by 1 + lengthInd only (mh:112, :117).  No transport id: return (mh:122-125,
 *     no_tid).
 *   3 the payload is everything behind next, minus the two CRC bytes when the flag is set (mh:120); segmentSize = its first 13 bits, the
 *     segment starts 2 bytes in (mh:139).
 *   4 the cache (mh:211-259): 15 entries.  getHandle looks an id up in the cache first and then in the directory's components; setHandle
 *     takes the first free entry, and when none is free it evicts the entry with the lowest order number (evictions) -- that object is gone.
 *   5 type 3 (mh:142-154): looked at only when the segment number is 0 (hdr_not_first otherwise); IGNORED when a handle for the id exists,
 *     in the cache or in the directory (mh:145-149, hdr_known) -- a header never replaces a header; else a new object, set_header
 *     (mo:71-115) on the segment, a cache entry.
 *   6 type 4 (mh:156-170): for an id without a handle the object is made with set_header run over the BODY segment's bytes (mh:159-164,
 *     from_body) and put into the cache; such an object keeps that header for good, since 5 ignores every later header.  Then
 *     add_body_segment (mo:117-175) and the emit when complete, as in "MOT objects of the X-PAD" 6.
 *   7 type 6 (mh:172-204), segment number 0: the same transport id as the directory's: return (dirs_repeated); else the directory and
 *     every object in it are deleted and a new MotDirectory is made from dirSize (30 bits), numObjects (16 bits) and the segment (md:28-57,
 *     dirs_begun): the segment goes to offset 0, and the directory is analysed at once when segmentSize >= dirSize.  Other segment numbers:
 *     dropped when there is no directory of that id (mh:198-201) or the segment is marked already (md:102); else a last flag sets
 *     num_dirSegments, the segment is marked and copied to segmentNumber * dir_segmentSize -- the size of segment 0 -- (md:104-108,
 *     dir_segments), and the directory is analysed when every segment below num_dirSegments is marked (md:112-118).  Nothing prevents a
 *     second analysis when a further segment arrives.
 *   8 analyse_theDirectory (md:124-152): base = 11, the 16-bit extension length is skipped, then for each of numObjects entries: a
 *     transport id of 0 ends the walk; else a MotObject as a directory element with set_header on the entry's bytes, base += 2 +
 *     headerSize, and setHandle puts it into the first component not in use (md:78-88, dir_objects).  A second analysis therefore
 *     registers nothing once all components are in use -- and registers entries AGAIN, behind the first ones, when the first walk ended
 *     early.  Kept.  (An object that finds no component is never seen again: only its headerSize is read.)
 *   9 any other type: return (mh:206-207, type_other).  Nothing is cleared after an emit.
 * Guards, where the reference reads outside the bytes it was given or grows without bound; each is counted:
 *   C1 (mh:103-115, :139, :151-167): a header field beyond the group, a payload shorter than 2 bytes or 2 + segmentSize beyond the payload:
 *      the group is ignored, state unchanged, grp_short (an empty group counts here too).  Checked in front of the dispatch of 5..9.
 *   C2 (mo:84-87, :212-230, :185): a type-3 or created-from-body segment shorter than the 7 bytes of the header core: the group is ignored
 *      and no handle is made.  An extension read at an index >= segmentSize ends the walk, as M2.  For a directory entry, whose
 *      set_header gets no size at all (md:145), the bound is the directory's end, and 8 192 bytes (headerSize has 13 bits).  hdr_bad.
 *   C3: M3 as it is (mo:135-137), obj_overflow.
 *   D1 (mh:188-189, md:127): segment 0 of a directory is shorter than the 13 bytes its fields and the analysis read: ignored, the old
 *      directory stays.  dir_short.
 *   D2 (md:46-47): dirSize > max_dir_bytes or numObjects > max_dir_objects: the directory is refused, the state is as if there were none of
 *      that id; the old one is still deleted, as mh:183-184 does.  dirs_refused.
 *   D3 (md:102, :107-108, :52): a directory segment number >= 512 (marked[512]) or a copy that would pass dirSize: the segment is dropped
 *      and not marked, its last flag not looked at.  dir_seg_bad.  The constructor's copy of segment 0 is clipped to dirSize.
 *   D4 (md:127, :133, :139-146): the analysis would read the extension length, an entry's id or its header core at or beyond dirSize: the
 *      walk ends there.  dir_cut.
 * Memory per carousel slot, B = max_object_bytes rounded up to 8, D = max_dir_objects, Y = max_dir_bytes rounded up to 8: one allocation of
 *   ring(B) + (15 + D) * (B + 8 192 + 65 536 + 56) + Y + 64 + 4 * D (rounded up to 8) bytes, ring(B) = 2 * (B + 8 192) as a power of two,
 * plus 256 * 32 bytes of records: every object has an arena, 8 KiB of name room and the 8 192-entry segment table, so the reference's
 * segment-number range is kept whole.  The defaults take 9.3 MB.
 * Parity of this path with the reference's object code is unpinned: mot_handler.cpp cannot be compiled without the GUI's headers
 * (dabradio.h), so the tests compare the device with a line-by-line restatement (tests/carousel_cases.py).
 * Out of scope: the SPI/EPG decoders, image decoding, the charset of the object name, the default name "trid_<n>", packet-mode FEC.  The
 * Journaline, TDC and IP handlers: the next section. */
#define DABX_MOT_FLAG_DIR_ELEMENT 1   /* dabx_mot_object.au of a carousel slot, bit 0: the dirElement argument of signal_new_mot_object */
typedef struct {
  uint32_t size;             /* sizeof(dabx_carousel_config) of the caller */
  uint32_t max_object_bytes; /* guard C3; 0 = 65 536; below 256 or above 4 MiB: DABX_E_ARG.  Read only when size >= 8 */
  uint32_t max_dir_objects;  /* guard D2; 0 = 49; above 1 009: DABX_E_ARG.  Read only when size >= 12 */
  uint32_t max_dir_bytes;    /* guard D2; 0 = 65 536; below 256 or above 1 MiB: DABX_E_ARG.  Read only when size >= 16 */
  int32_t  reserved[4];      /* zero */
} dabx_carousel_config;      /* 32 bytes */
typedef struct {
  int64_t objects, object_bytes;    /* dabx_mot_object records emitted and their bytes */
  int64_t objects_lost;      /* objects that had left the rings before a dabx_read_mot_objects call could return them */
  int32_t groups;            /* data groups walked */
  int32_t headers;           /* set_header calls that read a header core */
  int32_t segments;          /* body segments stored (mo:135-137) */
  int32_t crc_bad;           /* 1 */
  int32_t type_other;        /* 9 */
  int32_t no_tid;            /* 2 */
  int32_t grp_short;         /* guard C1, and the empty groups of 1 */
  int32_t hdr_bad;           /* guard C2 */
  int32_t seg_number_bad;    /* mo:119-123 */
  int32_t seg_duplicate;     /* mo:139-143 */
  int32_t resets;            /* reset() calls: one per object made (mo:75-79 in the constructor) and guard C3 */
  int32_t obj_overflow;      /* guard C3 */
  int32_t hdr_known;         /* 5: a type-3 group for an id that has a handle */
  int32_t hdr_not_first;     /* 5: a type-3 group with a segment number other than 0 */
  int32_t from_body;         /* 6: objects made from a body segment */
  int32_t evictions;         /* 4 */
  int32_t dirs_begun;        /* 7: directories made */
  int32_t dirs_repeated;     /* 7: segment 0 of the directory there is */
  int32_t dirs_refused;      /* guard D2 */
  int32_t dir_segments;      /* 7: directory segments stored, segment 0 included */
  int32_t dir_objects;       /* 8: objects registered in a component */
  int32_t dir_short;         /* guard D1 */
  int32_t dir_seg_bad;       /* guard D3 */
  int32_t dir_cut;           /* guard D4 */
  int32_t dg_overrun;        /* data groups that had left the packet rings before k_carousel reached them (the rings hold two batches: always 0) */
  int32_t active;            /* 1: carousel decoding is on for the slot (all else is zero otherwise) */
} dabx_carousel_stats;       /* 128 bytes */
/* Switches the carousel decoding of slot subch_idx of `stream` on (cfg != NULL) or off (NULL).  On only for a slot in packet mode
 * (dabx_set_packet_mode); DABX_E_ARG otherwise.  It starts with an empty cache and no directory at the next data group completed; calling
 * it again restarts it.  Calling dabx_set_packet_mode for the slot, on or off, ends its carousel decoding: the packet stage restarts with
 * empty rings.  The setting and the state stay with the slot wherever dabx_set_subchannels says it "keeps decoding without interruption", a
 * move to other capacity units included; a new or changed slot loses them.  The data groups of the slot are produced and delivered
 * exactly as before.  The objects are dabx_mot_object records, read with dabx_read_mot_objects (a slot is a PAD slot or a packet slot, never
 * both); for a carousel slot `frame` is dabx_datagroup_info.last_frame of the group that completed the object and the byte `au` carries
 * flags: DABX_MOT_FLAG_DIR_ELEMENT.  An engine without a carousel slot allocates and launches nothing for this stage.  Drains the engine. */
int  dabx_set_carousel_mode(dabx_engine *e, int stream, int subch_idx, const dabx_carousel_config *cfg);
int  dabx_get_carousel_stats(dabx_engine *e, int stream, int subch_idx, dabx_carousel_stats *out);
/* ------------------------------------------------------------------------------------------------------------
 * The data handlers of a packet-mode slot: what DataProcessor does with the MSC data groups of a packet-mode sub-channel whose handler is
 * not MotHandler (data_processor.cpp:53-101, :208, :236) behind the hand-over of dabx_datagroup_info -- tdc_dataHandler (TPEG; DSCTy 5
 * with application type 4), IpDataHandler (DSCTy 59) and JournalineDataHandler (DSCTy 44, or DSCTy 5 with application type 0x44a) -- on
 * the device (k_data_handler, behind k_packet on the MSC batch's stream, one wave per slot with the mode on), down to the bytes a TPEG
 * decoder, a UDP socket or an NML parser is fed: every put_data_into_ring_buffer / callback is one dabx_data_item plus its bytes.
 * dabx_data_handler_for says which handler a component needs.  N is the group's length in bytes; the reference's bit offsets are restated
 * in bytes; every name in the right-hand column of dabx_data_stats is a counter of the decision it stands beside.
 *
 * TDC (base/backend/data/tdc_datahandler.cpp:52-193, tdc:).  The whole group is searched, header and CRC included, and the group's own CRC
 * verdict is not looked at.  From o = 0, while o < N:
 *   1 o advances byte by byte while o + 2 < N and bytes o, o + 1 are not FF 0F (tdc:62-72); o + 2 >= N: return (tdc:73-76, walk_end).  A
 *     sync word in the last two bytes is therefore never found.  Kept.
 *   2 length = bytes o + 2, o + 3 as a SIGNED 16-bit value; length < 0 or length >= N - o: return (tdc:85-88, tdc_len_bad).
 *   3 the header check (tdc:91-113): bytes o .. o + 3, byte o + 6 and min(length, 11) bytes from o + 7; its CCITT CRC (start 0xFFFF,
 *     complemented) against bytes o + 4, o + 5; a mismatch: return (tdc_hdr_crc_bad).
 *   4 type (byte o + 6) 0 (tdc:130-151): the item is `length` bytes from o + 7, DABX_DATA_CRC_OK when check_crc_bytes(frame, length - 2)
 *     holds; a failure is only counted (tdc_crc0_bad) and the frame goes out all the same.  Type 1 (tdc:153-193): the item is `length`
 *     bytes from o + 7; the component walk of tdc:171-190 changes nothing observable and reads outside the frame: it is not performed.
 *     Any other type: return (tdc:123-126, tdc_type_other).
 *   5 o = o + 7 + length, and the loop goes on.
 * IP (base/backend/data/ip_datahandler.cpp:44-148, ip:):
 *   1 crc_flag && !crc_ok of the record: return (ip:59, ip_dg_crc_bad; the CRC is not run again).
 *   2 next = 2, + 2 with the extension flag, + 2 with the segment flag, whose fields are not used (ip:64-74); with the user-access flag
 *     lengthInd = the low nibble of the byte at next, next += 1 + lengthInd (ip:78-88; the transport id is not used).
 *   3 ipLength = bytes next + 2, next + 3, accepted only if ipLength < N (ip:95, else ip_len_bad).  Version nibble != 4: return (ip:103,
 *     ip_not_v4).
 *   4 h = low nibble of byte 0 of the datagram; the sum of its 2 h big-endian half-words, folded ONCE, is accepted when the low 16 bits of
 *     its complement are 0 (ip:121-129, else ip_checksum_bad).  The single fold is kept.  Protocol (byte 9) != 17: return (ip_proto_other).
 *   5 the item is bytes [4 h + 8, ipLength) of the datagram (ip:134, :145-147); zero bytes is a legal item.
 * Journaline (base/backend/data/journaline/dabdgdec_impl.c:130-296, dg:; journaline_datahandler.cpp:38-132, jl:; NML.cpp:363-385, nml:),
 * a counter per return code of DAB_DATAGROUP_DECODER_putData:
 *   1 N < 2, or the extension flag and N < 4: jl_hdr_short (code 2).  Segment flag: jl_segmented (3).  data_len = N - 2 - 2 ext; 0: jl_empty
 *     (4).  With the CRC flag: data_len < 2: jl_len_bad (5), then data_len -= 2, and crc_ok == 0 of the record: jl_crc_bad (6; the CRC is
 *     not run again).  Without the CRC flag: jl_no_crc (7).  Group type != 0: silently ignored (dg:227-235, jl_type_other).  The
 *     user-access flag is ignored: its field stays in the object.  Kept.
 *   2 the object is data_len bytes behind the header.  nml_len < 4: nml_short (nml:363-368).  Type bits (byte 2 >> 5) 0 or above 4: the
 *     reference makes these INVALID and drops them (jl:105-106), so does the device (nml_type_bad).
 *   3 otherwise one item, DABX_DATA_NEW_REVISION set when the object id was never filed or its revision index differs from the one filed
 *     (jl:113-125); the table (64 KiB per slot: id -> revision, 0xFF = none) is updated either way.  With only_new_revisions an object
 *     without the flag is counted (nml_repeat) and not emitted.
 *   Stated deviation: the device files every object that passes 2; the reference files only what its parser (inflate, item walk) accepted.
 * Guards, where the reference reads outside the group or its buffer; each is counted and the handler returns:
 *   T1 (tdc:80-84): o + 7 > N, length, CRC and type lie beyond the group.  tdc_cut.
 *   T2 (tdc:103-108, :136-139, :166-169): o + 7 + length > N, the check vector and the copy read up to six bytes beyond the group.  tdc_cut.
 *   T3 (tdc:140): length < 2, check_crc_bytes reads bytes -2 and -1 of its buffer.  The flag stays clear, tdc_crc0_short, the frame goes out.
 *   I1 (ip:47-50, :81, :94, :99-103, :114-123, :134, :146), counted once as ip_short and the group dropped: a header field or the length
 *      word beyond the group; ipLength < 10 (0 included: ipVector[0], data[9]); next + ipLength > N; 4 h > ipLength; ipLength - 4 h - 8 < 0.
 *      In the order of the reference's reads: flags, lengthInd, length word, then ip:95, then ipLength < 10 and next + ipLength > N, the
 *      version, 4 h > ipLength, the checksum, the protocol, the negative payload.
 *   J1 (jl:48): data_len > 4096, the memcpy into nml[4096].  nml_too_long, in front of nml_short.
 * Memory per slot: a byte ring of the size of the packet slot's byte ring (a handler's output is never longer than the groups it reads), 256
 * records, and 64 KiB for a Journaline slot.
 * Parity of this path with the reference's object code is unpinned, as for every DataProcessor path: the handlers cannot be compiled
 * without the GUI's headers (dabradio.h), so the tests compare the device with a line-by-line restatement (tests/data_handler_cases.py).
 * Out of scope: NML parsing and inflate, TPEG decoding, sending datagrams, _handle_TDC_async_stream (which does nothing observable),
 * packet-mode FEC.  In bulk the items travel in the data section of the slab (DABX_DELIVER_DATA, dabx_chunk_data below). */
#define DABX_DATA_HANDLER_TDC 1
#define DABX_DATA_HANDLER_IP 2
#define DABX_DATA_HANDLER_JOURNALINE 3
#define DABX_DATA_HANDLER_MOT 4       /* dabx_data_handler_for only: use dabx_set_carousel_mode */
#define DABX_DATA_TDC_0 1             /* dabx_data_item.kind: a TDC frame of type 0, ... */
#define DABX_DATA_TDC_1 2             /* ... of type 1, */
#define DABX_DATA_UDP 3               /* the payload of a UDP datagram, */
#define DABX_DATA_NML 4               /* an NML object */
#define DABX_DATA_CRC_OK 1            /* dabx_data_item.flags, TDC type 0: the frame's own CRC holds */
#define DABX_DATA_NEW_REVISION 2      /* ... NML: the object id was never filed or its revision index has changed */
typedef struct {
  uint32_t size;             /* sizeof(dabx_data_config) of the caller */
  int32_t  handler;          /* DABX_DATA_HANDLER_TDC, _IP or _JOURNALINE; anything else: DABX_E_ARG */
  int32_t  only_new_revisions; /* Journaline: objects without DABX_DATA_NEW_REVISION are not emitted.  Read only when size >= 12 */
  int32_t  reserved[5];      /* zero */
} dabx_data_config;          /* 32 bytes */
typedef struct {
  int64_t  byte_pos;         /* of the item's first byte in the bytes returned with it */
  int64_t  frame;            /* dabx_datagroup_info.last_frame of the group */
  uint16_t length;           /* bytes */
  uint8_t  kind;             /* DABX_DATA_TDC_0, _TDC_1, _UDP, _NML */
  uint8_t  flags;            /* DABX_DATA_CRC_OK, DABX_DATA_NEW_REVISION */
  uint16_t a;                /* TDC: the byte offset of the sync word in the group; UDP: the first 16-bit word of the UDP header (source port); NML: the object id */
  uint16_t b;                /* UDP: the second word (destination port); NML: object byte 2 (type / static / compressed / revision) in the
                                low byte, byte 1 of the group (continuity / repetition index) in the high byte; TDC: 0 */
  uint32_t group;            /* the group's index in the slot's sequence of data groups (dabx_packet_stats.dg_count counts them) */
  uint32_t reserved;
} dabx_data_item;            /* 32 bytes */
typedef struct {
  int64_t groups;            /* data groups handed to the handler */
  int64_t items, bytes;      /* dabx_data_item records emitted and their bytes */
  int64_t lost;              /* items that had left the rings before a dabx_read_data_items call could return them */
  int64_t dg_overrun;        /* data groups that had left the packet rings before k_data_handler reached them (the rings hold two batches: always 0) */
  int64_t walk_end;          /* TDC 1 */
  int64_t tdc_cut;           /* guards T1, T2 */
  int64_t tdc_len_bad;       /* TDC 2 */
  int64_t tdc_hdr_crc_bad;   /* TDC 3 */
  int64_t tdc_crc0_bad;      /* TDC 4: a type-0 frame emitted without DABX_DATA_CRC_OK */
  int64_t tdc_crc0_short;    /* guard T3 */
  int64_t tdc_type_other;    /* TDC 4 */
  int64_t ip_dg_crc_bad;     /* IP 1 */
  int64_t ip_len_bad;        /* IP 3 */
  int64_t ip_not_v4;         /* IP 3 */
  int64_t ip_checksum_bad;   /* IP 4 */
  int64_t ip_proto_other;    /* IP 4 */
  int64_t ip_short;          /* guard I1 */
  int64_t jl_hdr_short, jl_segmented, jl_empty, jl_len_bad, jl_crc_bad, jl_no_crc;      /* Journaline 1: return codes 2 .. 7 */
  int64_t jl_type_other;     /* Journaline 1 */
  int64_t nml_too_long;      /* guard J1 */
  int64_t nml_short;         /* Journaline 2 */
  int64_t nml_type_bad;      /* Journaline 2 */
  int64_t nml_repeat;        /* Journaline 3: objects held back by only_new_revisions */
  int64_t launches;          /* k_data_handler launches of the engine (whatever the slot) */
  int64_t active;            /* 1: a handler is on for the slot (all else but launches is zero otherwise) */
  int64_t handler;           /* DABX_DATA_HANDLER_* of the slot */
} dabx_data_stats;           /* 256 bytes */
/* Switches a data handler of slot subch_idx of `stream` on (cfg != NULL) or off (NULL).  On only for a slot in packet mode
 * (dabx_set_packet_mode); DABX_E_ARG otherwise, and for an unknown handler or a reserved word that is not 0.  It starts with empty rings
 * (and an empty Journaline table) at the next data group completed; calling it again restarts it.  Calling dabx_set_packet_mode for the
 * slot, on or off, ends it: the packet stage restarts with empty rings.  The setting and the state stay with the slot wherever
 * dabx_set_subchannels says it "keeps decoding without interruption", a move to other capacity units included; a new or changed slot loses
 * them.  Independent of the carousel mode: both may read the same groups.  The data groups of the slot are produced and delivered exactly
 * as before.  An engine without such a slot allocates and launches nothing for this stage.  Drains the engine. */
int  dabx_set_data_mode(dabx_engine *e, int stream, int subch_idx, const dabx_data_config *cfg);
/* The newest k <= n items of the slot that are still in its rings, oldest first, with exactly the contract of dabx_read_mot_objects: info
 * [n]; bytes (NULL: the records alone) receives the items' bytes back to back, byte_pos counted from the first returned; of the newest n
 * only the newest that fit max_bytes are returned.  Returns k; 0 for a slot without a handler.  Drains the engine. */
int  dabx_read_data_items(dabx_engine *e, int stream, int subch_idx, int n, dabx_data_item *info, uint8_t *bytes, size_t max_bytes);
int  dabx_get_data_stats(dabx_engine *e, int stream, int subch_idx, dabx_data_stats *out);
/* The switch of data_processor.cpp:53-101, a pure function: the handler of a packet-mode component with this DSCTy and (first) user
 * application type (dabx_packet_component; dabx_fig_user_apps_entry).  DABX_DATA_HANDLER_TDC, _IP, _JOURNALINE, DABX_DATA_HANDLER_MOT (use
 * the carousel mode) or 0: the reference installs an empty handler. */
int  dabx_data_handler_for(int dscty, int app_type);
/* The data section (DABX_DELIVER_DATA): one dabx_chunk_data per (stream, slot) from dabx_chunk_header_ext2.off_data, all zero for a slot
 * without a handler; behind the table every such slot has room for 256 records and for what the slot's data-group room holds (4 * 7
 * logical frames and DABX_DG_MAX_BYTES: a handler's output is never longer than the groups it read) -- of more the newest that fit are
 * delivered and the rest counted in items_lost.  Record i's item is the `length` bytes at bytes_off + byte_pos.  Gathered behind the
 * batch's stages (k_deliver_data) like the AAC section; the section exists while at least one slot has a handler on. */
typedef struct {
  int64_t  first_item;       /* number, since the handler was switched on, of the first record in the chunk */
  int32_t  n_items, items_lost;        /* records in the chunk; records between the previous chunk's and these that were not delivered */
  uint64_t rec_off, bytes_off;
  int64_t  n_bytes;
  int64_t  groups, items, bytes;       /* dabx_data_stats after the chunk's batch */
  int64_t  reserved[8];
} dabx_chunk_data;           /* 128 bytes */
/* ------------------------------------------------------------------------------------------------------------
 * Bulk delivery of the results to the host.  The reference hands every FIB to IFibDecoder::process_FIB
 * (base/decoder/fib_decoder_if.h:81, called from fic_decoder.cpp:234-261) and every logical frame to
 * FrameProcessor::add_to_frame (base/backend/frame_processor.h:43-46, called from backend.cpp:160) the moment it exists;
 * Mp4Processor hands on the RS-corrected super frame (mp4processor.cpp:149-158).  For n_streams ensembles the engine does the
 * same in bulk: with a delivery open, everything a CHUNK of frames produced -- a chunk is what one MSC batch decodes, at most
 * DABX_CHUNK_FRAMES frames of every stream; a dabx_process call closes its last chunk -- is gathered on the device into ONE
 * contiguous slab and copied with ONE asynchronous DMA (an SDMA engine) into a page-locked host slab, next to the decode of the following chunk.
 * No call of the receiver waits for it, nothing is copied per stream or per CIF.  dabx_read_fibs / _msc / _superframes /
 * _eti remain as the convenience form for single streams (they drain the engine and copy from the device rings); the ETI frames have
 * their bulk form too, DABX_DELIVER_ETI below.
 *
 * A slab starts with a dabx_chunk_header; all dabx_chunk_* offsets are bytes from the slab's first byte:
 *   stream table  dabx_chunk_stream[n_streams]              which frames of the stream the chunk holds + the stream's scalars
 *   slot table    dabx_chunk_subch[n_streams * max_subch]   which logical / super frames of the sub-channel + its counters
 *   FIBs          [n_streams][max_frames][12][32] bytes, CRC flags [n_streams][max_frames][12], frame records
 *                 dabx_chunk_frame[n_streams][max_frames]   (row f = frame first_frame + f of the stream, f < n_frames)
 *   logical frames of slot (s, j): n_cifs x 3 * kbps bytes from msc_off -- the bytes dabx_read_msc returns, oldest first
 *   super frames   of slot (s, j): n_sf rows of sf_pitch bytes (110 * kbps / 8 used) from sf_off -- dabx_read_superframes' bytes;
 *                  their n_sf dabx_superframe_info records (AU table, per-AU CRC verdicts, corrections) from sfi_off
 * Chunks are numbered from 0 and delivered in order.  dabx_process fails with DABX_E_STATE, before it has started anything,
 * when the call would close more chunks than there are free host slabs: a consumer that falls behind holds the receiver up,
 * it never loses data silently.  dabx_delivery_open refuses an engine whose FIB ring is shorter than a chunk (dabx_config.out_frames
 * < DABX_CHUNK_FRAMES) when FIBs are to be delivered; frames_lost / cifs_lost / sf_lost count what a device ring could not hold until
 * the chunk was packed all the same (always 0 so far).
 * Threads: dabx_delivery_next / dabx_delivery_release may be called from ONE consumer thread next to the thread that drives the
 * engine (dabx_push_iq*, dabx_process, ...); everything else keeps the one-thread-per-handle rule. */
#define DABX_CHUNK_FRAMES 7
#define DABX_CHUNK_MAGIC 0x43584244u       /* "DBXC" */
enum { DABX_DELIVER_FIB = 1, DABX_DELIVER_MSC = 2, DABX_DELIVER_SF = 4,
       /* logical frames only of the slots that are NOT DAB+ (instead of DABX_DELIVER_MSC): for a DAB+ service the logical frames' consumer,
          Mp4Processor, runs on the device and the host's input is the super frame -- FIB | SF | this = what a receiver's host side needs,
          half the bytes of "everything" for a DAB+ multiplex */
       DABX_DELIVER_MSC_NOT_DABPLUS = 8,
       /* the MSC data groups of the packet-mode slots (dabx_set_packet_mode): with this bit, or with what == 0, AND at least one packet-mode
          slot the slab gains a data-group section (dabx_chunk_dg below) and dabx_chunk_header.what shows the bit; without a packet-mode slot
          a slab is byte for byte what it is without the bit, dabx_delivery_slab_bytes included */
       DABX_DELIVER_DG = 16,
       /* the PAD items of the PAD-enabled slots (dabx_set_pad_mode): with this bit, or with what == 0, AND at least one PAD slot the slab
          gains a PAD section (dabx_chunk_pad below) and dabx_chunk_header.what shows the bit; without a PAD slot a slab is byte for byte
          what it is without the bit, dabx_delivery_slab_bytes included */
       DABX_DELIVER_PAD = 32,
       /* the MOT objects of the MOT-enabled PAD slots (dabx_set_mot_mode) and of the carousel slots (dabx_set_carousel_mode): with this bit,
          or with what == 0, AND at least one MOT or carousel slot the slab gains a MOT section (dabx_chunk_mot below) and dabx_chunk_header.what shows the bit; without a MOT slot a slab is byte for
          byte what it is without the bit, dabx_delivery_slab_bytes included */
       DABX_DELIVER_MOT = 64,
       /* ETI(NI) frames of every stream, assembled on the device (the ETI section, dabx_chunk_eti below).  Opt-in: what == 0 does NOT
          include it, and without the bit a slab, dabx_delivery_slab_bytes and the kernels launched are exactly what they are without it.
          One ETI stream per ensemble carries the whole FIC and MSC: a consumer of ETI needs no other bit.  Needs dabx_config.out_frames
          >= DABX_CHUNK_FRAMES, like the FIBs; an engine created FIC-only refuses it (DABX_E_STATE, as dabx_read_eti) */
       DABX_DELIVER_ETI = 128,
       /* the TII events of every stream whose detector runs on the device (dabx_set_tii_mode; the TII section, dabx_chunk_tii below).  Opt-in
          like DABX_DELIVER_ETI: what == 0 does NOT include it, and without the bit a slab, dabx_delivery_slab_bytes and the kernels launched
          are exactly what they are without it.  With the bit the header is followed by a dabx_chunk_header_ext, which announces the section.
          The bit adds to a delivery of something else (FIBs, logical frames, ...): what == DABX_DELIVER_TII alone is DABX_E_ARG, as the
          mask 256 was before the bit existed */
       DABX_DELIVER_TII = 256,
       /* the PCM of every slot whose MP2 audio is decoded on the device (dabx_set_mp2_audio_mode; the MP2 audio section, dabx_chunk_mp2_audio
          below).  Opt-in exactly like DABX_DELIVER_ETI and DABX_DELIVER_TII: what == 0 does NOT include it, the bit alone is DABX_E_ARG, and
          without the bit a slab, dabx_delivery_slab_bytes and the kernels launched are exactly what they are without it.  With the bit the
          header is followed by a dabx_chunk_header_ext; the section exists while at least one slot has the mode on */
       DABX_DELIVER_MP2_AUDIO = 512,
       /* the LOAS/LATM stream of every DAB+ slot whose access units are framed on the device (dabx_set_aac_stream_mode; the AAC section,
          dabx_chunk_aac below).  Opt-in exactly like DABX_DELIVER_ETI, DABX_DELIVER_TII and DABX_DELIVER_MP2_AUDIO: what == 0 does NOT include
          it, the bit alone or with only those two is DABX_E_ARG, and without the bit a slab, dabx_delivery_slab_bytes and the kernels
          launched are exactly what they are without it.  With the bit the header is followed by a dabx_chunk_header_ext; the section exists
          while at least one slot has the mode on.  The value is 2048, not 1024: the mask 1024 has always been refused with DABX_E_ARG and
          callers rely on that (tests/test_gpu_mp2_audio_delivery.py), so 1024 stays refused */
       DABX_DELIVER_AAC = 2048,
       /* the scope records of every stream whose IQ scope runs on the device (dabx_set_scope_mode; the scope section, dabx_chunk_scope
          below).  Opt-in exactly like the four bits above: what == 0 does NOT include it, the bit alone or with only DABX_DELIVER_ETI, _TII,
          _MP2_AUDIO and _AAC beside it is DABX_E_ARG, and without the bit a slab, dabx_delivery_slab_bytes and the kernels launched are
          exactly what they are without it.  With the bit the header is followed by a dabx_chunk_header_ext.  The value is 8192, not 1024
          and not 4096: both masks have always been refused with DABX_E_ARG and callers rely on that
          (tests/test_gpu_aac_stream_delivery.py), so both stay refused */
       DABX_DELIVER_SCOPE = 8192,
       /* the CIR and correlation-plot records of every stream that has the mode on (dabx_set_cir_mode; the CIR section, dabx_chunk_cir
          below).  Opt-in exactly like the five bits above: what == 0 does NOT include it, the bit alone or with only DABX_DELIVER_ETI, _TII,
          _MP2_AUDIO, _AAC and _SCOPE beside it is DABX_E_ARG, and without the bit a slab, dabx_delivery_slab_bytes and the kernels launched
          are exactly what they are without it.  With the bit the header is followed by a dabx_chunk_header_ext.  The value is 32768, not
          1024, 4096 or 16384: those masks have always been refused with DABX_E_ARG and callers rely on that, so they stay refused */
       DABX_DELIVER_CIR = 32768,
       /* the RF spectrum and waterfall records of every stream that has the mode on (dabx_set_spectrum_mode; the spectrum section,
          dabx_chunk_spectrum below).  Opt-in exactly like the six bits above: what == 0 does NOT include it, the bit alone or with only
          DABX_DELIVER_ETI, _TII, _MP2_AUDIO, _AAC, _SCOPE and _CIR beside it is DABX_E_ARG, and without the bit a slab,
          dabx_delivery_slab_bytes and the kernels launched are exactly what they are without it.  With the bit the header is followed by a
          dabx_chunk_header_ext.  1024, 4096 and 16384 stay refused with DABX_E_ARG, as ever */
       DABX_DELIVER_SPECTRUM = 65536,
       /* the FIG change events of every stream that follows the FIC on the device (dabx_set_fig_mode; the FIG section, dabx_chunk_fig
          below).  Opt-in exactly like the seven bits above: what == 0 does NOT include it, the bit alone or with only DABX_DELIVER_ETI, _TII,
          _MP2_AUDIO, _AAC, _SCOPE, _CIR and _SPECTRUM beside it is DABX_E_ARG, and without the bit a slab, dabx_delivery_slab_bytes and the
          kernels launched are exactly what they are without it.  With the bit the header is followed by a dabx_chunk_header_ext.  The value
          is 262144, not 131072: the mask 131072 has always been refused with DABX_E_ARG, alone and beside other bits, and callers rely on
          that (tests/test_gpu_spectrum_delivery.py), so 131072 stays refused, as 1024, 4096 and 16384 do */
       DABX_DELIVER_FIG = 262144,
       /* the items of every packet-mode slot that has a data handler on (dabx_set_data_mode; the data section, dabx_chunk_data below).
          Opt-in exactly like the eight bits above: what == 0 does NOT include it, the bit alone or with only DABX_DELIVER_ETI, _TII,
          _MP2_AUDIO, _AAC, _SCOPE, _CIR, _SPECTRUM and _FIG beside it is DABX_E_ARG, and without the bit a slab, dabx_delivery_slab_bytes and
          the kernels launched are exactly what they are without it.  dabx_chunk_header_ext is full: with this bit a second extension,
          dabx_chunk_header_ext2, follows it at byte 192 and announces the section, and off_stream is 256.  1024, 4096, 16384 and 131072
          stay refused */
       DABX_DELIVER_DATA = 524288 };
typedef struct {
  int32_t host_slabs;       /* page-locked host slabs, >= 2 (0 = default 4) */
  int32_t what;             /* DABX_DELIVER_* mask, 0 = everything */
  int32_t copy_engine;      /* 0 (default): the slab goes to the host on an SDMA engine (HSA runtime, hsa_amd_memory_async_copy): no CU is
                               involved, the receiver's kernels do not notice it.  1: hipMemcpyAsync -- on ROCm 7.2 a shader copy that holds up
                               every kernel running next to it for its duration (kept for comparison: tools/copy_interference.hip) */
  int32_t reserved[5];
} dabx_delivery_config;
typedef struct {
  uint32_t magic, abi;      /* DABX_CHUNK_MAGIC, DABX_ABI_VERSION */
  uint64_t seq;             /* chunk number */
  int32_t  n_streams, max_subch, max_frames /* DABX_CHUNK_FRAMES */, what;
  uint64_t bytes;           /* size of the slab as copied */
  uint64_t off_stream, off_subch, off_fib, off_crc, off_frame, off_msc, off_sf;
  uint64_t off_dg;          /* the data-group section: dabx_chunk_dg[n_streams * max_subch]; 0 = the slab has none */
  uint64_t off_pad;         /* the PAD section: dabx_chunk_pad[n_streams * max_subch]; 0 = the slab has none */
  uint64_t off_mot;         /* the MOT section: dabx_chunk_mot[n_streams * max_subch]; 0 = the slab has none */
  uint64_t off_eti;         /* the ETI section: dabx_chunk_eti[n_streams]; 0 = the slab has none */
} dabx_chunk_header;        /* 128 bytes */
/* The header's extension: present when, and only when, dabx_chunk_header.what carries a bit >= 256.  It follows the header at byte 128,
 * and the stream table then starts at 192 (off_stream says so: every table of a slab is found through the header's offsets). */
#define DABX_CHUNK_EXT_MAGIC 0x45584244u   /* "DBXE" */
typedef struct {
  uint32_t magic;           /* DABX_CHUNK_EXT_MAGIC */
  uint32_t bytes;           /* 64 */
  uint64_t off_tii;         /* the TII section: dabx_chunk_tii[n_streams]; 0 = the slab has none */
  uint64_t off_mp2_audio;   /* the MP2 audio section: dabx_chunk_mp2_audio[n_streams * max_subch]; 0 = the slab has none */
  uint64_t off_aac;         /* the AAC section: dabx_chunk_aac[n_streams * max_subch]; 0 = the slab has none */
  uint64_t off_scope;       /* the scope section: dabx_chunk_scope[n_streams]; 0 = the slab has none */
  uint64_t off_cir;         /* the CIR section: dabx_chunk_cir[n_streams]; 0 = the slab has none (the first of three words that were reserved) */
  uint64_t off_spectrum;    /* the spectrum section: dabx_chunk_spectrum[n_streams]; 0 = the slab has none (the second of them) */
  /* the FIG section: dabx_chunk_fig[n_streams]; 0 = the slab has none.  It takes the last of the reserved words, which keeps its old name
     beside the new one (an anonymous union: C11 and C++; compilers that speak GNU C take it in C99 as well) */
#if defined(__GNUC__)
  __extension__
#endif
  union { uint64_t off_fig; uint64_t reserved[1]; };
} dabx_chunk_header_ext;    /* 64 bytes */
/* The second extension: present when, and only when, dabx_chunk_header.what carries DABX_DELIVER_DATA.  It follows the first at byte 192,
 * and the stream table then starts at 256 (off_stream says so). */
#define DABX_CHUNK_EXT2_MAGIC 0x32584244u  /* "DBX2" */
typedef struct {
  uint32_t magic;           /* DABX_CHUNK_EXT2_MAGIC */
  uint32_t bytes;           /* 64 */
  uint64_t off_data;        /* the data section: dabx_chunk_data[n_streams * max_subch]; 0 = the slab has none */
  uint64_t reserved[6];     /* zero */
} dabx_chunk_header_ext2;   /* 64 bytes */
typedef struct {
  int64_t first_frame;      /* index, since the stream was opened, of the first frame in the chunk */
  int32_t n_frames;         /* frames of this stream in the chunk, 0..max_frames (a stream out of lock delivers none) */
  int32_t frames_lost;      /* frames decoded since the previous chunk that had left the FIB ring before this one was packed */
  int32_t state, fic_ratio_percent, cif_count;      /* as in dabx_stats, after the chunk's last frame */
  float   snr_db_est, freq_offs_bb_hz, clock_err_hz, signal_level;
  int32_t fic_ber_bits, fic_ber_errors;             /* FicDecoder's channel-BER counters (dabx_stats) */
  float   mer_db_est;                               /* dabx_stats.mer_db_est (0 unless dabx_set_lcd_statistics).  The two LCD statistics
                                                       (snr_db_est, mer_db_est) are what the demapper had last written when the record was
                                                       gathered: with 48 streams and more the chunk's last frame's MSC symbols may still be
                                                       in the demapper then (a HIP stream of its own), and they are that frame's or the
                                                       previous one's; dabx_get_stats after dabx_synchronize shows the last frame's */
  int64_t fib_ok, fib_total;                        /* cumulative */
} dabx_chunk_stream;        /* 72 bytes */
typedef struct {
  int64_t sym0_pos;         /* dabx_read_frame_info */
  int32_t start_index, reserved;
} dabx_chunk_frame;
typedef struct {
  int32_t active, subch_id, kbps, dab_plus;
  int64_t start_cif;        /* dabx_subch_stats.start_cif: logical frame i of the slot belongs to CIF start_cif + 16 + i */
  int64_t first_cif;        /* index of the chunk's first logical frame in the slot's sequence (0 = the slot's first) */
  int32_t n_cifs;           /* logical frames in the chunk */
  int32_t cifs_lost;
  int64_t first_sf;         /* index of the chunk's first super frame in the slot's sequence */
  int32_t n_sf, sf_lost;
  uint64_t msc_off, sf_off;
  int32_t sf_pitch, reserved;
  int64_t sf_ok, sf_fail, rs_corrected, rs_failed, fc_corrected, au_ok, au_bad;      /* cumulative, as dabx_subch_stats */
  uint64_t sfi_off;         /* n_sf dabx_superframe_info records, row i for super-frame row i (ABI 6) */
} dabx_chunk_subch;         /* 144 bytes */
/* The data-group section (DABX_DELIVER_DG): one dabx_chunk_dg per (stream, slot) from off_dg, all zero for a slot that is not in packet
 * mode; behind the table, per packet-mode slot, room for one record per possible packet of a chunk (4 * max_frames * kbps / 8
 * dabx_datagroup_info from rec_off) and for the chunk's logical-frame bytes plus DABX_DG_MAX_BYTES (from bytes_off): fixed by the
 * configuration like the rest of the slab.  It lies in the slab's head part, in front of off_msc, and is gathered behind k_deliver_msc.
 * The chunk carries the n_dg groups first_dg .. first_dg + n_dg - 1 of the slot's sequence, completed since the previous chunk: group i is
 * the n-th record's bytes_off + byte_pos .. + length (byte_pos counts from bytes_off; in the slot's own sequence the chunk's first byte
 * is byte dg_bytes - n_bytes).  dg_lost: groups completed since the previous chunk that are not in this one (they had left the slot's rings,
 * or -- useful lengths beyond the packets -- did not fit the room).  The counters are cumulative, as dabx_packet_stats. */
typedef struct {
  int64_t  first_dg;
  int32_t  n_dg, dg_lost;
  uint64_t rec_off, bytes_off;
  int64_t  n_bytes;
  int64_t  frames, packets, addr_match, continuity_err, crc_bad, len_bad, walk_short, dg_count, dg_bytes, dg_crc_bad, dg_overflow;
} dabx_chunk_dg;            /* 128 bytes */
/* The PAD section (DABX_DELIVER_PAD): one dabx_chunk_pad per (stream, slot) from off_pad, all zero for a slot without PAD decoding; behind
 * the table, per PAD slot, room for 144 dabx_pad_item from item_off and 144 * DABX_DL_MAX_BYTES + 16 896 bytes from bytes_off, fixed by
 * the configuration: a chunk is one batch, which completes at most 6 super frames of at most 6 access units whose X-PAD has at most 4
 * sub-fields, each emitting at most one item; a label is at most DABX_DL_MAX_BYTES, and the groups of a chunk are together at most what
 * was under assembly (below 16 896 bytes) plus less than a label per sub-field.  The section lies in the slab's head part, behind the
 * data-group section and in front of off_msc, and is gathered behind k_deliver_dg (k_deliver_pad).  The chunk carries the n_items items
 * first_item .. first_item + n_items - 1 of the slot's sequence, emitted since the previous chunk: item i is bytes_off + byte_pos ..
 * + length (byte_pos counts from bytes_off).  items_lost: items emitted since the previous chunk that are not in this one (always 0 with
 * this room).  The counters are cumulative, as dabx_pad_stats. */
typedef struct {
  int64_t  first_item;
  int32_t  n_items, items_lost;
  uint64_t item_off, bytes_off;
  int64_t  n_bytes;
  int64_t  superframes, aus, pad_aus, pad_bad, labels, label_bytes, groups, group_bytes, dg_crc_bad, dl_overflow, li_bad;
} dabx_chunk_pad;           /* 128 bytes */
/* The MOT section (DABX_DELIVER_MOT): one dabx_chunk_mot per (stream, slot) from off_mot, all zero for a slot without MOT decoding; behind
 * the table, per MOT slot, room for 16 dabx_mot_object from rec_off and 2 * max_object_bytes bytes from bytes_off, fixed by the
 * configuration.  The section lies in the slab's head part, behind the PAD section and in front of off_msc, and is gathered behind
 * k_deliver_pad (k_deliver_mot).  The chunk carries the n_objects objects first_object .. first_object + n_objects - 1 of the slot's
 * sequence, emitted since the previous chunk: object i is bytes_off + byte_pos .. + body_len + name_len (byte_pos counts from bytes_off).
 * objects_lost: objects emitted since the previous chunk that are not in this one -- more than 16, more bytes than the room, or gone from
 * the slot's rings; those still in the rings stay readable through dabx_read_mot_objects.  The counters are cumulative, as
 * dabx_mot_stats.  A carousel slot (dabx_set_carousel_mode) has its row and its room in the same section, behind the rooms of the MOT slots,
 * filled by a second gather launch (k_deliver_carousel); its counters are those of dabx_carousel_stats and progress_events is 0. */
typedef struct {
  int64_t  first_object;
  int32_t  n_objects, objects_lost;
  uint64_t rec_off, bytes_off;
  int64_t  n_bytes;
  int64_t  objects, object_bytes, groups, headers, segments, crc_bad, grp_short, hdr_bad, obj_overflow, resets, progress_events;
} dabx_chunk_mot;           /* 128 bytes */
/* The ETI section (DABX_DELIVER_ETI): one dabx_chunk_eti per stream from off_eti -- in the slab's head part, at the next multiple of 16
 * behind the MOT section, 64 * n_streams bytes -- and, at the next multiple of 256 behind the logical frames (the very end of the slab),
 * room for 4 * DABX_CHUNK_FRAMES rows of DABX_ETI_FRAME_BYTES (6144) bytes per stream: n_streams * 4 * DABX_CHUNK_FRAMES * 6144 bytes, fixed by
 * the configuration.  Stream s's rows start at rows_off = (start of the rows) + s * 4 * DABX_CHUNK_FRAMES * 6144; its n_eti rows are contiguous,
 * compacted and in CIF order: rows_off .. + n_eti * 6144 can go to a file or a pipe as it is, as a raw ETI(NI) stream.  With DABX_DELIVER_ETI alone
 * a slab is the header, the stream table, the slot table (each rounded up to 16 bytes), the ETI table, and from the next multiple of 256 the rows.
 * The frames are those of dabx_read_eti, byte for byte (row i is CIF first_cif + i in the sense of its counter: the FIC of that CIF with
 * the logical frame that completes with it of every active sub-channel in slot order, a moved sub-channel with its old start address
 * before the move, the frame counter as FIG 0/0 gave it after the frame's 12 FIBs), from a cursor of the stage's own in device memory: the two do
 * not disturb each other.  A delivery opened on a running stream starts with the CIFs decoded from then on and with the counter unknown:
 * rows begin with the first delivered frame that carries a FIG 0/0, exactly as a first dabx_read_eti call on empty rings would begin.
 * A sub-channel that is added or replaced (not one that only moves) makes the stage forget the counter in the same way, as it resets dabx_read_eti's cursor.
 * Every CIF decoded since the previous chunk is a row or counted: cifs_lost (it had left a ring before the chunk was packed, or exceeded the
 * rows' room; always 0 so far), cifs_waiting (the reference makes no frame for it either: a sub-channel's de-interleaver is not filled yet, or no FIG
 * 0/0 has been seen, eti_generator.cpp:156-160), cifs_refused (the configured sub-channels do not fit a frame: dabx_eti_frame's DABX_E_ARG).
 * A stream out of lock delivers n_eti = 0.  The rows are gathered behind the chunk's Viterbi decode and travel with the slab's tail (k_eti). */
typedef struct {
  int64_t  first_cif;       /* CIF of row 0; first_cif + n_eti is the next chunk's first_cif */
  int32_t  n_eti, cifs_lost, cifs_waiting, cifs_refused;
  int32_t  cif_hi, cif_lo;  /* CIFCountHi / Lo after the chunk's last frame (-1: no FIG 0/0 yet) */
  uint64_t rows_off;
  int64_t  fib_frames;      /* frames of the stream whose FIBs the stage has walked for the counter */
  uint64_t reserved[2];
} dabx_chunk_eti;           /* 64 bytes */
/* The TII section (DABX_DELIVER_TII): one dabx_chunk_tii per stream from dabx_chunk_header_ext.off_tii -- in the slab's head part, at the
 * next multiple of 16 behind the ETI table (or where that would be) -- followed by room for 4 event slots per stream, n_streams * 4 * (32 + 32 * 16)
 * bytes, fixed by the configuration: a chunk of DABX_CHUNK_FRAMES frames holds at most 4 TII null symbols, so at most 4 events even with
 * min_frames = 1.  An event slot is a dabx_tii_event followed by DABX_TII_MAX_RESULTS dabx_tii_result records (of which n_results are
 * valid), DABX_TII_EVENT_SLOT_BYTES in all; stream s's n_events slots lie one behind the other from ev_off, oldest first.  Every event a
 * stream's detector completed since the previous chunk is in the chunk or counted in events_lost.  Gathered on the front-end stream when
 * the chunk closes (k_deliver_tii): the events are front-end results like the FIBs. */
typedef struct {
  int64_t  first_event;     /* number, since the stream's mode was first switched on, of the first event in the chunk */
  int32_t  n_events, events_lost;
  uint64_t ev_off;
  int64_t  events_total;    /* events the stream's detector has completed so far: first_event + n_events */
} dabx_chunk_tii;           /* 32 bytes */
/* The scope section (DABX_DELIVER_SCOPE; "IQ scope and carrier plots" below): one dabx_chunk_scope per stream from
 * dabx_chunk_header_ext.off_scope, in the slab's head part behind the AAC section (or where that would be), followed by room for
 * DABX_CHUNK_FRAMES record slots for each stream that has the mode on WHEN THE DELIVERY IS OPENED (a chunk's frames cannot show more; a
 * stream switched on later has no room and delivers none: rec_off = 0).  A record slot is a dabx_scope_record, the IQ vector [1536] cf32
 * and the carrier vector [1536] f32, DABX_SCOPE_SLOT_BYTES in all, byte for byte what dabx_read_scope returns; stream s's n_records slots
 * lie one behind the other from rec_off, oldest first.  Every record a stream wrote since the previous chunk is in the chunk or counted in
 * records_lost.  Gathered on the front-end stream when the chunk closes (k_deliver_records), with a cursor of its own. */
typedef struct {
  int64_t  first_record;    /* number, since the stream's mode was first switched on, of the first record in the chunk */
  int32_t  n_records, records_lost;
  uint64_t rec_off;         /* 0 = the stream has no room in this delivery */
  int64_t  records_total;   /* records the stream has written so far: first_record + n_records */
} dabx_chunk_scope;         /* 32 bytes */
/* The CIR section (DABX_DELIVER_CIR; "Channel impulse response and correlation plot" below): one dabx_chunk_cir per stream from
 * dabx_chunk_header_ext.off_cir, in the slab's head part behind the scope section (or where that would be), followed by room for
 * DABX_CIR_CHUNK_RECORDS record slots for each stream that has the mode on WHEN THE DELIVERY IS OPENED (a stream switched on later has no
 * room and delivers none: rec_off = 0).  A chunk of DABX_CHUNK_FRAMES = 7 frames completes at most 2 records of each kind: a CIR record
 * takes six frames' worth of committed samples (1 179 648, fed a frame per step: windows complete six steps apart, so steps 1 and 7 of a
 * chunk at the most), a correlation show takes six counted calls of one per step (again steps 1 and 7 at the most) -- 4 slots.  (A host
 * that commits many frames before it processes them can complete a CIR window in every step; what does not fit is counted in
 * records_lost, the newest are kept.)  A record slot is a dabx_cir_record, the values [2048] f32 and the indices [72] int16,
 * DABX_CIR_SLOT_BYTES in all, byte for byte what dabx_read_cir returns; stream s's n_records slots lie one behind the other from rec_off,
 * oldest first, both kinds in the order they were completed.  Every record a stream wrote since the previous chunk is in the chunk or
 * counted in records_lost.  Gathered on the front-end stream when the chunk closes (k_deliver_records), with a cursor of its own. */
#define DABX_CIR_CHUNK_RECORDS 4
typedef struct {
  int64_t  first_record;    /* number, since the stream's mode was first switched on, of the first record in the chunk */
  int32_t  n_records, records_lost;
  uint64_t rec_off;         /* 0 = the stream has no room in this delivery */
  int64_t  records_total;   /* records the stream has written so far: first_record + n_records */
} dabx_chunk_cir;           /* 32 bytes */
/* The spectrum section (DABX_DELIVER_SPECTRUM; "RF spectrum and waterfall" below): one dabx_chunk_spectrum per stream from
 * dabx_chunk_header_ext.off_spectrum, in the slab's head part behind the CIR section (or where that would be), followed by room for
 * DABX_SPECTRUM_CHUNK_RECORDS record slots for each stream that has the mode on WHEN THE DELIVERY IS OPENED (a stream switched on later
 * has no room and delivers none: rec_off = 0).  Shows lie more than 512 000 consumed samples apart and a step consumes at most a frame and
 * a frame's worth of search (393 216 samples), so a chunk of DABX_CHUNK_FRAMES = 7 frames completes at most 6 records (three in lock): all
 * of them have room, and records_lost stays 0 (the field is kept for the shape the other sections have: the newest are kept should a
 * chunk ever complete more).  A record slot is DABX_SPECTRUM_SLOT_BYTES, byte for byte what dabx_read_spectrum returns; stream s's
 * n_records slots lie one behind the other from rec_off, oldest first.  Every record a stream wrote since the previous chunk is in the
 * chunk or counted in records_lost.  Gathered on the front-end stream when the chunk closes (k_deliver_records), with a cursor of its own. */
#define DABX_SPECTRUM_CHUNK_RECORDS 6
typedef struct {
  int64_t  first_record;    /* number, since the stream's mode was first switched on, of the first record in the chunk */
  int32_t  n_records, records_lost;
  uint64_t rec_off;         /* 0 = the stream has no room in this delivery */
  int64_t  records_total;   /* records the stream has written so far: first_record + n_records */
} dabx_chunk_spectrum;      /* 32 bytes */
/* The FIG section (DABX_DELIVER_FIG; "The FIC followed on the device" below): one dabx_chunk_fig per stream from
 * dabx_chunk_header_ext.off_fig, in the slab's head part behind the spectrum section (or where that would be), followed by room for
 * DABX_FIG_CHUNK_RECORDS event slots for each stream that has the mode on WHEN THE DELIVERY IS OPENED (a stream switched on later has no
 * room and delivers none: rec_off = 0).  A slot is a dabx_fig_event, byte for byte what dabx_read_fig_events returns; stream s's n_records
 * slots lie one behind the other from rec_off, oldest first.  The room is sized for a real ensemble's start-up: about 18 sub-channels' worth
 * of table and label events spread over the first second.  Of more events than that in one chunk the newest are delivered and the rest
 * counted in records_lost: events are notifications, the database (dabx_fig_subchannels, dabx_fig_labels, ...) stays complete.  Gathered
 * on the front-end stream when the chunk closes (k_deliver_records), with a cursor of its own. */
#define DABX_FIG_CHUNK_RECORDS 32
typedef struct {
  int64_t  first_record;    /* number, since the stream's mode was switched on, of the first event in the chunk */
  int32_t  n_records, records_lost;
  uint64_t rec_off;         /* 0 = the stream has no room in this delivery */
  int64_t  records_total;   /* events the stream has written so far: first_record + n_records */
} dabx_chunk_fig;           /* 32 bytes */
typedef struct {
  uint64_t seq;
  const void *data;         /* the host slab: valid until dabx_delivery_release(seq) */
  uint64_t bytes;
} dabx_chunk;
int  dabx_delivery_open(dabx_engine *e, const dabx_delivery_config *cfg /* NULL = defaults */);
int  dabx_delivery_close(dabx_engine *e);      /* drains the engine; chunks not yet fetched are dropped.  The consumer thread must have
                                                  left dabx_delivery_next before this (and before dabx_destroy) is called */
/* The oldest chunk not yet handed out: returns 1 and fills *out when it is complete in host memory, 0 when no chunk is ready
 * (wait == 0) or none is queued at all (wait != 0 waits for a queued one to land). */
int  dabx_delivery_next(dabx_engine *e, int wait, dabx_chunk *out);
int  dabx_delivery_release(dabx_engine *e, uint64_t seq);
/* Back-pressure for the engine's thread: waits (at most timeout_ms, < 0 = for ever) until n host slabs are free and returns the
 * number that are (>= n: a dabx_process call that closes n chunks will be accepted; < n: timed out).  n above the number of host slabs
 * the delivery was opened with is an error (it would wait for ever). */
int  dabx_delivery_wait_free(dabx_engine *e, int n, int timeout_ms);
/* What the copies themselves took (the copier's own clock around each transfer): link rate = bytes_copied / copy_seconds. */
typedef struct {
  uint64_t chunks_closed, chunks_landed, bytes_copied;
  double   copy_seconds, copy_seconds_max;     /* sum / longest single transfer */
  double   gather_wait_seconds;                /* the copier's waits for the chunks' gather kernels (idle time, not a cost) */
  int32_t  copy_engine;                        /* dabx_delivery_config.copy_engine */
  uint32_t sdma_engine_mask;                   /* hsa_amd_sdma_engine_id_t the transfers are put on (0: the runtime's choice) */
  double   calibration_GBps;                   /* rate of the 16-MiB probe transfer dabx_delivery_open made on that engine (an engine below
                                                  35 GB/s is replaced by the fastest of engines 0..7) */
  uint64_t reserved[3];
} dabx_delivery_info;
int  dabx_delivery_get_info(dabx_engine *e, dabx_delivery_info *out);
/* Bytes one slab takes with the sub-channels configured now (what one chunk moves over the link). */
long long dabx_delivery_slab_bytes(dabx_engine *e);

/* ------------------------------------------------------------------------------------------------------------
 * Bulk ingest: the delivery's mirror image for the samples.  dabx_push_iq* hands over one stream's samples per call -- right for a
 * device front end, 512 calls per chunk for a host that feeds 512 recordings.  With an ingest open the host fills ONE page-locked slab
 * with the next n samples of EVERY stream ([n_streams][n] samples of fmt, stream after stream), ONE SDMA transfer moves it, one kernel
 * converts it into all rings and one commit makes it readable:
 *     fill slab k;  dabx_ingest_submit(e, k, n);            the transfer starts, the call returns
 *     dabx_ingest_commit(e, k');                            waits for the transfer of slab k' (the previous one), converts, commits
 *     dabx_process(e, frames, 0);                           decodes it while slab k is still on the link
 * The raw_reader.cpp:66-70 / wav_reader.cpp:164 sample maps (fmt 2 / 1) run on the device: only 2 / 4 bytes per sample cross the link. */
typedef struct {
  int32_t host_slabs;       /* page-locked input slabs, >= 1 (0 = default 2) */
  int32_t fmt;              /* 0 cf32, 1 int16 IQ, 2 uint8 IQ: as dabx_push_iq (a native ring, dabx_create_ex: its own format only -- the commit
                               scatters the slab's codes into the rings, no cf32 is written) */
  int32_t max_frames;       /* samples per stream a slab holds, in frames of T_F (0 = default DABX_CHUNK_FRAMES) */
  int32_t copy_engine;      /* as dabx_delivery_config.copy_engine */
  int32_t reserved[4];
} dabx_ingest_config;
int  dabx_ingest_open(dabx_engine *e, const dabx_ingest_config *cfg);
/* The general form -- what a host with n_streams RECORDINGS has: every stream its own container, byte order, sample rate (the readers'
 * 1-ms linear interpolation of wav_reader.cpp:67-82,190-206 / xml_reader.cpp:237-244 runs on the device, per stream, with its state carried
 * from slab to slab) and its own length.  formats[s] = the dabx_iq_format of stream s as dabx_probe_iq_file returns it (data_offset /
 * data_bytes are ignored; cfg->fmt too).  A slab is n_streams regions of dabx_ingest_pitch() bytes; the host puts the next payload bytes
 * of stream s at byte s * pitch and says how many (n_bytes[s]: whole samples -- a reader keeps an odd tail for its next slab --, 0 = the
 * recording has ended or is not ready).  Still ONE SDMA transfer per slab, TWO kernel launches per commit whatever the number of streams
 * and formats, and the results are byte-identical to n_streams dabx_feed_bytes calls (tests/test_gpu_ingest.py).
 * With a native ring (dabx_create_ex) every stream's format must be one whose samples ARE the ring's codes; DABX_E_ARG otherwise. */
struct dabx_iq_format_s;                                                      /* "Recorded-IQ files" below */
int  dabx_ingest_open_formats(dabx_engine *e, const dabx_ingest_config *cfg, const struct dabx_iq_format_s *formats /* [n_streams] */);
long long dabx_ingest_pitch(dabx_engine *e);                                  /* bytes per stream region of a slab */
int  dabx_ingest_submit_bytes(dabx_engine *e, int k, const size_t *n_bytes /* [n_streams] */);   /* then dabx_ingest_commit(e, k) as above */
int  dabx_ingest_close(dabx_engine *e);
int  dabx_ingest_slab(dabx_engine *e, int k, void **host, size_t *capacity_bytes);
int  dabx_ingest_submit(dabx_engine *e, int k, size_t n_samples);     /* DABX_E_STATE: the slab's previous transfer has not been committed */
int  dabx_ingest_commit(dabx_engine *e, int k);                        /* DABX_E_STATE: a ring cannot take the samples (dabx_process first) */

/* Per-kernel timing with HIP events recorded on the engine's stream around every launch of a batch step
 * (bench.py's roofline leg).  dabx_get_profile drains the events recorded since the last call: for each of
 * the n kernels of a step it returns the accumulated milliseconds and the number of launches; names[i]
 * points to a static string.  Returns n.  dabx_set_profiling: 0 = off, 1 = every kernel as scheduled (kernels of the engine's
 * HIP streams overlap, so a duration includes what the kernel waited for the chip's other tenants; the event pairs
 * serialise neighbouring kernels a little: ~4 % on the 512-stream bench), -1 = every kernel with the host waiting for each
 * one (one kernel on the chip at a time: stand-alone durations; slow), 2 + i = only kernel i, as scheduled. */
#define DABX_MAX_KERNELS 16
int  dabx_set_profiling(dabx_engine *e, int on);
int  dabx_get_profile(dabx_engine *e, double total_ms[DABX_MAX_KERNELS], int64_t launches[DABX_MAX_KERNELS],
                      const char *names[DABX_MAX_KERNELS]);

/* ------------------------------------------------------------------------------------------------------------
 * Recorded-IQ files: the byte formats the reference's file readers accept, decoded and -- for
 * recordings that are not at 2.048 MS/s -- resampled ON THE GPU into a stream's IQ ring.  Only the raw bytes cross
 * PCIe (2..8 B per sample instead of 8).
 *   family RAW  .raw/.iq   uint8 IQ, (x - 127.38)/128                      devices/filereaders/raw_files/raw_reader.cpp:66-70,155-158
 *   family WAV  .sdr/.wav  RIFF/WAVE, 2 channels, 1.536..3.0 MS/s, normalised like libsndfile's sf_readf_float
 *                          (wav_files/wavfiles.cpp:55-92, wav_reader.cpp:164): u8 (x-128)/128, s8 x/128, i16 x/2^15,
 *                          i24 x/2^23, i32 (float)x/2^31, f32 as stored
 *   family UFF  .uff       XML header + payload (xml_filereader/xml_descriptor.cpp:98-240, xml_reader.cpp:254-398):
 *                          int8 x/127, uint8 (x-127.38)/128, int16/24/32 x/2^(Bits-1), float32; MSB|LSB; IQ|QI
 * Resampling follows the reference's non-liquid build: 1-ms blocks of rate/1000 input samples are linearly
 * interpolated to 2048 output samples (wav_reader.cpp:67-82,190-206; xml_reader.cpp:76-81,226-248; the two readers
 * differ in their table arithmetic and in how the first block is primed, selected by `family`).
 * By default four defects of the reference's UFF reader are NOT reproduced (each evidently a typo, not a format rule;
 * docs/history/r01-r04_design_notebook.md 9): QI/float32 is decoded as swapped IQ (the reference does not swap, xml_reader.cpp:530,540), int24/MSB takes
 * the middle byte of Q from its own sample (the reference reads lbuf[4*i+4] of its 1-ms read block, :316 and :462),
 * QI/int24/MSB sign-extends with 0xFF000000 (the reference ORs 0x7F000000, :465,:469), QI/uint8 is decoded from the data
 * (the reference indexes its 256-entry table with the loop counter, :423).  With dabx_iq_format.reference_quirks = 1 the
 * first three are reproduced bit for bit -- the bytes a user of the reference gets from such a file -- and QI/uint8 is
 * refused, because the reference's read runs past its table from the 128th sample of every block (undefined behaviour).
 * Single-channel (I-only / Q-only) UFF files are refused in both modes. */
enum { DABX_FAMILY_RAW = 0, DABX_FAMILY_WAV = 1, DABX_FAMILY_UFF = 2 };
enum { DABX_C_U8 = 0, DABX_C_S8 = 1, DABX_C_I16 = 2, DABX_C_I24 = 3, DABX_C_I32 = 4, DABX_C_F32 = 5 };
typedef struct dabx_iq_format_s {
  int32_t family;        /* DABX_FAMILY_* : normalisation rule + resampler flavour */
  int32_t container;     /* DABX_C_* */
  int32_t big_endian;    /* UFF Ordering="MSB", RIFX */
  int32_t swap_iq;       /* UFF channel order Q,I */
  int32_t bits;          /* UFF Bits attribute: integer scale is 2^(bits-1) */
  int32_t sample_rate;   /* Hz; 2048000 = no resampling */
  int64_t data_offset;   /* first payload byte in the file */
  int64_t data_bytes;    /* payload length (clipped to the file) */
  int32_t reference_quirks; /* 1: reproduce the reference's UFF reader defects bit for bit (see above); dabx_probe_iq_file sets 0 */
  int32_t reserved;
} dabx_iq_format;
typedef struct dabx_feed dabx_feed;

/* Host only: recognise the container by content (RIFF/RIFX magic, "<?xml"/"<SDR" header) else by extension
 * (.raw/.iq) and fill *fmt.  DABX_E_ARG for unreadable / unsupported files (dabx_last_error says why). */
int  dabx_probe_iq_file(const char *path, dabx_iq_format *fmt);
/* Bytes per complex sample of a format (2, 4, 6 or 8), or DABX_E_ARG. */
int  dabx_iq_sample_bytes(const dabx_iq_format *fmt);
/* One-shot conversion (stage level, fresh resampler state): payload bytes -> cf32 at 2.048 MS/s on the host.
 * Returns the number of complex samples written (<= max_out), or < 0. */
long long dabx_convert_iq_bytes(const dabx_iq_format *fmt, const void *bytes, size_t n_bytes, float *iq_out, size_t max_out);
/* Streaming feed into the IQ ring of `stream`: keeps the resampler state between calls; any split of the payload
 * into calls gives the same samples.  dabx_feed_bytes returns the number of 2.048 MS/s samples committed to the
 * ring, DABX_E_STATE when the ring cannot take them (process first), or another error. */
int  dabx_feed_open(dabx_engine *e, int stream, const dabx_iq_format *fmt, dabx_feed **out);
long long dabx_feed_bytes(dabx_feed *f, const void *bytes, size_t n_bytes);
/* Upper bound of the samples dabx_feed_bytes(n_bytes) can commit (ring-space planning). */
long long dabx_feed_bound(const dabx_feed *f, size_t n_bytes);
void dabx_feed_close(dabx_feed *f);

/* ------------------------------------------------------------------------------------------------------------
 * ETI(NI) output: the 6144-byte / 24-ms container EtiGenerator writes
 * (base/eti_handler/eti_generator.cpp:169-199 frame assembly, :207-308 header).
 * dabx_eti_frame is host only: cif_hi/cif_lo are FibDecoder::get_cif_count's values when the frame's FIC had been
 * parsed, minor the CIF's position 0..3 in the transmission frame, sc/msc the sub-channels in FIC order with their
 * 3*kbps logical-frame bytes, fic96 the three FIBs of this CIF.  Returns the bytes used before the 0x55 padding. */
#define DABX_ETI_FRAME_BYTES 6144
int  dabx_eti_frame(int cif_hi, int cif_lo, int minor, const dabx_subch_desc *sc, int n_subch, const uint8_t *fic96,
                    const uint8_t *const *msc, uint8_t *out /* 6144 */);
/* The same assembly on the device (stage level, host pointers): n frames of ONE layout, one wavefront per frame, through the kernel body of
 * the delivery's ETI stage (DABX_DELIVER_ETI).  cif_hi / cif_lo / minor [n]; fic96 [n][96]; msc [n][sum of 3 * kbps]: a frame's sub-channel
 * bytes one behind the other in sc's order; out [n][6144]; used [n] = dabx_eti_frame's return value per frame.  Refuses (DABX_E_ARG) what
 * dabx_eti_frame refuses, and a kbps that is not a multiple of 8 (no sub-channel of the standard has one; the copy runs in dwords). */
int  dabx_eti_frames_device(int n, const int32_t *cif_hi, const int32_t *cif_lo, const int32_t *minor, const dabx_subch_desc *sc, int n_subch,
                            const uint8_t *fic96, const uint8_t *msc, uint8_t *out, int32_t *used);
/* ETI frames of `stream` for the CIFs decoded since the previous call (at most max_frames, oldest first), assembled
 * from the engine's FIB and logical-frame rings for the configured sub-channels.  Like the reference the FIC of a
 * CIF is paired with the (time-de-interleaved) MSC data that completes with that CIF; frames start once every
 * sub-channel's de-interleaver is filled and FIG 0/0 has been seen.  *lost_cifs (optional) counts CIFs that had
 * already left the rings: call at least every min(out_frames, 8) processed frames.  Returns the frame count. */
int  dabx_read_eti(dabx_engine *e, int stream, int max_frames, uint8_t *out, int32_t *lost_cifs);

/* ------------------------------------------------------------------------------------------------------------
 * TII: TiiDetector, base/ofdm/tii_detector.h:26-37, .cpp:149-240.  The engine accumulates the FFT of every TII
 * null symbol ((CIF count & 7) >= 4, dab_processor.cpp:273-300) on the device.  Two ways to the transmitters, per stream one or the other:
 * on the host -- dabx_read_tii hands the sum to the stream's host detector (dabx_tii_*) once `min_frames` of them are in (DabProcessor's
 * tiiFramesToCount) and returns the transmitters found, strongest first -- or on the device: dabx_set_tii_mode below runs the same detector
 * behind the frame tail, at the reference's cadence, and its events are read in bulk (DABX_DELIVER_TII) or by dabx_read_tii_events. */
typedef struct {
  uint8_t main_id, sub_id;   /* STiiResult */
  float strength, phase_deg;
  int32_t non_etsi_phase;
} dabx_tii_result;
typedef struct dabx_tii dabx_tii;
int  dabx_tii_create(dabx_tii **out);
void dabx_tii_destroy(dabx_tii *t);
void dabx_tii_reset(dabx_tii *t);
void dabx_tii_set_collisions(dabx_tii *t, int on, int sub_id);       /* set_detect_collisions, set_subid_for_collision_search */
int  dabx_tii_add(dabx_tii *t, const float *null_fft /* 2048 cf32 */);   /* add_to_tii_buffer */
int  dabx_tii_process(dabx_tii *t, int threshold_db, dabx_tii_result *out, int max_out);   /* process_tii_data */
/* Returns the number of results (0 while fewer than min_frames TII null symbols have been accumulated);
 * *frames_accumulated (optional) = the count before the call.  A loss of lock resets the detector like
 * dab_processor.cpp:150-152. */
int  dabx_read_tii(dabx_engine *e, int stream, int min_frames, int threshold_db, int collisions, int collision_sub_id,
                   dabx_tii_result *out, int max_out, int32_t *frames_accumulated);

/* The detector on the device (csrc/tii_core.h, k_tii): dabx_tii_process line for line, one 256-thread block per stream, launched behind
 * every frame tail while at least one stream has the mode on.  A stream with the mode on that is in lock runs its detector in the step
 * whose TII null symbol brings the count of the sum to min_frames -- exactly when DabProcessor runs process_tii_data
 * (dab_processor.cpp:287-300) --, writes one event (also when no transmitter is found: n_results = 0), and clears sum and count.  Every float
 * sum and product is taken in dabx_tii_process's order; only |z| ((float)sqrt in double) and arg (the device library's atan2f) may differ
 * from the host's libm in the last bits, ids, flags and order differ only where a decision of the detector lies within those bits.
 * Results of equal strength keep the order in which the detector made them.  A loss of lock clears the detector's state, like dabx_read_tii.
 * dabx_read_tii on a stream whose mode is on is refused (DABX_E_STATE): the two would take each other's sum. */
#define DABX_TII_MAX_RESULTS 32
typedef struct {
  int32_t enable;
  int32_t min_frames;        /* tiiFramesToCount; 0 = 5 (dabradio.cpp:85-93) */
  int32_t threshold_db;      /* 0 = 8 (configuration.cpp:62-77) */
  int32_t collisions, collision_sub_id;      /* set_detect_collisions, set_subid_for_collision_search */
  int32_t reserved[3];
} dabx_tii_config;           /* 32 bytes */
typedef struct {
  int64_t frame;             /* the stream's frame (index since it was opened) whose null symbol completed the sum */
  int32_t n_results;         /* records stored behind the event: min(n_found, DABX_TII_MAX_RESULTS), the strongest */
  int32_t n_found;           /* transmitters the detector found */
  int32_t frames_in_sum;     /* TII null symbols in the sum */
  int32_t epoch;             /* detector-reset epoch: moves with every loss of lock */
  int32_t threshold_db;
  int32_t reserved;
} dabx_tii_event;            /* 32 bytes */
#define DABX_TII_EVENT_SLOT_BYTES (32 + 16 * DABX_TII_MAX_RESULTS)
typedef struct {
  int64_t events;            /* events written */
  int64_t results;           /* records stored in them */
  int64_t truncated;         /* events with n_found > n_results */
  int64_t resets;            /* times the detector's state was cleared after a loss of lock */
  int64_t launches;          /* k_tii launches of the engine (the kernel has no row in the profile table) */
  int64_t reserved[3];
} dabx_tii_stats;            /* 64 bytes */
/* stream = -1: all streams.  cfg = NULL: defaults, enabled.  Switching a stream's mode on clears its detector state.  The first enable
 * allocates the stage; an engine that never enables the mode allocates and launches nothing for it.  Drains the engine. */
int  dabx_set_tii_mode(dabx_engine *e, int stream, const dabx_tii_config *cfg);
/* The events `stream` completed since the previous call, oldest first, at most max_events: ev [max_events], res [max_events][32] (optional).
 * The device keeps the last 8 per stream; *lost (optional) counts those that had left.  Drains the engine; a cursor of its own, the
 * delivery's is another.  Returns the number of events. */
int  dabx_read_tii_events(dabx_engine *e, int stream, int max_events, dabx_tii_event *ev, dabx_tii_result *res, int32_t *lost);
/* Any engine; all zeros without the mode (launches is the engine's, the same for every stream). */
int  dabx_get_tii_stats(dabx_engine *e, int stream, dabx_tii_stats *out);
/* The detector on crafted sums (stage level, host pointers, no engine): n independent detectors, one block each, through the device
 * function of k_tii.  sums [n][2048] cf32; pairs [n][768] cf32 is the detectors' state, in and out, so a caller can run rounds;
 * cfg [n] (min_frames is not looked at; enable = 0: that detector's pairs and outputs are left as they are); out [n][32]. */
int  dabx_tii_process_device(int n, const float *sums, float *pairs, const dabx_tii_config *cfg, dabx_tii_result *out,
                             int32_t *n_results, int32_t *n_found);

/* ------------------------------------------------------------------------------------------------------------
 * IQ scope and carrier plots: what OfdmDecoder hands its user on a shown symbol -- the constellation mIqVector and the per-carrier plot
 * mCarrVector (base/ofdm/ofdm_decoder.cpp:258-291, 303-324) --, computed on the device from the state the engine's demapper keeps
 * (csrc/scope_core.h, k_scope: one 768-thread block per stream with the mode on, directly in front of the frame's first demapper launch;
 * docs/history/scope.md).  The demapper kernels are not touched: k_scope replays the frame's demapper recurrences up to the shown symbol.
 * Which symbol (cfg.symbol): 0 follows the reference's two counters (mShowCntIqScope > 76 on symbol mNextShownOfdmSymbIdx, which the
 * statistics counter (> 380) moves on by one, 75 wrapping to 1; :154-157, :323, :349-351; neither is touched by reset()) -- from a fresh
 * engine decoded frames 3, 5, 7 at symbol 1, then frame 9 at symbol 2, and so on; 1..75 shows that symbol of every decoded frame (the two
 * counters run on underneath as they would with 0).  The counters are the stream's, kept on the device, advanced only by frames the
 * stream decodes while its mode is on; changing the types of an enabled stream keeps them.
 * iq_type: EIqPlotType 0..2 (glob_enums.h: PHASE_CORR_CARR_NORMED, PHASE_CORR_MEAN_NORMED, RAW_MEAN_NORMED).  3 and 4 (the DC-offset plots)
 * are refused with DABX_E_ARG: they need the DC bin and mDcAdc, which the stored spectra do not carry.
 * carrier_type: ECarrierPlotType 0..9 (SB_WEIGHT, EVM_PER, EVM_DB, STD_DEV, PHASE_ERROR, PRS_PHASE, PRS_PHASE_UNWRAP, FOUR_QUAD_PHASE,
 * REL_POWER, SNR) and 13 (NULL_OVR_POW).  10..12 (the three NULL_* level plots) are refused with DABX_E_ARG: they need a per-bin IIR over
 * null-symbol spectra that nothing keeps.  STD_DEV needs dabx_set_lcd_statistics(on) (the phase-deviation IIR, :204-208): DABX_E_STATE
 * without it.  REL_POWER and NULL_OVR_POW use mMeanPowerOvrAll as it stands after carriers 0..k of the shown symbol (:214 lies inside the
 * carrier loop), the two mean-normed IQ plots as it stood in front of the symbol (:162).
 * The IQ vector is indexed by nomCarrIdx, the carrier vector by realCarrRelIdx, as the reference fills them. */
typedef struct {
  int32_t enable;
  int32_t iq_type;           /* EIqPlotType 0..2 */
  int32_t carrier_type;      /* ECarrierPlotType 0..9, 13 */
  int32_t symbol;            /* 0 = the reference's cadence, 1..75 = this OFDM symbol of every decoded frame */
  int32_t reserved[4];
} dabx_scope_config;         /* 32 bytes */
typedef struct {
  int64_t frame;             /* the stream's frame (index since it was opened) the symbol belongs to */
  int32_t symbol;            /* 1..75 */
  uint8_t iq_type, carrier_type, soft_bit_type /* ESoftBitType 1..3 the demapper ran with */, reserved0;
  float   mean_value;        /* mMeanValue in front of the symbol (:234-250) */
  float   mean_power_all;    /* mMeanPowerOvrAll in front of the symbol (:162) */
  int32_t reserved[2];
} dabx_scope_record;         /* 32 bytes */
#define DABX_SCOPE_CARRIERS 1536
#define DABX_SCOPE_SLOT_BYTES (32 + DABX_SCOPE_CARRIERS * 8 + DABX_SCOPE_CARRIERS * 4)   /* record, IQ vector (cf32), carrier vector (f32) */
typedef struct {
  int64_t shows;             /* records written for the stream */
  int64_t lost;              /* records dabx_read_scope found gone from the ring of 8 */
  int64_t launches;          /* k_scope launches of the engine (the kernel has no row in the profile table) */
  int64_t reserved[5];
} dabx_scope_stats;          /* 64 bytes */
/* ofdm_decoder.h:86-88, set_select_iq_plot_type / set_select_carrier_plot_type.  stream = -1: all streams.  cfg = NULL: defaults (types 0,
 * the reference's cadence), enabled.  The first enable allocates the stage; an engine that never enables the mode allocates and launches
 * nothing for it, and with no stream enabled the launch sequence is what it is without the mode.  Drains the engine. */
int  dabx_set_scope_mode(dabx_engine *e, int stream, const dabx_scope_config *cfg);
/* ofdm_decoder.cpp:320-322 (the two ring buffers and signal_slot_show_iq).  The records `stream` completed since the previous call, oldest
 * first, at most max_records: recs [max], iq [max][1536] cf32, carr [max][1536] f32 (either vector optional).  The device keeps the last 8
 * per stream; *lost (optional) counts those that had left.  Drains the engine; a cursor of its own.  Returns the number of records. */
int  dabx_read_scope(dabx_engine *e, int stream, int max_records, dabx_scope_record *recs, float *iq, float *carr, int32_t *lost);
/* Any engine; all zeros without the mode (launches is the engine's, the same for every stream).  (:323: every show counts.) */
int  dabx_get_scope_stats(dabx_engine *e, int stream, dabx_scope_stats *out);
/* ofdm_decoder.cpp:154-157, :323, :349-351 on the host, no engine and no device: the two counters over the 75 decode_symbol calls of one
 * decoded frame -- the very function k_scope runs.  counters = { mShowCntIqScope, mShowCntStatistics, mNextShownOfdmSymbIdx }, in and out
 * (a fresh decoder: 0, 0, 1).  Returns the symbol shown in that frame, 0 = none. */
int  dabx_scope_cadence_frame(int32_t counters[3]);

/* ------------------------------------------------------------------------------------------------------------
 * Channel impulse response and correlation plot: the two displays that tell the transmitters of an SFN apart (csrc/cir_core.h, k_cir and
 * k_cir_corr; docs/history/cir.md).  One opt-in mode, two kinds of record:
 * kind 0, the CIR of CirViewer::show_cir (base/spectrum_viewer/cir_viewer.cpp:54-107, scalar build) over the window SampleReader captures
 * (base/main/sample_reader.cpp:179-196, :250-265; CIR_BUFF_SIZE = 97 x 2048).  For a stream switched on at read position `base`, window n
 * covers the absolute sample positions [base + n * 1 179 648, base + n * 1 179 648 + 198 656) -- six frames' worth of consumed samples
 * apart, whether the stream is in lock or searching, as the reference counts them.  The samples are those the frame head reads in front
 * of its NCO: behind the DC / IQ correction where that is on, converted from a native ring as every kernel converts them.  Row j (0..384)
 * is the 2048 samples from the window's first + 512 j: forward transform, product with the conjugate reference table (the PRS correlator's),
 * unnormalised backward transform, y[j] = sqrtf(max_i(re^2 + im^2)) / 26000 with max starting at 0 and a strict `>` (:86-93).  Kept: a row
 * with a NaN anywhere gives 0 (a NaN wins no comparison), a row whose largest square overflows gives inf.  The rows are computed as their
 * samples are committed, at the head of every front-end step -- about 64 per stream and step instead of 385 every sixth --, so a row's
 * samples are normally unread and intact; row 384 completes the record.  A step computes rows of one window only.
 * The trust rule: a row is only read if no push the ABI has accepted may be writing one of its ring slots -- its first sample has not
 * been read by the receiver yet (>= rd), or nothing issued so far reaches round the ring to it (>= write horizon - ring length; a
 * zero-copy commit without dabx_announce_write puts the horizon at ~0).  Looked at before and after the row's loads.  Otherwise
 * y[j] = -1 and the row counts in rows_untrusted.
 * Deviation: switching the CIR off and on again starts a new window at the stream's read position then; the reference would splice the
 * half-filled buffer.
 * kind 1, the correlation plot of PhaseReference::correlate_with_phase_ref_and_find_max_peak (base/ofdm/phasereference.cpp:110-195): the
 * mean of |corr| over the 2048 lags of the sync window, the accepted peak indices mIndices of the call that shows (:143-169) and the
 * threshold line sum * iThreshold (:192).  k_cir_corr stands directly in front of the frame head, evaluates its two guards (in lock, a
 * frame's samples committed) and computes the same |corr| from the same samples, NCO phase and rounded frequency with the same device
 * function.  The reference's state machine, quirks included: mean += |corr| on EVERY call, also those that return -1 (:121); sum == 0
 * returns (:128); a call without an accepted peak returns without counting (:171); otherwise ++counter, and when counter > 5 the mean is
 * divided by 6, shown with sum * threshold and ALL accepted indices in walk order, and counter = 0 (:179-193) -- the mean is NOT cleared
 * (no line does), so every later show carries a sixth of the one before.  The threshold factor is the stream's: 3 after a search, doubled
 * in lock.  At most 69 indices: the walk visits 750 positions and an accepted peak moves it on by 11 (:166 and the loop's own step).
 * While a stream has the correlation on, the search for streams out of lock runs in step, as it does with cfg.dc_iq_correction: a search
 * running beside the step could hand a stream to the frame head between k_cir_corr and the head, and the plot would miss a call the
 * head made.  Deviation: the correlations the SEARCH makes of candidates that fail are not accumulated (the search kernel is not touched);
 * a candidate that correlates is counted once, when the frame head repeats it. */
typedef struct {
  int32_t enable;
  int32_t cir;               /* 0/1: kind 0 */
  int32_t correlation;       /* 0/1: kind 1 */
  int32_t reserved[5];       /* 0 */
} dabx_cir_config;           /* 32 bytes */
typedef struct {
  int64_t frame;             /* frames the stream had decoded when the record was completed */
  int64_t first_sample;      /* kind 0: the window's first absolute sample position; kind 1: the sync window's (the read position of the call that showed) */
  float   threshold;         /* kind 1: sum * iThreshold of the call that showed (:192); kind 0: 0 */
  int32_t rows_untrusted;    /* kind 0: rows given up for the trust rule (their value is -1) */
  int16_t n_values;          /* 385 (kind 0) or 2048 (kind 1) */
  int16_t n_indices;         /* kind 1: accepted peaks, 0..69 */
  uint8_t kind;              /* DABX_CIR_KIND_* */
  uint8_t reserved[3];
} dabx_cir_record;           /* 32 bytes */
#define DABX_CIR_KIND_CIR 0
#define DABX_CIR_KIND_CORRELATION 1
#define DABX_CIR_ROWS 385                /* (97 * 2048 - 2048) / 512 + 1 */
#define DABX_CIR_WINDOW 198656           /* 97 * 2048 */
#define DABX_CIR_PERIOD 1179648          /* 6 * 196 608 */
#define DABX_CIR_CORR_LAGS 2048
#define DABX_CIR_MAX_INDICES 69          /* ceil(750 / 11) */
#define DABX_CIR_INDEX_ROOM 72           /* the index list's int16 slots in a record slot */
#define DABX_CIR_SLOT_BYTES (32 + DABX_CIR_CORR_LAGS * 4 + DABX_CIR_INDEX_ROOM * 2)   /* record, values [2048] f32, indices [72] int16 */
typedef struct {
  int64_t shows[2];          /* records completed, per kind */
  int64_t lost;              /* records dabx_read_cir found gone from the ring of 4 */
  int64_t rows_untrusted;    /* CIR rows given up for the trust rule, all windows */
  int64_t launches;          /* steps of the engine that launched a kernel of the stage */
  int64_t reserved[3];
} dabx_cir_stats;            /* 64 bytes */
/* stream = -1: all streams.  cfg = NULL or enable = 0: off.  The first enable allocates the stage; an engine that never enables the mode
 * allocates and launches nothing for it, and with no stream enabled the launch sequence is what it is without the mode.  Switching a
 * stream's CIR on (from off) puts `base` at its read position; switching its correlation on (from off) clears its mean and counter.
 * Drains the engine. */
int  dabx_set_cir_mode(dabx_engine *e, int stream, const dabx_cir_config *cfg);
/* The records `stream` completed since the previous call, oldest first, both kinds in the order they were completed, at most max_records:
 * recs [max], values [max][2048] f32 (the first n_values of a row count, the rest is 0), indices [max][72] int16 (the first n_indices;
 * either array optional).  The device keeps the last 4 per stream; *lost (optional) counts those that had left.  Drains the engine; a
 * cursor of its own.  Returns the number of records. */
int  dabx_read_cir(dabx_engine *e, int stream, int max_records, dabx_cir_record *recs, float *values, int16_t *indices, int32_t *lost);
/* Any engine; all zeros without the mode (launches is the engine's, the same for every stream). */
int  dabx_get_cir_stats(dabx_engine *e, int stream, dabx_cir_stats *out);
/* cir_viewer.cpp:66-95 on crafted rows, no engine: the row function of k_cir on n_rows windows of 2048 cf32 samples each (iq [n][2048]
 * interleaved re, im), y [n]. */
int  dabx_cir_rows_device(const float *iq, int n_rows, float *y);
/* The window / row bookkeeping k_cir and k_cir_finish run, on the host, no engine and no device.  walk = { base, window, rows_done }, in
 * and out; wr = one past the last committed sample; cap = the most rows a step takes.  Returns the number of rows due (rows_done ..
 * rows_done + n - 1 of `window`, each with all 2048 samples below wr), *first (optional) = the first due row's first sample, *completed
 * (optional) = 1 if row 384 is among them; walk is moved on past them. */
int  dabx_cir_rows_due(int64_t walk[3], uint64_t wr, int32_t cap, int64_t *first, int32_t *completed);
/* The trust rule k_cir runs, on the host: 1 = a row whose first sample is `first` may be read. */
int  dabx_cir_row_trusted(uint64_t first, uint64_t rd, uint64_t horizon, uint64_t ring_len);

/* ------------------------------------------------------------------------------------------------------------
 * RF spectrum and waterfall: the display that shows whether a carrier is there at all, an adjacent-channel interferer, a tilted passband
 * or a DC spur -- in lock or not (csrc/spectrum_core.h, k_spectrum; docs/history/spectrum.md).  One opt-in mode, one record per show of
 * SpectrumViewer::show_spectrum (base/spectrum_viewer/spectrum_viewer.cpp:141-234) with the row WaterfallScope::show_waterfall
 * (waterfall_scope.cpp:52-79) paints from it.
 * The capture (base/ofdm/sample_reader.cpp:198-205, :267-272, :285-296): a window is the 2048 consumed samples from W on, behind the DC / IQ
 * correction where that is on and in front of the NCO.  It is shown at E, the first end of a get_samples call made with iShowSpec == true
 * -- a single-sample call of the null-symbol search (:96-99) or the read of one of a frame's symbols 1..75 (dab_processor.cpp:321); not
 * the T_u block in front of the PRS correlation, the rest of symbol 0 (:392, :409), the null symbol (:270) or the 20 T_u reads that seed
 * the level (:141) -- with E - W > 512 000; the next window starts at E.  While searching E = W + 512 001; in lock E is one of the
 * symbol ends sym0_end + 2552 j.
 * The show: the flat-top window (glob_defs.h:252-266, made in double and cast to float), the forward 2048-point transform, per display
 * bin the mean of |X| over four bins (bin i < 256 from transform bins 1024 + 4 i + j, bin 256 + i from 4 i + j), val = 20 log10f(y / 512 +
 * 1e-6f), the IIR db += 0.2f (val - db) from 0, the global extrema over the 512 bins and the local ones over bins 64..447 (strict
 * comparisons from -1000 / +1000), the four limits filtered with alpha = 0.01 / 0.10 / 1.00 from Glob {-30, -90} and Loc {-31, -50},
 * _calc_spectrum_display_limits (:112-139) on Glob, and on Loc only if Glob changed.  The waterfall: yMax = (Glob.Max + 5)(1 - s) +
 * Loc.Max s, yMin = Glob.Min (1 - s) + Loc.Min s with s = zoom_percent / 100; no row if yMax - yMin <= 0, otherwise
 * row[i] = (int)(clamp((db[i] - yMin) / (yMax - yMin), 0, 1) * 255).
 * k_spectrum stands directly behind the frame head of every front-end step while a stream has the mode on.  It evaluates a window as
 * soon as its 2048 samples are committed -- under the trust rule of the CIR stage (dabx_cir_row_trusted, the same function), looked at
 * before and after the loads -- and keeps the result until the schedule says it is shown.  A window that starts at a symbol end of the
 * frame the head has just begun is read before the receiver reads it; one that starts in a searched range lies behind the read position
 * and is read only if nothing issued reaches round the ring to it.  A window that is not trusted is not evaluated: its record has
 * untrusted = 1, db, limits and row as they stood, and the IIR state does not move.
 * Deviations: the first window starts at the read position at which the mode is switched on (the reference's buffer fills from its last
 * reset); |X| is sqrtf(re^2 + im^2), not std::abs, which differs only where the squares leave the float range; a NaN db gives row index 0
 * (the reference's cast of a NaN is undefined); the schedule is taken from what the existing kernels leave -- read position, state, the
 * frame's symbol-0 position, the count of failed correlations -- so the position of a search candidate whose correlation failed is not
 * known: a show whose sample W + 512 000 may lie inside such a candidate's T_u block is placed as if it did not, up to 2048 samples
 * early, and has inexact = 1; while a stream has the mode on the search runs in step, as with cfg.dc_iq_correction.  The x axis, the
 * colour table and the painting stay with the host; so does the digital level bar. */
typedef struct {
  int32_t enable;
  int32_t averaging;         /* DABX_SPECTRUM_AVR_*: the filter of the four limits, 0 slow (0.01), 1 medium (0.10), 2 fast (1.00) */
  int32_t zoom_percent;      /* 0..100: the waterfall's scaling slider */
  int32_t reserved[5];       /* 0 */
} dabx_spectrum_config;      /* 32 bytes */
#define DABX_SPECTRUM_AVR_SLOW 0
#define DABX_SPECTRUM_AVR_MEDIUM 1
#define DABX_SPECTRUM_AVR_FAST 2
typedef struct {
  int64_t frame;             /* frames the stream had decoded at the show */
  int64_t first_sample;      /* W: the window's first absolute sample position */
  int32_t untrusted;         /* 1: the window was not evaluated (the trust rule) */
  int32_t row_valid;         /* 1: `row` is a waterfall row; 0: yMax - yMin <= 0, or untrusted */
  int32_t inexact;           /* 1: the show position may be up to 2048 samples early (above) */
  int32_t reserved;
} dabx_spectrum_record;      /* 32 bytes */
typedef struct {
  float glob_max, glob_min, loc_max, loc_min;    /* mSpecViewLimits behind the show */
  float y_min, y_max;        /* the waterfall's range for the stream's zoom */
  float reserved[2];
} dabx_spectrum_limits_rec;  /* 32 bytes: directly behind the record */
#define DABX_SPECTRUM_BINS 512
#define DABX_SPECTRUM_SIZE 2048
#define DABX_SPECTRUM_PERIOD 512000      /* INPUT_RATE / 4 */
#define DABX_SPECTRUM_RING 8
#define DABX_SPECTRUM_SLOT_BYTES (32 + 32 + DABX_SPECTRUM_BINS * 4 + DABX_SPECTRUM_BINS)   /* record, limits, db [512] f32, row [512] u8 */
typedef struct {
  int64_t shows;             /* records completed */
  int64_t untrusted;         /* ... of them not evaluated for the trust rule */
  int64_t lost;              /* records dabx_read_spectrum found gone from the ring of 8 */
  int64_t launches;          /* steps of the engine that launched the stage's kernel */
  int64_t inexact;           /* records with inexact = 1 */
  int64_t reserved[3];
} dabx_spectrum_stats;       /* 64 bytes */
/* stream = -1: all streams.  cfg = NULL or enable = 0: off.  The first enable allocates the stage and uploads the window table; an engine
 * that never enables the mode allocates and launches nothing for it, and with no stream enabled the launch sequence is what it is without
 * the mode.  Switching a stream on (from off) puts W at its read position and the IIR and the limits at their initial values; changing
 * averaging or zoom_percent on a running stream keeps the state.  Drains the engine. */
int  dabx_set_spectrum_mode(dabx_engine *e, int stream, const dabx_spectrum_config *cfg);
/* The records `stream` completed since the previous call, oldest first, at most max_records: recs [max], limits [max], db [max][512] f32,
 * row [max][512] u8 (the last three optional).  The device keeps the last 8 per stream; *lost (optional) counts those that had left.
 * Drains the engine; a cursor of its own.  Returns the number of records. */
int  dabx_read_spectrum(dabx_engine *e, int stream, int max_records, dabx_spectrum_record *recs, dabx_spectrum_limits_rec *limits, float *db,
                        uint8_t *row, int32_t *lost);
/* Any engine; all zeros without the mode (launches is the engine's, the same for every stream). */
int  dabx_get_spectrum_stats(dabx_engine *e, int stream, dabx_spectrum_stats *out);
/* spectrum_viewer.cpp:169-218 on crafted windows, no engine: the row function of k_spectrum on n windows of 2048 cf32 samples each
 * (iq [n][2048] interleaved re, im), one behind the other through ONE display buffer: state [512 + 4] in and out = mDisplayBuffer and the
 * four extrema {glob max, glob min, loc max, loc min} of the last window (in: ignored); lin [n][512] = mYValVec of each window (the
 * un-averaged linear values), db [n][512] = mDisplayBuffer behind each window, ext [n][4] (optional) = each window's extrema. */
int  dabx_spectrum_rows_device(const float *iq, int n, float *state, float *lin, float *db, float *ext);
/* spectrum_viewer.cpp:220-230 and waterfall_scope.cpp:57-60, the function k_spectrum runs, on the host, no engine and no device:
 * ext [4] = a show's extrema {glob max, glob min, loc max, loc min}; limits [4] in and out = {Glob.Max, Glob.Min, Loc.Max, Loc.Min};
 * averaging 0..2, zoom_percent 0..100; y [2] out = {yMin, yMax}.  Returns 1 if the waterfall has a row, 0 if not. */
int  dabx_spectrum_limits(const float ext[4], float limits[4], int averaging, int zoom_percent, float y[2]);
/* waterfall_scope.cpp:73-74 on the host: row [n] from db [n] for a range {yMin, yMax} with yMax - yMin > 0. */
int  dabx_spectrum_waterfall_row(const float *db, int n, const float y[2], uint8_t *row);
/* The capture schedule k_spectrum runs, on the host: the smallest end E of a show-enabled call with E - W > 512 000 inside one piece of
 * the receiver's walk, or -1 ("not in here").  kind 0: the searched range [a, b) (single-sample calls, ends a + 1 .. b); kind 1: a frame
 * whose symbol 0 ends at a (one past its last sample; ends a + 2552 j, j = 1..75; b is ignored). */
int64_t dabx_spectrum_next_show(uint64_t W, int kind, uint64_t a, uint64_t b);
/* One look of k_spectrum at a stream, on the host (csrc/spectrum_core.h, spectrum_look): what a front-end step did to the stream, from
 * what the existing kernels leave behind the frame head.  walk = { W, pos, lost_seen, state_seen } in and out: the window's first
 * sample, the position up to which the schedule has been evaluated, and the failed-correlation count and state (0 init, 1 searching,
 * 2 in lock) of the look before.  rd, state, sync_lost: the stream's read position, state and failed-correlation count now; frame_ok,
 * sym0_pos: whether this step's head has begun a frame, and where the T_u part of its symbol 0 lies.  Returns E (and moves W on to it,
 * as the kernel does) or -1; *inexact (optional) = 1 if E lies in a searched range in which a candidate's correlation failed. */
int64_t dabx_spectrum_look(int64_t walk[4], uint64_t rd, int state, int64_t sync_lost, int frame_ok, uint64_t sym0_pos, int32_t *inexact);

/* ------------------------------------------------------------------------------------------------------------
 * MP2 audio:the MP2 decoder of a DAB (MPEG-1/2 Audio Layer II) audio sub-channel on the device -- Mp2Processor's frame assembly and
 * _mp2_decode_frame (base/backend/audio/mp2processor.cpp:197-243, :292-609, :678-763; kjmp2), k_mp2_audio: one 256-thread block per
 * slot with the mode on, behind k_dabplus on the MSC batch's stream, beside the PAD stage.  The decoder is pure 32-bit integer
 * arithmetic, so the device gives the reference's samples exactly: 1152 stereo int16 samples per MP2 frame for which _mp2_decode_frame
 * returns > 0, interleaved L/R as opPcm holds them (a mono frame has the same sample in both channels).
 * The sync walk is that of the PAD stage's MP2 source ("Programme-associated data" above) on state of its own, so the two are
 * independent: either, both or neither may be on for a slot.  Every bit of GetSampleRate and GetData goes into MP2frame (:689, :725,
 * :737), kept per slot on the device: 6 * kbps bytes, all that is ever written; bytes are never cleared between frames, so a 48 kHz
 * frame behind a 24 kHz one leaves stale bytes behind it, which the parser can read.  Quirks kept: grouped code words beyond nlevels^3
 * (:325-329), scale factor 63 (:311), a 44.1 / 32 kHz header decoded with its own tables at the sticky rate, bound > sblimit (:478), the
 * sample of channel 0 copied to channel 1 from `bound` on whatever channel 1's scale factors say (:548-550), the header check in int
 * arithmetic (bit-rate index 0 passes :399 and is refused at :412), two's-complement wrap-around of U[i] * D[i] (:587: codes beyond
 * the quantiser's range reach it; codes within it stay below 2^31).
 * Guard G1: frame_pos may run past MP2frame (48 * kbps bytes): the longest parse reads 4500 bytes with quantiser tables A / B and 1690
 * with the LSR table (the window's refill reads up to two bytes more), so below 96 kbit/s a crafted header reaches it.  The device reads
 * bytes >= 6 * kbps as zero -- what the reference holds up to 48 * kbps --; a frame whose refill reads a byte at or beyond 48 * kbps is
 * counted in `overread`, flagged in its record, and decoded over zeros.
 * Parity with the reference's object code is unpinned, as for the rest of Mp2Processor (mp2processor.cpp needs the GUI's headers): the
 * tests compare the device with a line-by-line restatement (tests/mp2_audio_cases.py).
 * Out of scope: resampling and playback, the "MP2 dump" ring (frameBuffer; frame_size and the header bytes are in the record), the
 * signal_* cadence of :703-707. */
#define DABX_MP2_PCM_BYTES 4608        /* 1152 samples x 2 channels x int16 */
typedef struct {
  uint32_t size;             /* sizeof(dabx_mp2_audio_config) of the caller */
  int32_t  reserved[7];      /* zero */
} dabx_mp2_audio_config;     /* 32 bytes */
typedef struct dabx_mp2_audio_frame_s {
  int64_t  byte_pos;         /* position of the frame's first PCM byte in the slot's sequence of PCM bytes (a multiple of 4608) */
  int64_t  frame;            /* the logical frame in which the MP2 frame completed, in the numbering of dabx_pad_item.frame */
  int32_t  sample_rate;      /* sampleRate when the frame was decoded: the sticky 48 000 / 24 000 of :250-264 */
  int32_t  frame_size;       /* what _mp2_decode_frame returned (:454) */
  uint8_t  header[3];        /* MP2frame[1 .. 3] */
  uint8_t  stereo;           /* signal_is_stereo's argument (:444) */
  uint8_t  flags;            /* bit 0: the frame was over-read (guard G1) */
  uint8_t  reserved[3];
} dabx_mp2_audio_frame;      /* 32 bytes, little-endian, no holes */
typedef struct {
  int64_t decode_calls;      /* _mp2_decode_frame calls (:388) = MP2 frames completed */
  int64_t frames_out;        /* ... that returned > 0: records and PCM frames written */
  int64_t bad_header;        /* ... that returned at :397-402 (the only place errorFrames moves) */
  int64_t refused;           /* ... that returned at :412-421: free format (bit-rate index 0), sampling frequency 3 */
  int64_t overread;          /* frames_out with flags bit 0 (guard G1) */
  int64_t launches;          /* k_mp2_audio launches of the engine (the kernel has no row in the profile table) */
  int32_t sample_rate;       /* sampleRate */
  int32_t frames_lost;       /* frames that had left the rings before a dabx_read_mp2_audio call could return them */
  int16_t number_of_frames, error_frames;      /* the live window of :388-394 */
  int16_t voffs;             /* Voffs */
  int16_t active;            /* 1: the mode is on for the slot (all else but launches is zero otherwise) */
} dabx_mp2_audio_stats;      /* 64 bytes */
/* Switches MP2 audio decoding of slot subch_idx of `stream` on (cfg != NULL) or off (NULL).  On: only an active slot with dab_plus == 0
 * that is not in packet mode, at a multiple of 8 kbit/s up to 384 -- the rules of DABX_PAD_SOURCE_MP2 --, DABX_E_ARG otherwise.  A slot
 * that is switched on starts as a fresh Mp2Processor: searching for sync, sampleRate 48 000, V and MP2frame zero, Voffs 0, empty rings;
 * the walk starts with the next logical frame decoded.  The setting and the state stay with the slot wherever dabx_set_subchannels says
 * it "keeps decoding without interruption", a move to other capacity units included; a new or changed slot loses them.  A slot with the
 * mode on cannot become a packet-mode slot.  An engine without such a slot allocates and launches nothing for this stage.  Drains the
 * engine. */
int  dabx_set_mp2_audio_mode(dabx_engine *e, int stream, int subch_idx, const dabx_mp2_audio_config *cfg);
/* The newest n frames still in the rings, oldest first: their records into recs[], their PCM back to back into pcm[], 4608 bytes each;
 * byte_pos is rebased to the returned buffer.  When n frames exceed max_bytes the newest that fit are returned (pcm == NULL: records
 * only).  Returns the number of frames.  The rings hold two batches: 64 records, 512 KiB.  Drains the engine. */
int  dabx_read_mp2_audio(dabx_engine *e, int stream, int subch_idx, int n, dabx_mp2_audio_frame *recs, uint8_t *pcm, size_t max_bytes);
int  dabx_get_mp2_audio_stats(dabx_engine *e, int stream, int subch_idx, dabx_mp2_audio_stats *out);
/* The MP2 audio section (DABX_DELIVER_MP2_AUDIO): one dabx_chunk_mp2_audio per (stream, slot) from dabx_chunk_header_ext.off_mp2_audio,
 * all zero for a slot without the mode; behind the table every such slot has room for DABX_CHUNK_FRAMES * 4 records and as many times
 * 4608 bytes -- a logical frame completes at most one MP2 frame -- fixed by the configuration.  Record i's PCM is the 4608 bytes at
 * bytes_off + byte_pos.  Gathered behind the batch's stages like the PAD section. */
typedef struct {
  int64_t  first_frame;      /* number, since the mode was switched on, of the first record in the chunk */
  int32_t  n_frames, frames_lost;
  uint64_t rec_off, bytes_off;
  int64_t  n_bytes;          /* n_frames * 4608 */
  int64_t  decode_calls, frames_out, bad_header, refused, overread;      /* dabx_mp2_audio_stats after the chunk's batch */
  int64_t  sample_rate, voffs, number_of_frames, error_frames;
  int64_t  reserved[2];
} dabx_chunk_mp2_audio;      /* 128 bytes */

/* ------------------------------------------------------------------------------------------------------------
 * AAC stream: the LOAS/LATM stream of a DAB+ audio sub-channel on the device -- the access-unit walk of Mp4Processor::_process_super_frame
 * and _build_aac_stream over BitWriter (base/backend/audio/mp4processor.cpp:320-391, :395-445, bit_writer.cpp:29-59), k_aac_stream: one
 * 64-thread block per slot with the mode on, behind k_dabplus on the MSC batch's stream, beside the PAD stage.  It walks the super
 * frames k_dabplus has completed since the slot's last visit and takes k_dabplus's verdicts (dabx_superframe_info): it re-runs no CRC.
 * Per access unit a = 0 .. num_aus - 1, in order, ONE record:
 *   au_len_bad bit set (:325-331)                   length 0, flags DABX_AAC_LOST_LEN -- where the reference conceals
 *   length good, au_crc_ok bit clear (:377-382)     length 0, flags DABX_AAC_LOST_CRC -- where the reference conceals
 *   otherwise (:333-341)                            one LOAS frame of the L = au_start[a + 1] - au_start[a] - 2 payload bytes at au_start[a]
 * so the records are the reference's sequence of "frame / conceal" events.  The bytes of a slot's frames follow each other without
 * padding, each frame on a byte boundary: what mpFrameBuffer receives (:341, the "AAC dump") and what convert_mp4_to_pcm of the fdk-aac
 * build is handed (:357); written to a file they play in any AAC player.  LOAS because it is the only container that can say "960-sample
 * transform" (ADTS cannot).
 * The frame (:399-441): 11-bit sync word 0x2B7, 13-bit audioMuxLengthBytes = size - 3 (bit_writer.cpp:54-59), StreamMuxConfig with
 *   CoreSrIndex = dac ? (sbr ? 6 : 3) : (sbr ? 8 : 5), CoreChConfig = aacChannelMode ? 2 : 1, ExtensionSrIndex = dac ? 3 : 5
 * (:266-269; psFlag and mpegSurround do not enter), PayloadLengthInfo of L / 255 bytes 0xFF and one byte L % 255, the payload.  The header
 * is 69 bits without SBR and 78 with, so the payload lies 5 / 6 bits off the byte grid and the last byte ends in 3 / 2 zero bits; a frame
 * is 10 + L / 255 + L bytes without SBR, 11 + L / 255 + L with.  L = 0 is legal (one length byte 0, no payload); L runs to 960.
 * Unbounded output: for a super frame whose AU table is in order the access units partition it and each adds at most 12 bytes net, so it
 * emits at most 110 * kbps / 8 + 72 bytes.  A crafted table with starts out of order can hold overlapping access units that each pass
 * their CRC; the reference emits them all, and so does the device: there is no guard.  Such a stream simply emits more bytes; the rings
 * lose oldest-first, counted in `lost` and in the chunk's frames_lost, as the sibling rings do.
 * Parity with the reference's object code is unpinned (mp4processor.cpp needs the GUI's headers): the tests compare the device with a
 * bit-serial, line-cited restatement (tests/aac_stream_cases.py).
 * Out of scope: AAC decoding itself, the raw-AU path of the faad build (:359-364), resampling and playback, the signal_* cadence of
 * :384-389. */
enum { DABX_AAC_LOST_LEN = 1, DABX_AAC_LOST_CRC = 2 };      /* dabx_aac_frame.flags */
#define DABX_AAC_MAX_FRAME_BYTES 974   /* 11 + 960 / 255 + 960 */
typedef struct {
  uint32_t size;             /* sizeof(dabx_aac_stream_config) of the caller */
  int32_t  format;           /* 0: LOAS/LATM; anything else is DABX_E_ARG */
  int32_t  reserved[6];      /* zero */
} dabx_aac_stream_config;    /* 32 bytes */
typedef struct dabx_aac_frame_s {
  int64_t  byte_pos;         /* position of the frame's first byte in the slot's sequence of LOAS bytes */
  int64_t  first_frame;      /* dabx_superframe_info.first_frame of the access unit's super frame */
  uint16_t length;           /* bytes of the LOAS frame; 0 for a lost access unit */
  uint16_t au_len;           /* L; for DABX_AAC_LOST_LEN the 16 low bits of the computed value */
  uint8_t  au, num_aus;      /* the access unit's index in its super frame, and how many that has */
  uint8_t  stream_parms;     /* dabx_superframe_info.stream_parms */
  uint8_t  flags;            /* 0, DABX_AAC_LOST_LEN or DABX_AAC_LOST_CRC */
  uint8_t  reserved[8];
} dabx_aac_frame;            /* 32 bytes, little-endian, no holes */
typedef struct {
  int64_t superframes;       /* super frames walked */
  int64_t records;           /* access units visited = records written */
  int64_t frames;            /* ... of these LOAS frames */
  int64_t frame_bytes;       /* bytes of all LOAS frames */
  int64_t lost_len, lost_crc;      /* records with DABX_AAC_LOST_LEN / DABX_AAC_LOST_CRC */
  int64_t launches;          /* k_aac_stream launches of the engine (the kernel has no row in the profile table) */
  int64_t lost;              /* records that had left the rings before a dabx_read_aac_frames call could return them */
} dabx_aac_stream_stats;     /* 64 bytes */
/* Switches the LOAS framing of slot subch_idx of `stream` on (cfg != NULL) or off (NULL).  On: only an active DAB+ slot (dab_plus == 1)
 * that is not in packet mode, cfg->format 0 and the reserved words 0; DABX_E_ARG otherwise.  A slot that is switched on starts with empty
 * rings and all counts 0; the walk starts with the next super frame completed.  Independent of the slot's PAD and MOT modes.  The
 * setting stays with the slot wherever dabx_set_subchannels says it "keeps decoding without interruption", a move included; a new or
 * changed slot loses it, as it loses PAD decoding.  A slot with the mode on cannot become a packet-mode slot.  An engine without such a
 * slot allocates and launches nothing for this stage.  Drains the engine. */
int  dabx_set_aac_stream_mode(dabx_engine *e, int stream, int subch_idx, const dabx_aac_stream_config *cfg);
/* The newest n records still in the rings, oldest first: into recs[], their LOAS frames back to back into bytes[]; byte_pos is rebased
 * to the returned buffer.  When they exceed max_bytes the newest that fit are returned (bytes == NULL: records only).  Returns the number
 * of records.  The rings hold two batches of in-order super frames: 128 records and the next power of two >= 2 * 6 * (110 * kbps / 8 + 72)
 * bytes.  Drains the engine. */
int  dabx_read_aac_frames(dabx_engine *e, int stream, int subch_idx, int n, dabx_aac_frame *recs, uint8_t *bytes, size_t max_bytes);
int  dabx_get_aac_stream_stats(dabx_engine *e, int stream, int subch_idx, dabx_aac_stream_stats *out);
/* The AAC section (DABX_DELIVER_AAC): one dabx_chunk_aac per (stream, slot) from dabx_chunk_header_ext.off_aac, all zero for a slot
 * without the mode; behind the table every such slot has room for 36 records (a chunk closes at most 6 super frames of at most 6
 * access units) and for 6 * (110 * kbps / 8 + 72) bytes -- enough for every chunk of super frames whose AU tables are in order; of more
 * the newest that fit are delivered and the rest counted in frames_lost.  Record i's frame is the `length` bytes at bytes_off + byte_pos.
 * Gathered behind the batch's stages like the MP2 audio section. */
typedef struct {
  int64_t  first_frame;      /* number, since the mode was switched on, of the first record in the chunk */
  int32_t  n_frames, frames_lost;      /* records in the chunk; records between the previous chunk's and these that were not delivered */
  uint64_t rec_off, bytes_off;
  int64_t  n_bytes;
  int64_t  superframes, records, frames, frame_bytes, lost_len, lost_crc;      /* dabx_aac_stream_stats after the chunk's batch */
  int64_t  reserved[5];
} dabx_chunk_aac;            /* 128 bytes */

/* ------------------------------------------------------------------------------------------------------------
 * The FIC followed on the device (csrc/fig_core.h, k_fig): what dabx_fibdec does with FIG 0/0 .. 0/3 -- walk_fib's decisions bit for bit,
 * both swap rules -- plus the labels of FIG 1/0, 1/1, 1/4 and 1/5 (fib_decoder_fig1.cpp:49-152, fib_decoder.cpp:744-778), one wave per
 * stream behind every decoded frame, with a per-stream database that stays on the device.  A label is filed iff its key is unknown (1/0:
 * the one ensemble label; 1/1: SId16; 1/4: P/D + SCIdS + SId; 1/5: SId32) and its charset is 0, 6 or 15 (charsets.h:50-55); filed are the 16
 * raw bytes, the charset, the character flag field and the identifier.  Charset conversion, the short label and FIG 1/6 stay with the host.
 * A restart (_restart_fib_decoding, fib_decoder.cpp:131-141) clears the labels too.
 * Where it departs from the reference:
 *  - the tables are bounded.  64 sub-channels per configuration are all there can be (6-bit id).  The others are counted guards that a legal
 *    ensemble cannot reach: DABX_FIG_MAX_COMPONENTS service components and DABX_FIG_MAX_PACKETS packet components per configuration,
 *    DABX_FIG_MAX_LABELS labels per kind.  An entry that does not fit is dropped and counted (over_components, over_packets, over_labels);
 *  - a FIG 1 whose label field (16 bytes + the flag field) does not lie inside its own FIG, by the header's length, is dropped and counted
 *    (label_short).  The reference reads on into whatever follows.  Like walk_fib the walk stops at a FIG that runs past byte 30.
 * The events below are lossy notifications, newest kept; the database (dabx_fig_info, _subchannels, _packet_components, _labels, _follow)
 * is the truth. */
#define DABX_FIG_MAX_COMPONENTS 256
#define DABX_FIG_MAX_PACKETS 64
#define DABX_FIG_MAX_LABELS 64
#define DABX_FIG_MAX_EVENTS 256       /* events a stream's ring holds */
typedef struct {
  int32_t enable;             /* 0: off -- the stream's database is dropped, dabx_follow_fic works again */
  int32_t reference_quirks;   /* dabx_fibdec_set_reference_quirks: swap only after change flags 3 */
  int32_t service_info;       /* != 0: the service information of FIG 0/5 .. 0/19 is followed too ("Service information" below); 0: not */
  int32_t reserved[1];
} dabx_fig_config;
enum { DABX_FIG_LABEL_ENSEMBLE = 0, DABX_FIG_LABEL_SERVICE = 1, DABX_FIG_LABEL_COMPONENT = 4, DABX_FIG_LABEL_DATA_SERVICE = 5 };
typedef struct {
  uint32_t id;                /* 1/0: EId, otherwise the SId */
  uint16_t char_flags;        /* CharFlagField */
  uint8_t  kind;              /* the FIG 1 extension: 0, 1, 4, 5 */
  uint8_t  charset;           /* 0 EBU Latin, 6 UCS-2, 15 UTF-8 */
  uint8_t  label[16];         /* as transmitted */
  uint8_t  pd, scids;         /* 1/4 only */
  uint8_t  reserved[6];
} dabx_fig_label;             /* 32 bytes */
enum { DABX_FIG_ANNOUNCE = 1, DABX_FIG_SWAP = 2, DABX_FIG_RESTART = 3, DABX_FIG_TABLE = 4, DABX_FIG_LABEL = 5 };
typedef struct {
  int32_t kind;               /* DABX_FIG_* */
  int32_t epoch;              /* restarts so far (a RESTART event carries the new count) */
  int64_t frame;              /* fib / 12 */
  int64_t fib;                /* index of the FIB within the stream, counted like dabx_fibdec_info.fibs_processed (TABLE: the frame's last) */
  int64_t cif;                /* 4 * (fib / 12) + (fib % 12) / 3 */
  union {
    struct { int32_t flags, occurrence_change; int64_t at_cif; } announce;      /* change flags 0 -> non-zero; at_cif as dabx_follow_fic */
    struct { int32_t n_changes, n_subch, n_components, n_packets; } swap;       /* the new current configuration */
    struct { int32_t next, n_subch, n_components, n_packets; } table;           /* at most one per frame and configuration that gained an entry */
    dabx_fig_label label;                                                       /* a label was filed */
    int32_t words[8];
  } u;
} dabx_fig_event;             /* 64 bytes */
typedef struct {
  int64_t fibs_good, fibs_bad;                   /* FIBs walked / counted and skipped for their CRC */
  int64_t figs, end_markers, fig_overrun;        /* FIGs stepped through; walks ended by 0xFF; by a FIG running past byte 30 */
  int64_t fig_other_type, fig0_other_ext;        /* FIGs of type 2..7; FIG 0 of another extension (or a FIG 0/0 shorter than 5) */
  int64_t fig00;
  int64_t subch_new, subch_known, comp_new, comp_known, packet_new, packet_known;
  int64_t restarts, swaps, announces;
  int64_t over_components, over_packets, over_labels;       /* the guards: entries dropped because the table was full */
  int64_t label_new, label_known, label_charset, label_short, label_other_ext;
  int64_t events;                                /* events written to the ring */
  int64_t launches;                              /* k_fig launches of the engine */
  int64_t reserved[5];
} dabx_fig_stats;             /* 256 bytes */
/* stream -1 = all.  cfg == NULL or enable != 0: on.  A stream that is switched on starts from an empty database with the FIB count of the
 * frames decoded so far, as a dabx_follow_fic decoder would; switching off drops it.  While no stream has the mode on nothing is launched,
 * and an engine that never enables it allocates nothing.  dabx_follow_fic on a stream with the mode on is refused (DABX_E_STATE).  Drains
 * the engine. */
int  dabx_set_fig_mode(dabx_engine *e, int stream, const dabx_fig_config *cfg);
/* The database of a stream with the mode on (DABX_E_STATE otherwise), one device-to-host copy per call.  As dabx_fibdec_get_info,
 * dabx_fibdec_subchannels (with the dab_plus join), dabx_fibdec_packet_components (with the sid join) and dabx_follow_fic (frames_missed
 * is always 0: no frame is skipped); dabx_fig_labels returns every filed label in order of filing. */
int  dabx_fig_info(dabx_engine *e, int stream, dabx_fibdec_info *out);
int  dabx_fig_subchannels(dabx_engine *e, int stream, int next, dabx_subch_desc *out, int max_out);
int  dabx_fig_packet_components(dabx_engine *e, int stream, int next, dabx_packet_component *out, int max_out);
int  dabx_fig_follow(dabx_engine *e, int stream, dabx_reconf *out);
int  dabx_fig_labels(dabx_engine *e, int stream, dabx_fig_label *out, int max_out);
int  dabx_get_fig_stats(dabx_engine *e, int stream, dabx_fig_stats *out);
/* The newest events still in the stream's ring that no earlier call has returned, oldest first, at most max_events; *lost (optional): those
 * that had left the ring.  The rule of dabx_read_tii_events. */
int  dabx_read_fig_events(dabx_engine *e, int stream, int max_events, dabx_fig_event *ev, int32_t *lost);
/* The walk on crafted FIBs, without an engine: n_decoders fresh decoders, one wave each, decoder d walks fibs[d][n_fibs][32] with
 * crc_ok[d][n_fibs].  Every output is optional (NULL) and has a row per decoder: info[d]; n_tab[d][2][3] sizes of (current, next) x
 * (sub-channels, components, packets); subch[d][2][64] and packets[d][2][DABX_FIG_MAX_PACKETS] as the getters return them; n_labels[d] and
 * labels[d][4 * DABX_FIG_MAX_LABELS]; stats[d]; n_events[d] = events written, events[d][DABX_FIG_MAX_EVENTS] the newest of them, oldest first. */
int  dabx_fig_walk_device(const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, int reference_quirks, dabx_fibdec_info *info,
                          int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets, int32_t *n_labels, dabx_fig_label *labels,
                          dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events);

/* ------------------------------------------------------------------------------------------------------------
 * Service information (csrc/fig_si_core.h; dabx_fig_config.service_info): the FIG 0 extensions behind 0/3 that the reference decodes
 * (fib_decoder_fig0.cpp:333-720) -- 0/5 component language, 0/7 configuration information, 0/8 component global definition, 0/9 country / LTO,
 * 0/10 date and time, 0/13 user applications, 0/14 FEC scheme, 0/17 programme type, 0/18 announcement support, 0/19 announcement switching --
 * walked by the same wave at the point where the walk counts fig0_other_ext (which it still does), and the join of all tables into one
 * record per service component (dabx_fig_directory; fib_decoder.cpp:219-290, :351-460).  With service_info = 0 nothing of this exists.
 * Where the tables live, as in the reference: 0/7, 0/8, 0/13, 0/14 and the clusters of 0/18 / 0/19 in the configuration the C/N flag selects
 * (_get_config_ptr); 0/5, 0/9 and 0/17 in the current one; the time of 0/10 in scalars.  Its decisions, line for line:
 *  - the first description of a key wins (0/5 :346/:366, 0/7 :392, 0/8 :435, 0/14 :569, 0/17 :596); FIG 0/9 is read once (:456);
 *  - FIG 0/5's long form asks "known?" through a getter whose argument is 8 bits wide (fib_config_fig0.h:242): a component with SCId >= 256
 *    is never known and filed again by every repetition (until the cap below);
 *  - FIG 0/13 looks its key up in the CURRENT configuration and files into the C/N one (:525, :547): with C/N = 1 every repetition files
 *    again.  A known entry is stepped over by its stored SizeBits (:554).  NumUserApps is clamped to 6 (:532-536); the cursor then stands
 *    inside the 7th application, stays there (ua_clamped) and what follows is read as the next entry;
 *  - FIG 0/17 steps by 32 bits whatever its flags say, while offset < length * 8 (:590-611);
 *  - FIG 0/18 reads a 16-bit SId whatever P/D says (:626); cluster id 0 is skipped (:635); _get_cluster (fib_decoder.cpp:722-742) searches
 *    64 entries, takes the first free one for an unknown id and falls back to entry 0 when all are in use; _set_cluster overwrites the
 *    flags and appends the SId if the cluster does not list it (:707-719);
 *  - FIG 0/19 (:658-719): a cluster whose flags meet the ASw flags counts up, and announces the start when the count reaches 5; one that
 *    counted and no longer meets them is set back to 0 and announces the stop.  An unknown cluster id gets an entry of its own here too,
 *    with flags 0 (asw_unknown): _get_cluster never returns the null pointer that :686-689 leaves the FIG for;
 *  - FIG 0/10 overwrites the time with every FIG (:491-506) and reports it iff a FIG 0/9 is filed (:508-513).
 * A swap follows the configuration's: under reference_quirks the object that becomes current brings only what was filed into it, so 0/5,
 * 0/9 and 0/17 are gone after it; under the default rule every SI table the announcement never filled is carried over, 0/5, 0/9 and 0/17
 * always.  A restart clears every table and the time.
 * Where it departs from the reference (all of it is here):
 *  - the tables are bounded: DABX_FIG_MAX_GLOBAL_DEFS (one per service component), DABX_FIG_MAX_USER_APPS (64 packet components + 64
 *    sub-channels with X-PAD applications), DABX_FIG_MAX_LANGUAGES (64 sub-channels + 64 packet components), DABX_FIG_MAX_PTYS (FIG 0/7
 *    counts at most 63 services), 64 FEC entries and 64 clusters (all there can be), DABX_FIG_MAX_CLUSTER_SIDS (cluster, SId) pairs in all
 *    (63 services x 7 clusters of a FIG 0/18 entry = 441).  What does not fit is dropped and counted: over_global_defs, over_user_apps,
 *    over_languages, over_ptys, over_cluster_sids;
 *  - an entry whose fields do not lie inside its own FIG, by the header's length, ends that FIG's walk and is counted (outside).  The
 *    reference reads on into whatever follows;
 *  - no timer gate: mFibLoadingState, which keeps _set_cluster and FIG 0/19 closed until Qt timers have run out (:679,
 *    fib_decoder.cpp:695), has no counterpart; both are evaluated from the first FIB;
 *  - of a user application the type, the data length and the first four data bytes are kept (an X-PAD application has its XPadAppTy and
 *    DSCTy there); the reference keeps type and length;
 *  - an announcement's start and stop are ONE event per cluster, with the number of SIds the cluster lists in n_services -- also when it
 *    lists none (a cluster that FIG 0/19 itself made, or entry 0 answering for an id that found no room).  The reference signals once per
 *    listed SId (:697-716) and so not at all for such a cluster: a host that wants its behaviour drops events with n_services 0;
 *  - a reset (restart; the next configuration after a swap) clears the cluster table too; FibConfigFig0::reset leaves it;
 *  - the directory gives a secondary audio component its SCIdS from the short-form FIG 0/8 entry of (SId, SubChId) and its FIG 1/4 label
 *    through that; the reference lists primary audio components only. */
#define DABX_FIG_MAX_GLOBAL_DEFS 256
#define DABX_FIG_MAX_USER_APPS 128
#define DABX_FIG_MAX_LANGUAGES 128
#define DABX_FIG_MAX_PTYS 128
#define DABX_FIG_MAX_CLUSTERS 64
#define DABX_FIG_MAX_CLUSTER_SIDS 512
#define DABX_FIG_CLUSTER_LIST 24      /* SIds a dabx_fig_cluster lists */
enum { DABX_FIG_SI_TABLE = 6, DABX_FIG_TIME = 7, DABX_FIG_ANNOUNCE_START = 8, DABX_FIG_ANNOUNCE_STOP = 9 };
/* Payloads of the SI events, in dabx_fig_event.u.words (they are written for a stream with service_info on only):
 *  SI_TABLE        at the frame's end, per configuration that gained an SI entry in it: next, mask of DABX_FIG_SI_HAS_*, then the sizes of
 *                  its 0/8, 0/13, 0/14, cluster and (cluster, SId) tables, and n_languages | n_ptys << 16 (current configuration only);
 *  TIME            mjd, hour, minute, second (-1: short form), lto_minutes, utc_flag, lsi;
 *  ANNOUNCE_START / _STOP   cluster id, ASw flags, SubChId, services in the cluster, next (the C/N flag). */
enum { DABX_FIG_SI_HAS_LANGUAGE = 1, DABX_FIG_SI_HAS_CONFIG = 2, DABX_FIG_SI_HAS_GLOBAL_DEF = 4, DABX_FIG_SI_HAS_LTO = 8, DABX_FIG_SI_HAS_USER_APPS = 16,
       DABX_FIG_SI_HAS_FEC = 32, DABX_FIG_SI_HAS_PTY = 64, DABX_FIG_SI_HAS_CLUSTER = 128 };
typedef struct {
  int32_t has_config[2], n_services[2], count[2];          /* FIG 0/7 of (current, next) */
  int32_t has_lto, lto_minutes, ecc, inter_table, lto_ext;  /* FIG 0/9: Ensemble LTO * 30, ECC, InterTableId, Ext flag */
  int32_t time_set, mjd, hour, minute, second, lsi, utc_flag;   /* FIG 0/10, the newest; second -1: short form */
  int32_t n_global_defs[2], n_user_apps[2], n_fec[2], n_clusters[2], n_cluster_sids[2];
  int32_t n_languages, n_ptys;
  int32_t reserved[2];
} dabx_fig_si_scalars;          /* 128 bytes */
typedef struct {
  uint32_t sid;
  int8_t   scids, pd, ls, ext;
  int16_t  subch_id, scid;    /* short form: the sub-channel (scid -1); long form: the SCId (subch_id -1) */
} dabx_fig_global_def;        /* 12 bytes */
typedef struct {
  uint32_t sid;
  uint16_t size_bits;         /* SizeBits: the entry's length behind the FIG's cursor */
  uint8_t  scids, pd;
  uint8_t  n_apps, len[6], reserved0;        /* UserAppDataLength of each */
  uint16_t type[6];           /* UserAppType */
  uint8_t  data[6][4];        /* the first four bytes of each application's data, 0 where there are fewer */
  uint8_t  reserved[12];
} dabx_fig_user_apps_entry;   /* 64 bytes */
typedef struct { int32_t ls, id, language, reserved; } dabx_fig_language;           /* ls 0: id = SubChId, 1: id = SCId */
typedef struct { uint32_t sid; int32_t sd, code, reserved; } dabx_fig_programme_type;
typedef struct { int32_t subch_id, scheme; } dabx_fig_fec_scheme;
typedef struct {
  int32_t cluster_id, flags, announcing, n_services;       /* ASu flags; the FIG 0/19 count; SIds filed */
  uint32_t sid[DABX_FIG_CLUSTER_LIST];                      /* the first of them, in order of filing */
  int32_t reserved[4];
} dabx_fig_cluster;           /* 128 bytes */
typedef struct {
  int64_t si_figs;                               /* FIG 0 of an extension the SI walk knows */
  int64_t language_new, language_known, config_new, config_known, global_def_new, global_def_known, lto_new, lto_known;
  int64_t time_set;                              /* FIG 0/10 read */
  int64_t user_apps_new, user_apps_known, user_apps_clamped, fec_new, fec_known, pty_new, pty_known;
  int64_t cluster_new, cluster_fallback, cluster_zero, cluster_sid_new, cluster_sid_known;
  int64_t asw_count, asw_start, asw_stop, asw_unknown;
  int64_t over_global_defs, over_user_apps, over_languages, over_ptys, over_cluster_sids;        /* the guards: dropped, table full */
  int64_t outside;                               /* the guard: walks ended by an entry that does not lie inside its FIG */
} dabx_fig_si_stats;          /* 256 bytes */
enum { DABX_FIG_JOIN_SUBCH = 1, DABX_FIG_JOIN_PACKET = 2, DABX_FIG_JOIN_GLOBAL_DEF = 4, DABX_FIG_JOIN_USER_APPS = 8, DABX_FIG_JOIN_FEC = 16,
       DABX_FIG_JOIN_LANGUAGE = 32, DABX_FIG_JOIN_PTY = 64, DABX_FIG_JOIN_LABEL = 128 };
/* One service component with everything the tables say about it.  -1: not known (the look-up that gives it did not succeed). */
typedef struct {
  uint32_t sid;
  int8_t   comp_idx, ps, tmid, ty;      /* index within its FIG 0/2 service; P/S; TMId; ASCTy (TMId 0) or DSCTy (TMId 1: FIG 0/2, TMId 3: FIG 0/3) */
  int8_t   scids, subch_id, prot_level, short_form;
  int16_t  cu_start, cu_size, kbps, packet_address;
  int16_t  scid, language;
  int8_t   pty, fec_scheme, dg_flag, pd;            /* fec_scheme 0 without a FIG 0/14 (fib_decoder.cpp:408); pd: the P/D flag of its FIG 0/2 */
  uint8_t  n_apps, app_len[6], reserved0;
  uint16_t app_type[6];
  uint8_t  app_data[6][4];
  dabx_fig_label label;                 /* kind 0xFF: none */
  uint32_t joined;                      /* DABX_FIG_JOIN_* */
  int32_t  reference_defined;           /* what _get_data_for_audio_service / _get_data_for_packet_service returns for it (TMId 1: 0) */
  int32_t  reserved[4];
} dabx_fig_service;           /* 128 bytes */
/* The SI database of a stream with service_info on (DABX_E_STATE otherwise), one device-to-host copy per call; next: the configuration. */
int  dabx_fig_si_info(dabx_engine *e, int stream, dabx_fig_si_scalars *out);
int  dabx_fig_user_apps(dabx_engine *e, int stream, int next, dabx_fig_user_apps_entry *out, int max_out);
int  dabx_fig_global_defs(dabx_engine *e, int stream, int next, dabx_fig_global_def *out, int max_out);
int  dabx_fig_languages(dabx_engine *e, int stream, dabx_fig_language *out, int max_out);
int  dabx_fig_programme_types(dabx_engine *e, int stream, dabx_fig_programme_type *out, int max_out);
int  dabx_fig_fec_schemes(dabx_engine *e, int stream, int next, dabx_fig_fec_scheme *out, int max_out);
int  dabx_fig_clusters(dabx_engine *e, int stream, int next, dabx_fig_cluster *out, int max_out);
int  dabx_get_fig_si_stats(dabx_engine *e, int stream, dabx_fig_si_stats *out);
/* The service directory: one launch (k_fig_directory: a wave per stream, a lane per service component of the chosen configuration) and one
 * copy.  stream >= 0: out[max_per_stream], n_out[1]; stream -1: out[n_streams][max_per_stream], n_out[n_streams] (a stream without
 * service_info: n_out 0).  Records in the component table's filing order; n_out counts the components, of which min(n_out, max_per_stream)
 * are written.  The joins are fib_decoder.cpp's: audio :219-290 (a 32-bit SId is refused: reference_defined 0), packet :351-460 (the first
 * long-form FIG 0/8 of the SId whatever its SCId, :379; language through the 8-bit getter).  Charset conversion and the short label stay
 * with the host.  Returns 0. */
int  dabx_fig_directory(dabx_engine *e, int stream, int next, dabx_fig_service *out, int max_per_stream, int32_t *n_out);
/* dabx_fig_walk_device with the service information on: the outputs of that entry, then per decoder si_info[d], si_stats[d],
 * global_defs[d][2][DABX_FIG_MAX_GLOBAL_DEFS], user_apps[d][2][DABX_FIG_MAX_USER_APPS], fec[d][2][64], clusters[d][2][64],
 * languages[d][DABX_FIG_MAX_LANGUAGES], ptys[d][DABX_FIG_MAX_PTYS], and the directory of both configurations: n_dir[d][2],
 * dir[d][2][DABX_FIG_MAX_COMPONENTS].  Every output is optional. */
int  dabx_fig_si_walk_device(const uint8_t *fibs, const uint8_t *crc_ok, int n_decoders, int n_fibs, int reference_quirks, dabx_fibdec_info *info,
                             int32_t *n_tab, dabx_subch_desc *subch, dabx_packet_component *packets, int32_t *n_labels, dabx_fig_label *labels,
                             dabx_fig_stats *stats, int64_t *n_events, dabx_fig_event *events, dabx_fig_si_scalars *si_info, dabx_fig_si_stats *si_stats,
                             dabx_fig_global_def *global_defs, dabx_fig_user_apps_entry *user_apps, dabx_fig_fec_scheme *fec, dabx_fig_cluster *clusters,
                             dabx_fig_language *languages, dabx_fig_programme_type *ptys, int32_t *n_dir, dabx_fig_service *dir);

#ifdef __cplusplus
}
#endif
#endif
