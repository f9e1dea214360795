// iqfile.h -- internal: recorded-IQ decode/resample launchers (iqfile.hip) and the engine hooks they need.
#pragma once
#include "dabx_internal.h"

namespace dabx {

struct IqDecode {      // by-value kernel argument
  int family, container, big_endian, swap_iq;
  int bytes;           // per channel
  float int_scale;     // 1 / 2^(bits-1) for the integer containers
  // reference_quirks (UFF int24 / MSB only): samples per read block of the reference's reader (rate / 1000), 0 = off --
  // Q's middle byte comes from byte 4 i + 4 of the block (xml_reader.cpp:316,462); sign7f: QI ORs 0x7F000000 (:465,:469)
  int quirk_block, quirk_i24, quirk_sign7f;   // quirk_block != 0: the feed hands over whole read blocks only
  // What the destination holds (ring_fmt.h): RING_CF32 -- float2, the decoded value; RING_S16 / RING_U8 -- a native IQ ring, `dst` is its
  // untyped base and the payload's codes are stored as they are (int16: in machine byte order, I first).  Set by iq_native_ring only,
  // which admits just the containers whose codes ARE the ring's.
  int ring_fmt;
};
// iqfile.cpp: format check and the readers' interpolation tables (wav_reader.cpp:67-82, xml_reader.cpp:237-244), shared with the bulk ingest
int iq_check_format(const dabx_iq_format *f, IqDecode *d);
// d (from iq_check_format) is to feed a ring of ring_fmt: sets d->ring_fmt, or refuses (DABX_E_ARG, message with the format and the ring) what
// cannot be stored exactly as that ring's codes -- another rate (the interpolation makes floats), reference_quirks, another container
int iq_native_ring(const dabx_iq_format *f, IqDecode *d, int ring_fmt);
void iq_resample_tables(int family, int rate, int *M, int16_t *tab_int /* [2048] */, float *tab_frac /* [2048] */);

// The three formats of dabx_push_iq / dabx_ingest_config.fmt as decode records for a ring of ring_fmt (which ring_takes, engine.cpp, has admitted):
// 0 cf32 -> WAV / float32, 1 int16 -> WAV / int16, 2 uint8 -> RAW / uint8, all little-endian at 2.048 MS/s
int iq_push_decode(int fmt, int ring_fmt, IqDecode *d);

// THE way IQ samples get into a ring (iqfile.hip): one job is `n` samples of one payload for one destination.  Pushes, the file feed and
// dabx_convert_iq_bytes hand one over by value; a bulk-ingest commit uploads one per stream, in front of the kernels that read them.
struct IqJob {
  unsigned long long src_off;     // byte offset of the payload in IqIo::src: on a sample boundary of the allocation
  unsigned long long dst0;        // index of the first sample written (a ring: the absolute index, i.e. the committed count's host mirror)
  unsigned n;                     // complete input samples (0: the stream takes no part)
  unsigned carry_n;               // samples carried over from the previous job (resampling: <= M + 1)
  unsigned M;                     // input samples per millisecond (rate / 1000); 0: the payload is at 2.048 MS/s, no resampling
  unsigned blocks;                // 1-ms blocks this job resamples, 2048 output samples each  } iq_plan
  unsigned keep;                  // samples of [carry | decoded] kept for the next job        }
  unsigned tab;                   // index of the interpolation tables
  IqDecode dec;
};
// blocks, keep of a job from its carry_n, n, M; returns the samples it produces.  Block c reads V[c M .. c M + M] of V = [carry | decoded]
inline unsigned iq_plan(IqJob *j)
{
  j->blocks = j->keep = 0;
  if (!j->M) return j->n;
  const unsigned len = j->carry_n + j->n;
  j->blocks = len ? (len - 1) / j->M : 0;
  j->keep = len - j->blocks * j->M;            // 1 .. M samples (0 only before the first WAV sample)
  return j->blocks * 2048;
}
struct IqIo {                     // by-value kernel argument: what the jobs of one launch share.  Stream s (0 for a job by value) has row s of each
  const uint8_t *src;
  void *dst; int dst_len;         // [S][dst_len] elements of the jobs' dec.ring_fmt, written at (dst0 + i) % dst_len; dst_len 0: a linear buffer
  float2 *work; size_t work_pitch;    // [S][work_pitch] carry + decoded samples of a resampling job
  float2 *carry; size_t carry_pitch;  // [S][carry_pitch]
  const int16_t *tab_int; const float *tab_frac;   // [n_tabs][2048]
};
int launch_iq_job(const IqIo &io, const IqJob &j, hipStream_t st);
// jobs_dev [n_streams]; max_n / max_out: the largest n / blocks * 2048 among them; resamples: some job has M and n
int launch_iq_jobs(const IqIo &io, const IqJob *jobs_dev, int n_streams, unsigned max_n, unsigned max_out, bool resamples, hipStream_t st);
int launch_commit_counts(unsigned long long *wr, const unsigned *counts_dev, int n_streams, hipStream_t st);
}  // namespace dabx

// Head of every dabx_engine (engine.h: its first base): what this file's host side reads of an engine without calling into it
namespace dabx { struct EngineHead { int32_t ring_fmt = 0; }; }
extern "C" int dabx_internal_commit(dabx_engine *e, int stream, size_t n);   // commit of samples iqfile.cpp wrote itself (announces them first)
extern "C" int dabx_internal_ring_info(dabx_engine *e, int stream, float2 **ring, int *ring_len, unsigned long long *wr,
                                        unsigned long long *rd, hipStream_t *st);
