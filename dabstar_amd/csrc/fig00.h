// fig00.h -- the CIF counter a FIB's FIG 0/0 carries: ONE walk for the device (k_fic_frame -> dabx_stats.cif_count, the TII decision of
// k_frame_tail) and the host (dabx_read_eti -> the ETI frames' counter), so that the two can never tell different counters for one FIB.
//
// The rule is the reference's (FibDecoder::process_FIB, fib_decoder.cpp:74-100, and _process_Fig0s0, fib_decoder_fig0.cpp:95-101): FIG after
// FIG by the header's length field, stopped by the end marker 0xFF only; every FIG of type 0 whose second byte has extension 0 is a FIG 0/0,
// whatever its length field says, and its counter is read from the bytes 4 and 5 behind its header -- no length is checked anywhere, a FIG
// 0/0 "of length 0" still sets the counter from the bytes of the FIGs behind it, and the last FIG 0/0 of the FIB wins.  With the header
// at byte 25 or 26 the counter comes out of the FIB's two CRC bytes, as it does in the reference.
//
// Where it stops following the reference: a FIG 0/0 header at byte 27, 28 or 29 is ignored.  The reference reads bits of whatever lies
// behind the FIB in its buffer there (the next FIB of the block, the previous frame's bits, or past the buffer for FIB 11), which is
// nothing a receiver could rely on.  Its break after a FIG 0/1 with impossible content (mRestartFibDecoding) is not modelled either.
// dabx_fibdec (walk_fib, fib.cpp) walks more strictly: it stops at a FIG that runs past byte 30 and takes a FIG 0/0 of length >= 5 only.
#pragma once
#include <stdint.h>

namespace dabx {

// b: the FIB's 32 bytes (30 data + CRC; the caller has checked the CRC).  Returns whether the FIB carries a FIG 0/0; *hi / *lo (CIFCountHi,
// 0..31, and CIFCountLo, 0..255) are written only then.  The counter is hi * 250 + lo.
__host__ __device__ inline bool fib_fig00_counter(const uint8_t *b, int *hi, int *lo)
{
  bool found = false;
  int p = 0;
  while (p < 30) {
    const int type = b[p] >> 5, len = b[p] & 0x1F;
    if (type == 7 && len == 0x1F) break;
    if (type == 0 && p + 5 < 32 && (b[p + 1] & 0x1F) == 0) { *hi = b[p + 4] & 0x1F; *lo = b[p + 5]; found = true; }
    p += len + 1;
  }
  return found;
}

}  // namespace dabx
