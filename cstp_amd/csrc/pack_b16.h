// The bf16-storage path's weight pack (b16.hip) as a device function, shared with the replay kernel of igemm.hip (cstp_pack_replay,
// record kind 4): fp32 [kout][cin][taps] -> bf16 GEMM operand rows
//   forward:        wp[m = kout (Mp rows)][k = tap * ip + c   (Kw, zero beyond taps * ip)]
//   data gradient:  wp[m = cin  (Mp rows)][k = tap * ip + ko]
// ip = the reduction's channel count (cin / kout), or that count rounded up to 16 when it is not a multiple of 16 (the gather
// then covers the last, partial 16-channel group: the padded k carry zero weights)
#pragma once
#include "common.h"

namespace cstp {

__device__ __forceinline__ void pack_w_b16_body(const float* __restrict__ w, unsigned short* __restrict__ wp, int kout, int cin, int ntaps,
                                                int Mp, int Kw, int dgrad, int ip, int blk, int nblk) {
  const size_t total = (size_t)Mp * Kw;
  const int inner = dgrad ? kout : cin, mreal = dgrad ? cin : kout;
  for (size_t i = (size_t)blk * 256 + threadIdx.x; i < total; i += (size_t)nblk * 256) {
    const int k = (int)(i % Kw), m = (int)(i / Kw);
    const int tap = k / ip, c = k - tap * ip;
    float v = 0.f;
    if (m < mreal && tap < ntaps && c < inner) v = dgrad ? w[((size_t)c * cin + m) * ntaps + tap] : w[((size_t)m * cin + c) * ntaps + tap];
    wp[i] = f2bf(v);
  }
}

// the pack-plan hooks of igemm.hip (cstp_pack_mode / cstp_pack_register): true = the caller has replayed this workspace's pack
bool pack_skip(const void* dst);
// the bf16 pack site: true = skip this launch (it equals the record replayed into dst); mode 1 appends it to the record list
bool pack_site_b16(const float* w, void* dst, int nblocks, int kout, int cin, int ntaps, int Mp, int Kw, int dgrad, int ip);
// something other than a recorded pack is about to be written into ws: it no longer holds a replayed pack
void pack_clobbered(const void* ws);

}  // namespace cstp
