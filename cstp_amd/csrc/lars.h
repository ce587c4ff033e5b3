// LARS over the flat parameter arenas (cstp_lars_ratio / cstp_lars_step, spec in include/cstp_hip.h).
//
// What SGD and Adam do not need: a reduction PER TENSOR, over an arena whose ~170 tensors run from one float to millions, in a
// fixed number of launches and without a host read.  The host deals every trainable tensor's padded extent out in CHUNKS of at
// most CSTP_LARS_CHUNK floats (a chunk never crosses a tensor; its offset and length are multiples of 4 because tensors start on
// 16-byte boundaries and are zero-padded to four floats) and describes them in two int32 tables:
//   chunks [n_chunks][3] = {segment, offset, length}          offsets in floats from the arena base
//   segs   [n_segs][3]   = {first chunk, chunk count, adapted} a segment is one tensor; its chunks are consecutive
// One block owns one chunk, so a 2.4 M-float convolution weight is ~590 blocks and a 64-float BatchNorm vector is one small one.
//   1. lars_partial_kernel  block -> (sum p^2, sum (c g + wd p)^2) of its chunk, in double, stored at ws[2 * chunk ..]
//   2. lars_fold_kernel     one block per segment sums its chunks' partials in a fixed order and forms q
//   3. lars_update_kernel   block -> the update of its chunk with its segment's q
// No atomics anywhere: every partial has one writer and every sum one fixed order, so equal inputs give equal bits.
// The padding floats are zero in p, g and buf and stay zero: 0 * c = 0, q * (0 + wd * 0) = 0, momentum * 0 + 0 = 0, 0 - lr * 0 = 0.
// The tables come from the host but live on the device, so the entry points cannot check them; every kernel checks the entries it
// uses against the arena length and the table sizes and leaves a malformed one alone instead of following it out of bounds.
#pragma once
#include <math.h>

#include "common.h"

namespace cstp {

constexpr int LARS_THREADS = 256;
static_assert(CSTP_LARS_CHUNK % (4 * LARS_THREADS) == 0, "a full chunk is a whole number of float4 per thread");

struct LarsChunk { int seg, off, len; };

// The chunk of this block, or len = 0 when the entry does not describe floats of the arena.
__device__ __forceinline__ LarsChunk lars_chunk(const int32_t* __restrict__ chunks, int n_segs, size_t n) {
  LarsChunk c;
  c.seg = chunks[3 * blockIdx.x];
  c.off = chunks[3 * blockIdx.x + 1];
  c.len = chunks[3 * blockIdx.x + 2];
  const bool ok = c.seg >= 0 && c.seg < n_segs && c.off >= 0 && c.len > 0 && c.len <= CSTP_LARS_CHUNK && ((c.off | c.len) & 3) == 0 &&
                  (size_t)c.off + (size_t)c.len <= n;
  if (!ok) c.len = 0;
  return c;
}

// g' + wd p on the clipped gradient g' = c g: the same fp32 expression in the norm and in the update
__device__ __forceinline__ float lars_d(float gc, float p, float wd) { return fmaf(wd, p, gc); }

__global__ void __launch_bounds__(LARS_THREADS)
lars_partial_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t n, const int32_t* __restrict__ chunks,
                    const int32_t* __restrict__ segs, int n_segs, float wd, const float* __restrict__ coef_p,
                    double* __restrict__ part) {
  __shared__ double sm[16];
  const LarsChunk c = lars_chunk(chunks, n_segs, n);
  double a = 0.0, b = 0.0;
  if (c.len > 0 && segs[3 * c.seg + 2] != 0) {      // block-uniform: tensors that are not adapted are not read here at all
    const float coef = coef_p != nullptr ? coef_p[0] : 1.f;
    const float4* p4 = reinterpret_cast<const float4*>(p + c.off);
    const float4* g4 = reinterpret_cast<const float4*>(g + c.off);
    const int n4 = c.len >> 2;
#pragma unroll
    for (int k = 0; k < CSTP_LARS_CHUNK / (4 * LARS_THREADS); ++k) {
      const int i = k * LARS_THREADS + threadIdx.x;
      if (i < n4) {
        const float4 pv = p4[i], gv = g4[i];
        const float dx = lars_d(gv.x * coef, pv.x, wd), dy = lars_d(gv.y * coef, pv.y, wd);
        const float dz = lars_d(gv.z * coef, pv.z, wd), dw = lars_d(gv.w * coef, pv.w, wd);
        a += (double)pv.x * pv.x + (double)pv.y * pv.y + (double)pv.z * pv.z + (double)pv.w * pv.w;
        b += (double)dx * dx + (double)dy * dy + (double)dz * dz + (double)dw * dw;
      }
    }
  }
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  if (threadIdx.x == 0) { part[2 * (size_t)blockIdx.x] = a; part[2 * (size_t)blockIdx.x + 1] = b; }
}

__global__ void __launch_bounds__(LARS_THREADS)
lars_fold_kernel(const double* __restrict__ part, const int32_t* __restrict__ segs, int n_chunks, float eta,
                 float* __restrict__ ratio) {
  __shared__ double sm[16];
  const int first = segs[3 * blockIdx.x], count = segs[3 * blockIdx.x + 1], adapted = segs[3 * blockIdx.x + 2];
  double a = 0.0, b = 0.0;
  if (adapted != 0 && first >= 0 && count > 0 && count <= n_chunks - first)
    for (int i = threadIdx.x; i < count; i += LARS_THREADS) { a += part[2 * (size_t)(first + i)]; b += part[2 * (size_t)(first + i) + 1]; }
  a = block_sum(a, sm);
  b = block_sum(b, sm);
  if (threadIdx.x == 0) {
    float q = 1.f;
    if (adapted != 0 && a > 0.0 && b > 0.0) q = (float)((double)eta * sqrt(a) / sqrt(b));
    ratio[blockIdx.x] = q;
  }
}

__global__ void __launch_bounds__(LARS_THREADS)
lars_update_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, size_t n,
                   const int32_t* __restrict__ chunks, const int32_t* __restrict__ segs, int n_segs,
                   const float* __restrict__ ratio, const float* __restrict__ lr_p, float momentum, float wd,
                   const float* __restrict__ coef_p, int write_back) {
  const LarsChunk c = lars_chunk(chunks, n_segs, n);
  if (c.len == 0) return;
  const bool adapted = segs[3 * c.seg + 2] != 0;
  const float q = adapted ? ratio[c.seg] : 1.f;
  const float wde = adapted ? wd : 0.f;             // biases and BatchNorm parameters: no decay, no adaptation (q = 1, + 0 * p)
  const float lr = lr_p[0];
  const float coef = coef_p != nullptr ? coef_p[0] : 1.f;
  float4* p4 = reinterpret_cast<float4*>(p + c.off);
  float4* g4 = reinterpret_cast<float4*>(g + c.off);
  float4* b4 = reinterpret_cast<float4*>(buf + c.off);
  const int n4 = c.len >> 2;
#pragma unroll
  for (int k = 0; k < CSTP_LARS_CHUNK / (4 * LARS_THREADS); ++k) {
    const int i = k * LARS_THREADS + threadIdx.x;
    if (i < n4) {
      float4 pv = p4[i], gv = g4[i], bv = b4[i];
      gv.x *= coef; gv.y *= coef; gv.z *= coef; gv.w *= coef;
      bv.x = fmaf(momentum, bv.x, q * lars_d(gv.x, pv.x, wde)); bv.y = fmaf(momentum, bv.y, q * lars_d(gv.y, pv.y, wde));
      bv.z = fmaf(momentum, bv.z, q * lars_d(gv.z, pv.z, wde)); bv.w = fmaf(momentum, bv.w, q * lars_d(gv.w, pv.w, wde));
      pv.x = fmaf(-lr, bv.x, pv.x); pv.y = fmaf(-lr, bv.y, pv.y); pv.z = fmaf(-lr, bv.z, pv.z); pv.w = fmaf(-lr, bv.w, pv.w);
      if (write_back) g4[i] = gv;
      b4[i] = bv;
      p4[i] = pv;
    }
  }
}

inline bool lars_aligned(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

}  // namespace cstp

extern "C" int cstp_lars_chunk(void) { return CSTP_LARS_CHUNK; }

extern "C" size_t cstp_lars_workspace_bytes(int32_t n_chunks) {
  return n_chunks > 0 ? (size_t)n_chunks * 2 * sizeof(double) : 0;
}

extern "C" int cstp_lars_ratio(void* stream, const float* p, const float* g, size_t n, const int32_t* chunks, int32_t n_chunks,
                               const int32_t* segs, int32_t n_segs, float weight_decay, float eta, const float* coef,
                               float* ratio, void* ws, size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(p && g && chunks && segs && ratio && ws, "null argument");
  CSTP_REQUIRE(n_chunks > 0 && n_segs > 0 && n_segs <= n_chunks, "bad table size");
  CSTP_REQUIRE(n > 0 && n < ((size_t)1 << 31), "arena must hold 1 .. 2^31 - 1 floats (offsets are int32)");
  CSTP_REQUIRE(ws_bytes >= cstp_lars_workspace_bytes(n_chunks), "workspace too small");
  CSTP_REQUIRE(lars_aligned(p) && lars_aligned(g) && lars_aligned(ws), "arenas must be 16-byte aligned");
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(lars_partial_kernel, dim3(n_chunks), dim3(LARS_THREADS), 0, as_stream(stream), p, g, n, chunks, segs, n_segs,
                     weight_decay, coef, part);
  hipLaunchKernelGGL(lars_fold_kernel, dim3(n_segs), dim3(LARS_THREADS), 0, as_stream(stream), part, segs, n_chunks, eta, ratio);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_lars_step(void* stream, float* p, float* g, float* buf, size_t n, const int32_t* chunks, int32_t n_chunks,
                              const int32_t* segs, int32_t n_segs, const float* ratio, const float* lr, float momentum,
                              float weight_decay, const float* coef, int32_t write_back_grad) {
  using namespace cstp;
  CSTP_REQUIRE(p && g && buf && chunks && segs && ratio && lr, "null argument");
  CSTP_REQUIRE(n_chunks > 0 && n_segs > 0 && n_segs <= n_chunks, "bad table size");
  CSTP_REQUIRE(n > 0 && n < ((size_t)1 << 31), "arena must hold 1 .. 2^31 - 1 floats (offsets are int32)");
  CSTP_REQUIRE(lars_aligned(p) && lars_aligned(g) && lars_aligned(buf), "arenas must be 16-byte aligned");
  hipLaunchKernelGGL(lars_update_kernel, dim3(n_chunks), dim3(LARS_THREADS), 0, as_stream(stream), p, g, buf, n, chunks, segs,
                     n_segs, ratio, lr, momentum, weight_decay, coef, write_back_grad);
  CSTP_LAUNCH_CHECK();
  return 0;
}
