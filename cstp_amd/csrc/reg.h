// Fine-tuning regularisers: dropout with a counter-based mask and the stochastic-depth residual join
// (cstp_dropout, cstp_droppath_add_relu_forward / _backward; spec in include/cstp_hip.h).
//
// Dropout.  The mask is a pure function of (seed, offset, element index): element e takes word e & 3 of
// Philox4x32-10(counter = (e >> 2, offset), key = seed), so no mask tensor exists, the backward pass is the same call on dy, and a
// resumed run reproduces it.  A thread owns one GROUP of four consecutive elements and evaluates Philox once for it; where x and
// y are 16-byte aligned a full group travels as one float4, otherwise (the last, partial group; views that start off a 16-byte
// boundary) the same thread handles its elements one by one -- the same words, the same comparison, the same product: equal bits.
//
// Drop-path.  y[b][i] = relu(scale[b] * z[b][i] + res[b][i]) over rows of `row` elements: grid.y walks the samples, so the
// sample index is never divided out of a 64-bit element index; grid.x strides through the row in 16-byte pieces (4 floats / 8
// bf16) when the row length and the pointers allow, element by element otherwise.  bf16 storage computes in fp32 and rounds to
// nearest even.  The optional fp32 absmax by-product is one atomicMax per block into a cell the caller hands over holding 0 (one
// launch has no earlier kernel that could zero it, and a memset is a launch of its own on this runtime).
// The backward writes dz = scale[b] * g and dres = g (g = dy where y > 0, else 0) in one launch; either may be absent.
#pragma once
#include "common.h"
#include "philox.h"

namespace cstp {

constexpr int REG_THREADS = 256;
constexpr int REG_MAX_BLOCKS = 4096;      // memory-bound: a few blocks per CU, the rest by striding

// (Philox4, philox4x32_10: philox.h, shared with the erased box of randaug.h)

// u = (w >> 8) * 2^-24 is exact in fp32; kept iff u >= p
__device__ __forceinline__ float dropout_one(float x, uint32_t w, float p, float inv_keep) {
  const float u = (float)(w >> 8) * 5.9604644775390625e-8f;
  return u >= p ? x * inv_keep : 0.f;
}

template <bool VEC>
__global__ void __launch_bounds__(REG_THREADS)
dropout_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, float p, float inv_keep, uint32_t k0, uint32_t k1,
               uint32_t o0, uint32_t o1) {
  const int64_t groups = (n + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * REG_THREADS;
  for (int64_t q = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; q < groups; q += stride) {
    const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), o0, o1, k0, k1);
    const int64_t e = q << 2;
    if (VEC && e + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(x + e);
      float4 o;
      o.x = dropout_one(v.x, r.v[0], p, inv_keep);
      o.y = dropout_one(v.y, r.v[1], p, inv_keep);
      o.z = dropout_one(v.z, r.v[2], p, inv_keep);
      o.w = dropout_one(v.w, r.v[3], p, inv_keep);
      *reinterpret_cast<float4*>(y + e) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + j < n) y[e + j] = dropout_one(x[e + j], r.v[j], p, inv_keep);
    }
  }
}

// round to nearest even; NaN stays NaN.  Kept beside common.h's f2bf on purpose: this is integer arithmetic with an explicit NaN
// rule whose bits the tests pin, and it is not known to equal the hardware conversion on every NaN payload.
__device__ __forceinline__ unsigned short reg_f2bf(float a) {
  const unsigned u = __builtin_bit_cast(unsigned, a);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ unsigned reg_umax(unsigned a, unsigned b) { return a > b ? a : b; }

__device__ __forceinline__ float droppath_one(float s, float z, float r) { return fmaxf(fmaf(s, z, r), 0.f); }

// W elements per piece: fp32 4 or 1, bf16 8 or 1.  T = float or unsigned short.
template <typename T, int W>
__global__ void __launch_bounds__(REG_THREADS)
droppath_fwd_kernel(const T* __restrict__ z, const T* __restrict__ res, const float* __restrict__ scale, T* __restrict__ y,
                    int64_t row, int64_t nsamp, unsigned* __restrict__ cell) {
  __shared__ unsigned red[REG_THREADS / 64];
  const int64_t pieces = row / W;             // W > 1 only when row % W == 0
  const int64_t stride = (int64_t)gridDim.x * REG_THREADS;
  unsigned mx = 0;
  for (int64_t b = blockIdx.y; b < nsamp; b += gridDim.y) {
    const float s = scale[b];
    const T* zb = z + b * row;
    const T* rb = res + b * row;
    T* yb = y + b * row;
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < pieces; i += stride) {
      if constexpr (sizeof(T) == 4 && W == 4) {
        const float4 zv = *reinterpret_cast<const float4*>(zb + 4 * i);
        const float4 rv = *reinterpret_cast<const float4*>(rb + 4 * i);
        float4 o;
        o.x = droppath_one(s, zv.x, rv.x); o.y = droppath_one(s, zv.y, rv.y);
        o.z = droppath_one(s, zv.z, rv.z); o.w = droppath_one(s, zv.w, rv.w);
        *reinterpret_cast<float4*>(yb + 4 * i) = o;
        mx = reg_umax(reg_umax(mx, abs_bits(o.x)), abs_bits(o.y));
        mx = reg_umax(reg_umax(mx, abs_bits(o.z)), abs_bits(o.w));
      } else if constexpr (sizeof(T) == 4) {
        const float o = droppath_one(s, zb[i], rb[i]);
        yb[i] = o;
        mx = reg_umax(mx, abs_bits(o));
      } else if constexpr (W == 8) {
        const uint4 zv = *reinterpret_cast<const uint4*>(zb + 8 * i);
        const uint4 rv = *reinterpret_cast<const uint4*>(rb + 8 * i);
        const unsigned zw[4] = {zv.x, zv.y, zv.z, zv.w}, rw[4] = {rv.x, rv.y, rv.z, rv.w};
        unsigned ow[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float lo = droppath_one(s, bf2f((unsigned short)(zw[j] & 0xffffu)), bf2f((unsigned short)(rw[j] & 0xffffu)));
          const float hi = droppath_one(s, bf2f((unsigned short)(zw[j] >> 16)), bf2f((unsigned short)(rw[j] >> 16)));
          ow[j] = (unsigned)reg_f2bf(lo) | ((unsigned)reg_f2bf(hi) << 16);
        }
        *reinterpret_cast<uint4*>(yb + 8 * i) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
      } else {
        yb[i] = reg_f2bf(droppath_one(s, bf2f(zb[i]), bf2f(rb[i])));
      }
    }
  }
  if (cell != nullptr) {          // kernel-uniform.  A NaN in y has the largest bits and shows in the cell
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = reg_umax(mx, (unsigned)__shfl_xor((int)mx, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned a = reg_umax(reg_umax(red[0], red[1]), reg_umax(red[2], red[3]));
      if (a != 0) atomicMax(cell, a);
    }
  }
}

template <typename T, int W>
__global__ void __launch_bounds__(REG_THREADS)
droppath_bwd_kernel(const T* __restrict__ y, const T* __restrict__ dy, const float* __restrict__ scale, T* __restrict__ dz,
                    T* __restrict__ dres, int64_t row, int64_t nsamp) {
  const int64_t pieces = row / W;
  const int64_t stride = (int64_t)gridDim.x * REG_THREADS;
  for (int64_t b = blockIdx.y; b < nsamp; b += gridDim.y) {
    const float s = scale[b];
    const T* yb = y + b * row;
    const T* gb = dy + b * row;
    T* zb = dz != nullptr ? dz + b * row : nullptr;
    T* rb = dres != nullptr ? dres + b * row : nullptr;
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < pieces; i += stride) {
      if constexpr (sizeof(T) == 4 && W == 4) {
        const float4 yv = *reinterpret_cast<const float4*>(yb + 4 * i);
        float4 g = *reinterpret_cast<const float4*>(gb + 4 * i);
        g.x = yv.x > 0.f ? g.x : 0.f; g.y = yv.y > 0.f ? g.y : 0.f; g.z = yv.z > 0.f ? g.z : 0.f; g.w = yv.w > 0.f ? g.w : 0.f;
        if (rb != nullptr) *reinterpret_cast<float4*>(rb + 4 * i) = g;
        if (zb != nullptr) *reinterpret_cast<float4*>(zb + 4 * i) = make_float4(s * g.x, s * g.y, s * g.z, s * g.w);
      } else if constexpr (sizeof(T) == 4) {
        const float g = yb[i] > 0.f ? gb[i] : 0.f;
        if (rb != nullptr) rb[i] = g;
        if (zb != nullptr) zb[i] = s * g;
      } else if constexpr (W == 8) {
        const uint4 yv = *reinterpret_cast<const uint4*>(yb + 8 * i);
        const uint4 gv = *reinterpret_cast<const uint4*>(gb + 8 * i);
        const unsigned yw[4] = {yv.x, yv.y, yv.z, yv.w}, gw[4] = {gv.x, gv.y, gv.z, gv.w};
        unsigned ow[4], sw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          // the mask picks whole bf16 values: dres is a copy of dy's bits or +0
          const unsigned glo = bf2f((unsigned short)(yw[j] & 0xffffu)) > 0.f ? (gw[j] & 0xffffu) : 0u;
          const unsigned ghi = bf2f((unsigned short)(yw[j] >> 16)) > 0.f ? (gw[j] >> 16) : 0u;
          ow[j] = glo | (ghi << 16);
          sw[j] = (unsigned)reg_f2bf(s * bf2f((unsigned short)glo)) | ((unsigned)reg_f2bf(s * bf2f((unsigned short)ghi)) << 16);
        }
        if (rb != nullptr) *reinterpret_cast<uint4*>(rb + 8 * i) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        if (zb != nullptr) *reinterpret_cast<uint4*>(zb + 8 * i) = make_uint4(sw[0], sw[1], sw[2], sw[3]);
      } else {
        const unsigned short g = bf2f(yb[i]) > 0.f ? gb[i] : (unsigned short)0;
        if (rb != nullptr) rb[i] = g;
        if (zb != nullptr) zb[i] = reg_f2bf(s * bf2f(g));
      }
    }
  }
}

inline bool reg_aligned16(const void* a) { return a == nullptr || (reinterpret_cast<uintptr_t>(a) & 15) == 0; }

// grid.y walks the samples, grid.x the pieces of a row; together at most ~REG_MAX_BLOCKS blocks, the rest by striding
inline dim3 droppath_grid(int64_t pieces, int64_t nsamp) {
  const int64_t gy = nsamp < 1024 ? nsamp : 1024;
  int64_t gx = (pieces + REG_THREADS - 1) / REG_THREADS;
  const int64_t cap = REG_MAX_BLOCKS / gy > 0 ? REG_MAX_BLOCKS / gy : 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace cstp

extern "C" int cstp_philox4x32_10(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4) {
  using namespace cstp;
  CSTP_REQUIRE(ctr4 && key2 && out4, "null argument");
  const Philox4 r = philox4x32_10(ctr4[0], ctr4[1], ctr4[2], ctr4[3], key2[0], key2[1]);
  for (int j = 0; j < 4; ++j) out4[j] = r.v[j];
  return 0;
}

extern "C" int cstp_dropout(void* stream, const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset) {
  using namespace cstp;
  CSTP_REQUIRE(x && y, "null argument");
  CSTP_REQUIRE(n > 0, "bad size");
  CSTP_REQUIRE(p >= 0.f && p < 1.f, "dropout probability outside [0, 1)");      // (a NaN fails both comparisons)
  CSTP_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0, "unaligned fp32 pointer");
  const float inv_keep = 1.0f / (1.0f - p);
  const int64_t groups = (n + 3) >> 2;
  int64_t blocks = (groups + REG_THREADS - 1) / REG_THREADS;
  if (blocks > REG_MAX_BLOCKS) blocks = REG_MAX_BLOCKS;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), o0 = (uint32_t)offset, o1 = (uint32_t)(offset >> 32);
  if (reg_aligned16(x) && reg_aligned16(y))
    hipLaunchKernelGGL((dropout_kernel<true>), dim3((unsigned)blocks), dim3(REG_THREADS), 0, as_stream(stream), x, y, n, p, inv_keep, k0, k1, o0, o1);
  else
    hipLaunchKernelGGL((dropout_kernel<false>), dim3((unsigned)blocks), dim3(REG_THREADS), 0, as_stream(stream), x, y, n, p, inv_keep, k0, k1, o0, o1);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_droppath_add_relu_forward(void* stream, const void* z, const void* res, const float* scale, void* y, int64_t n,
                                              int64_t row, int32_t bf16, uint32_t* y_absmax) {
  using namespace cstp;
  CSTP_REQUIRE(z && res && scale && y, "null argument");
  CSTP_REQUIRE(n > 0 && row > 0 && n % row == 0, "bad size");
  CSTP_REQUIRE(bf16 == 0 || y_absmax == nullptr, "absmax by-product: fp32 only");
  const int64_t nsamp = n / row;
  const unsigned esz = bf16 ? 2 : 4;
  CSTP_REQUIRE(((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(res) | reinterpret_cast<uintptr_t>(y)) & (esz - 1)) == 0,
               "unaligned activation pointer");
  hipStream_t st = as_stream(stream);
  const bool al = reg_aligned16(z) && reg_aligned16(res) && reg_aligned16(y);
  if (!bf16) {
    const float* zf = static_cast<const float*>(z);
    const float* rf = static_cast<const float*>(res);
    float* yf = static_cast<float*>(y);
    if (al && row % 4 == 0)
      hipLaunchKernelGGL((droppath_fwd_kernel<float, 4>), droppath_grid(row / 4, nsamp), dim3(REG_THREADS), 0, st, zf, rf, scale, yf, row, nsamp, y_absmax);
    else
      hipLaunchKernelGGL((droppath_fwd_kernel<float, 1>), droppath_grid(row, nsamp), dim3(REG_THREADS), 0, st, zf, rf, scale, yf, row, nsamp, y_absmax);
  } else {
    const unsigned short* zh = static_cast<const unsigned short*>(z);
    const unsigned short* rh = static_cast<const unsigned short*>(res);
    unsigned short* yh = static_cast<unsigned short*>(y);
    if (al && row % 8 == 0)
      hipLaunchKernelGGL((droppath_fwd_kernel<unsigned short, 8>), droppath_grid(row / 8, nsamp), dim3(REG_THREADS), 0, st, zh, rh, scale, yh, row, nsamp,
                         (unsigned*)nullptr);
    else
      hipLaunchKernelGGL((droppath_fwd_kernel<unsigned short, 1>), droppath_grid(row, nsamp), dim3(REG_THREADS), 0, st, zh, rh, scale, yh, row, nsamp,
                         (unsigned*)nullptr);
  }
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_droppath_add_relu_backward(void* stream, const void* y, const void* dy, const float* scale, void* dz, void* dres,
                                               int64_t n, int64_t row, int32_t bf16) {
  using namespace cstp;
  CSTP_REQUIRE(y && dy && scale, "null argument");
  CSTP_REQUIRE(dz != nullptr || dres != nullptr, "null argument: one of dz, dres is needed");
  CSTP_REQUIRE(n > 0 && row > 0 && n % row == 0, "bad size");
  const int64_t nsamp = n / row;
  const unsigned esz = bf16 ? 2 : 4;
  CSTP_REQUIRE(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dz) |
                 reinterpret_cast<uintptr_t>(dres)) & (esz - 1)) == 0, "unaligned activation pointer");
  hipStream_t st = as_stream(stream);
  const bool al = reg_aligned16(y) && reg_aligned16(dy) && reg_aligned16(dz) && reg_aligned16(dres);
  if (!bf16) {
    const float* yf = static_cast<const float*>(y);
    const float* gf = static_cast<const float*>(dy);
    float* zf = static_cast<float*>(dz);
    float* rf = static_cast<float*>(dres);
    if (al && row % 4 == 0)
      hipLaunchKernelGGL((droppath_bwd_kernel<float, 4>), droppath_grid(row / 4, nsamp), dim3(REG_THREADS), 0, st, yf, gf, scale, zf, rf, row, nsamp);
    else
      hipLaunchKernelGGL((droppath_bwd_kernel<float, 1>), droppath_grid(row, nsamp), dim3(REG_THREADS), 0, st, yf, gf, scale, zf, rf, row, nsamp);
  } else {
    const unsigned short* yh = static_cast<const unsigned short*>(y);
    const unsigned short* gh = static_cast<const unsigned short*>(dy);
    unsigned short* zh = static_cast<unsigned short*>(dz);
    unsigned short* rh = static_cast<unsigned short*>(dres);
    if (al && row % 8 == 0)
      hipLaunchKernelGGL((droppath_bwd_kernel<unsigned short, 8>), droppath_grid(row / 8, nsamp), dim3(REG_THREADS), 0, st, yh, gh, scale, zh, rh, row, nsamp);
    else
      hipLaunchKernelGGL((droppath_bwd_kernel<unsigned short, 1>), droppath_grid(row, nsamp), dim3(REG_THREADS), 0, st, yh, gh, scale, zh, rh, row, nsamp);
  }
  CSTP_LAUNCH_CHECK();
  return 0;
}
