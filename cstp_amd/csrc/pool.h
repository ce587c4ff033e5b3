// MaxPool3d and AdaptiveAvgPool3d(1), once for both activation storages: T = float (misc.hip: cstp_maxpool3d_*, cstp_avgpool_*)
// or unsigned short holding bf16 (b16.hip: cstp_b16_maxpool3d_*, cstp_b16_avgpool_*).  Values are compared and summed in fp32;
// only pool_ld / pool_st know the storage.  The entries keep their own argument checks and grid rules.
#pragma once
#include "common.h"

namespace cstp {

__device__ __forceinline__ float pool_ld(float v) { return v; }
__device__ __forceinline__ float pool_ld(unsigned short v) { return bf2f(v); }
template <typename T> __device__ __forceinline__ T pool_st(float v);
template <> __device__ __forceinline__ float pool_st<float>(float v) { return v; }
template <> __device__ __forceinline__ unsigned short pool_st<unsigned short>(float v) { return f2bf(v); }     // round to nearest even

// ---- MaxPool3d (models/BE/r3d_byol.py:158: kernel 3, stride 2, padding 1; any k/stride/pad here) -------------------
// forward: y = max over the window (padding = -inf), idx = flat index (d*H + h)*W + w of the FIRST maximum in (d, h, w)
// scan order (what aten's CPU kernel keeps: it only replaces on `>` or NaN); one thread per output element, lanes along w.
// y takes the winner's stored value as it is (bf16: no conversion back); every window holds an element (2 * pad <= kernel).
template <typename T>
__global__ void maxpool3d_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int32_t* __restrict__ idx, int rows, int D, int H,
                                     int W, int Do, int Ho, int Wo, int kd, int kh, int kw, int sd, int sh, int sw, int pd, int ph,
                                     int pw) {
  const size_t total = (size_t)rows * Do * Ho * Wo;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    size_t r = i;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho); r /= Ho;
    const int dd = (int)(r % Do); const size_t row = r / Do;
    const T* xp = x + row * (size_t)D * H * W;
    float best = -INFINITY;
    T bb = pool_st<T>(-INFINITY);
    int bi = -1;
    for (int a = 0; a < kd; ++a) {
      const int id = dd * sd - pd + a;
      if ((unsigned)id >= (unsigned)D) continue;
      for (int b = 0; b < kh; ++b) {
        const int ih = ho * sh - ph + b;
        if ((unsigned)ih >= (unsigned)H) continue;
        for (int c = 0; c < kw; ++c) {
          const int iw = wo * sw - pw + c;
          if ((unsigned)iw >= (unsigned)W) continue;
          const int fi = (id * H + ih) * W + iw;
          const T raw = xp[fi];
          const float v = pool_ld(raw);
          if (v > best || v != v || bi < 0) { best = v; bb = raw; bi = fi; }
        }
      }
    }
    y[i] = bb;
    idx[i] = bi;
  }
}

// backward as a GATHER (deterministic, no atomics): dx[p] = sum of dy over the (at most ceil(k/s)^3) windows that cover p
// and whose recorded argmax is p.
template <typename T>
__global__ void maxpool3d_bwd_kernel(const T* __restrict__ dy, const int32_t* __restrict__ idx, T* __restrict__ dx, int rows, int D,
                                     int H, int W, int Do, int Ho, int Wo, int kd, int kh, int kw, int sd, int sh, int sw, int pd,
                                     int ph, int pw) {
  const size_t total = (size_t)rows * D * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    size_t r = i;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const int d = (int)(r % D); const size_t row = r / D;
    const int fi = (d * H + h) * W + w;
    // output coordinates o with o*s - p <= c <= o*s - p + k - 1
    const int d_lo = (d + pd - kd + sd) > 0 ? (d + pd - kd + sd) / sd : 0, d_hi = (d + pd) / sd < Do - 1 ? (d + pd) / sd : Do - 1;
    const int h_lo = (h + ph - kh + sh) > 0 ? (h + ph - kh + sh) / sh : 0, h_hi = (h + ph) / sh < Ho - 1 ? (h + ph) / sh : Ho - 1;
    const int w_lo = (w + pw - kw + sw) > 0 ? (w + pw - kw + sw) / sw : 0, w_hi = (w + pw) / sw < Wo - 1 ? (w + pw) / sw : Wo - 1;
    const size_t obase = row * (size_t)Do * Ho * Wo;
    float acc = 0.f;
    for (int a = d_lo; a <= d_hi; ++a)
      for (int b = h_lo; b <= h_hi; ++b)
        for (int c = w_lo; c <= w_hi; ++c) {
          const size_t o = obase + ((size_t)a * Ho + b) * Wo + c;
          if (idx[o] == fi) acc += pool_ld(dy[o]);
        }
    dx[i] = pool_st<T>(acc);
  }
}

// ---- AdaptiveAvgPool3d(1): rows of T -> fp32 means, one wave per (b, c) row; backward fp32 dy -> dx in T --------------
template <typename T>
__global__ void avgpool_fwd_kernel(const T* __restrict__ x, float* __restrict__ y, int rows, int s) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const T* p = x + (size_t)row * s;
  float a = 0.f;
  for (int i = lane; i < s; i += 64) a += pool_ld(p[i]);
  a = wave_sum(a);
  if (lane == 0) y[row] = a / (float)s;
}

template <typename T>
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, T* __restrict__ dx, int rows, int s) {
  const size_t total = (size_t)rows * s;
  const float inv = 1.f / (float)s;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) dx[i] = pool_st<T>(dy[i / s] * inv);
}

// ---- host side: the geometry check and the launch; pointers, rows and the entry's own view of d/h/w are checked by the caller ----
inline bool pool_dims(int D, int H, int W, const int32_t* k, const int32_t* st, const int32_t* pd, int& Do, int& Ho, int& Wo) {
  if (D <= 0 || H <= 0 || W <= 0) return false;
  for (int i = 0; i < 3; ++i) if (k[i] <= 0 || st[i] <= 0 || pd[i] < 0 || 2 * pd[i] > k[i]) return false;
  Do = (D + 2 * pd[0] - k[0]) / st[0] + 1;
  Ho = (H + 2 * pd[1] - k[1]) / st[1] + 1;
  Wo = (W + 2 * pd[2] - k[2]) / st[2] + 1;
  return Do > 0 && Ho > 0 && Wo > 0;
}

// `blocks`: the entry's grid rule, from the number of elements the kernel strides over to its block count.  The fp32 and the
// bf16 entries differ here (misc.hip, b16.hip); which rule is better has not been measured.
typedef unsigned (*PoolBlocks)(size_t elements);

template <typename T>
int maxpool3d_forward(void* stream, PoolBlocks blocks, const T* x, T* y, int32_t* argmax, int rows, int d, int h, int w,
                      const int32_t* k, const int32_t* st, const int32_t* pd) {
  int Do, Ho, Wo;
  CSTP_REQUIRE(pool_dims(d, h, w, k, st, pd, Do, Ho, Wo), "bad pooling geometry");
  CSTP_REQUIRE((size_t)d * h * w < (1ull << 31), "plane too large for int32 argmax");
  hipLaunchKernelGGL(maxpool3d_fwd_kernel<T>, dim3(blocks((size_t)rows * Do * Ho * Wo)), dim3(256), 0, as_stream(stream), x, y, argmax,
                     rows, d, h, w, Do, Ho, Wo, k[0], k[1], k[2], st[0], st[1], st[2], pd[0], pd[1], pd[2]);
  CSTP_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int maxpool3d_backward(void* stream, PoolBlocks blocks, const T* dy, const int32_t* argmax, T* dx, int rows, int d, int h, int w,
                       const int32_t* k, const int32_t* st, const int32_t* pd) {
  int Do, Ho, Wo;
  CSTP_REQUIRE(pool_dims(d, h, w, k, st, pd, Do, Ho, Wo), "bad pooling geometry");
  hipLaunchKernelGGL(maxpool3d_bwd_kernel<T>, dim3(blocks((size_t)rows * d * h * w)), dim3(256), 0, as_stream(stream), dy, argmax, dx,
                     rows, d, h, w, Do, Ho, Wo, k[0], k[1], k[2], st[0], st[1], st[2], pd[0], pd[1], pd[2]);
  CSTP_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int avgpool_forward(void* stream, const T* x, float* y, int rows, int s) {
  hipLaunchKernelGGL(avgpool_fwd_kernel<T>, dim3(cdiv(rows, 4)), dim3(256), 0, as_stream(stream), x, y, rows, s);
  CSTP_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int avgpool_backward(void* stream, PoolBlocks blocks, const float* dy, T* dx, int rows, int s) {
  hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(blocks((size_t)rows * s)), dim3(256), 0, as_stream(stream), dy, dx, rows, s);
  CSTP_LAUNCH_CHECK();
  return 0;
}

}  // namespace cstp
