// SGD and Adam / AdamW over the flat arenas with PER-TENSOR hyper-parameters (cstp_tab_sgd_step / cstp_tab_adam_step, spec in
// include/cstp_hip.h), and the weight EMA of fine-tuning folded into the same pass.
//
// cstp_sgd_step / cstp_adam_step take one learning rate and one weight decay per launch, so an optimizer whose tensors differ in
// either (layer-wise learning-rate decay; no weight decay on biases and BatchNorm vectors) needs one launch per tensor: ~170 small
// launches where the flat arenas were built to need one.  The remedy is the one of lars.h: the host deals every trainable tensor's
// padded extent out in chunks of at most CSTP_LARS_CHUNK floats (the same chunk table, read through the same lars_chunk check)
// and one block owns one chunk; what differs per tensor is looked up per BLOCK in a float table
//   hyper [n_segs][2] = {lr scale, weight decay}                a segment is one tensor
// so the step is one launch whatever the grouping.  The base learning rate stays the device scalar it is in the plain kernels;
// lr[0] * scale[s] is one fp32 product (scale 1 gives lr[0] back exactly).
// The arithmetic per element is the plain kernels' (sgd_kernel / adam_kernel in misc.hip), expression for expression, so with all
// scales 1 and one decay the results are the plain kernels' bits.
// ema (optional, same layout as p): ema <- m * ema + (1 - m) * p_new, in the same pass: the separate pass would read p again.
// No atomics; a float has one writer.  Padding floats are zero in p, g, the state arenas and ema and stay zero (every update of
// an all-zero element is zero).  A table entry that does not describe floats of the arena is left alone (lars_chunk).
#pragma once
#include "lars.h"

namespace cstp {

struct TabHyper { float scale, wd; };

// {lr scale, weight decay} of the block's segment; block-uniform (c.seg < n_segs was checked by lars_chunk)
__device__ __forceinline__ TabHyper tab_hyper(const float* __restrict__ hyper, int seg) {
  TabHyper h;
  h.scale = hyper[2 * seg];
  h.wd = hyper[2 * seg + 1];
  return h;
}

// one element of sgd_kernel: g' = c g;  g' += wd p;  buf = first ? g' : momentum buf + g';  p -= lr buf
__device__ __forceinline__ void tab_sgd_elem(float& pv, float& gv, float& bv, float coef, float wd, float momentum, float lr,
                                             int first_step) {
  // (sgd_kernel's three multiply-adds are contracted; spelled out, as in tab_adam_elem below)
#pragma clang fp contract(off)
  float gr = gv * coef;
  gv = gr;
  gr = fmaf(wd, pv, gr);
  const float b = first_step ? gr : fmaf(momentum, bv, gr);
  bv = b;
  pv = fmaf(-lr, b, pv);
}

template <bool EMA>
__global__ void __launch_bounds__(LARS_THREADS)
tab_sgd_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema, size_t n,
               const int32_t* __restrict__ chunks, const float* __restrict__ hyper, int n_segs, const float* __restrict__ lr_p,
               float momentum, const float* __restrict__ coef_p, int first_step, int write_back, float em, float eom) {
  const LarsChunk c = lars_chunk(chunks, n_segs, n);
  if (c.len == 0) return;
  const TabHyper h = tab_hyper(hyper, c.seg);
  const float lr = lr_p[0] * h.scale;
  const float coef = coef_p != nullptr ? coef_p[0] : 1.f;
  float4* p4 = reinterpret_cast<float4*>(p + c.off);
  float4* g4 = reinterpret_cast<float4*>(g + c.off);
  float4* b4 = reinterpret_cast<float4*>(buf + c.off);
  float4* e4 = EMA ? reinterpret_cast<float4*>(ema + c.off) : nullptr;
  const int n4 = c.len >> 2;
#pragma unroll
  for (int k = 0; k < CSTP_LARS_CHUNK / (4 * LARS_THREADS); ++k) {
    const int i = k * LARS_THREADS + threadIdx.x;
    if (i < n4) {
      float4 pv = p4[i], gv = g4[i], bv = b4[i];
      tab_sgd_elem(pv.x, gv.x, bv.x, coef, h.wd, momentum, lr, first_step);
      tab_sgd_elem(pv.y, gv.y, bv.y, coef, h.wd, momentum, lr, first_step);
      tab_sgd_elem(pv.z, gv.z, bv.z, coef, h.wd, momentum, lr, first_step);
      tab_sgd_elem(pv.w, gv.w, bv.w, coef, h.wd, momentum, lr, first_step);
      if (write_back) g4[i] = gv;
      b4[i] = bv;
      p4[i] = pv;
      if (EMA) {
        float4 ev = e4[i];
        ev.x = ev.x * em + pv.x * eom; ev.y = ev.y * em + pv.y * eom; ev.z = ev.z * em + pv.z * eom; ev.w = ev.w * em + pv.w * eom;
        e4[i] = ev;
      }
    }
  }
}

// one element of adam_kernel (bias corrections passed in as 1 - beta1^t and sqrt(1 - beta2^t)).  Which of adam_kernel's products
// meet their sums in one rounding is the compiler's choice there (it packs the two moment updates into v_pk_mul_f32 / v_pk_add_f32,
// products and sums rounded separately, and fuses the rest); the choice is spelled out here so that this kernel, whose float4
// body the compiler would pack differently, rounds where that one does.
__device__ __forceinline__ void tab_adam_elem(float& pv, float gr, float& mv, float& vv, float lr, float step_size, float b1,
                                              float b2, float eps, float wd, int decoupled, float bc2_sqrt) {
#pragma clang fp contract(off)
  if (decoupled) pv *= fmaf(-lr, wd, 1.f);
  else gr = fmaf(wd, pv, gr);
  const float mi = b1 * mv + (1.f - b1) * gr;
  const float vi = b2 * vv + (1.f - b2) * gr * gr;
  mv = mi;
  vv = vi;
  pv = fmaf(-step_size, mi / (sqrtf(vi) / bc2_sqrt + eps), pv);
}

template <bool EMA>
__global__ void __launch_bounds__(LARS_THREADS)
tab_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                float* __restrict__ ema, size_t n, const int32_t* __restrict__ chunks, const float* __restrict__ hyper, int n_segs,
                const float* __restrict__ lr_p, float b1, float b2, float eps, int decoupled, float bc1, float bc2_sqrt, float em,
                float eom) {
  const LarsChunk c = lars_chunk(chunks, n_segs, n);
  if (c.len == 0) return;
  const TabHyper h = tab_hyper(hyper, c.seg);
  const float lr = lr_p[0] * h.scale;
  const float step_size = lr / bc1;
  float4* p4 = reinterpret_cast<float4*>(p + c.off);
  const float4* g4 = reinterpret_cast<const float4*>(g + c.off);
  float4* m4 = reinterpret_cast<float4*>(m + c.off);
  float4* v4 = reinterpret_cast<float4*>(v + c.off);
  float4* e4 = EMA ? reinterpret_cast<float4*>(ema + c.off) : nullptr;
  const int n4 = c.len >> 2;
#pragma unroll
  for (int k = 0; k < CSTP_LARS_CHUNK / (4 * LARS_THREADS); ++k) {
    const int i = k * LARS_THREADS + threadIdx.x;
    if (i < n4) {
      float4 pv = p4[i], mv = m4[i], vv = v4[i];
      const float4 gv = g4[i];
      tab_adam_elem(pv.x, gv.x, mv.x, vv.x, lr, step_size, b1, b2, eps, h.wd, decoupled, bc2_sqrt);
      tab_adam_elem(pv.y, gv.y, mv.y, vv.y, lr, step_size, b1, b2, eps, h.wd, decoupled, bc2_sqrt);
      tab_adam_elem(pv.z, gv.z, mv.z, vv.z, lr, step_size, b1, b2, eps, h.wd, decoupled, bc2_sqrt);
      tab_adam_elem(pv.w, gv.w, mv.w, vv.w, lr, step_size, b1, b2, eps, h.wd, decoupled, bc2_sqrt);
      m4[i] = mv;
      v4[i] = vv;
      p4[i] = pv;
      if (EMA) {
        float4 ev = e4[i];
        ev.x = ev.x * em + pv.x * eom; ev.y = ev.y * em + pv.y * eom; ev.z = ev.z * em + pv.z * eom; ev.w = ev.w * em + pv.w * eom;
        e4[i] = ev;
      }
    }
  }
}

}  // namespace cstp

extern "C" int cstp_tab_sgd_step(void* stream, float* p, float* g, float* buf, float* ema, size_t n, const int32_t* chunks,
                                 int32_t n_chunks, const float* hyper, int32_t n_segs, const float* lr, float momentum,
                                 const float* coef, int32_t first_step, int32_t write_back_grad, float ema_momentum) {
  using namespace cstp;
  CSTP_REQUIRE(p && g && buf && chunks && hyper && lr, "null argument");
  CSTP_REQUIRE(n_chunks > 0 && n_segs > 0 && n_segs <= n_chunks, "bad table size");
  CSTP_REQUIRE(n > 0 && n < ((size_t)1 << 31), "arena must hold 1 .. 2^31 - 1 floats (offsets are int32)");
  CSTP_REQUIRE(ema == nullptr || (ema_momentum >= 0.f && ema_momentum <= 1.f), "ema momentum outside [0, 1]");
  CSTP_REQUIRE(lars_aligned(p) && lars_aligned(g) && lars_aligned(buf) && lars_aligned(ema), "arenas must be 16-byte aligned");
  CSTP_REQUIRE(ema != p && ema != g && ema != buf, "ema must not alias p, g or buf");
  const float em = ema_momentum, eom = (float)(1.0 - (double)ema_momentum);
  if (ema != nullptr)
    hipLaunchKernelGGL(tab_sgd_kernel<true>, dim3(n_chunks), dim3(LARS_THREADS), 0, as_stream(stream), p, g, buf, ema, n, chunks,
                       hyper, n_segs, lr, momentum, coef, first_step, write_back_grad, em, eom);
  else
    hipLaunchKernelGGL(tab_sgd_kernel<false>, dim3(n_chunks), dim3(LARS_THREADS), 0, as_stream(stream), p, g, buf, ema, n, chunks,
                       hyper, n_segs, lr, momentum, coef, first_step, write_back_grad, em, eom);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_tab_adam_step(void* stream, float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                                  const int32_t* chunks, int32_t n_chunks, const float* hyper, int32_t n_segs, const float* lr,
                                  float beta1, float beta2, float eps, int32_t decoupled, int32_t step, float ema_momentum) {
  using namespace cstp;
  CSTP_REQUIRE(p && g && exp_avg && exp_avg_sq && chunks && hyper && lr, "null argument");
  CSTP_REQUIRE(step > 0, "step counts from 1");
  CSTP_REQUIRE(n_chunks > 0 && n_segs > 0 && n_segs <= n_chunks, "bad table size");
  CSTP_REQUIRE(n > 0 && n < ((size_t)1 << 31), "arena must hold 1 .. 2^31 - 1 floats (offsets are int32)");
  CSTP_REQUIRE(ema == nullptr || (ema_momentum >= 0.f && ema_momentum <= 1.f), "ema momentum outside [0, 1]");
  CSTP_REQUIRE(lars_aligned(p) && lars_aligned(g) && lars_aligned(exp_avg) && lars_aligned(exp_avg_sq) && lars_aligned(ema),
               "arenas must be 16-byte aligned");
  CSTP_REQUIRE(ema != p && ema != g && ema != exp_avg && ema != exp_avg_sq, "ema must not alias p, g or the moments");
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float em = ema_momentum, eom = (float)(1.0 - (double)ema_momentum);
  if (ema != nullptr)
    hipLaunchKernelGGL(tab_adam_kernel<true>, dim3(n_chunks), dim3(LARS_THREADS), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq,
                       ema, n, chunks, hyper, n_segs, lr, beta1, beta2, eps, decoupled, (float)bc1, (float)sqrt(bc2), em, eom);
  else
    hipLaunchKernelGGL(tab_adam_kernel<false>, dim3(n_chunks), dim3(LARS_THREADS), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq,
                       ema, n, chunks, hyper, n_segs, lr, beta1, beta2, eps, decoupled, (float)bc1, (float)sqrt(bc2), em, eom);
  CSTP_LAUNCH_CHECK();
  return 0;
}
