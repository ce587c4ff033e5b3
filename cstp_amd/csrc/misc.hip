// Pooling, loss heads and the per-step flat-arena utilities (EMA, grad-norm clip, SGD, Adam; LARS in lars.h).
// All HBM-streaming or tiny; fp32 data, fp64 only inside reductions.
#include "common.h"
#include "pool.h"

namespace cstp {

thread_local char g_err[512] = {0};

__global__ void channel_sum_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int c, int s) {
  if (s == 1) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    double a = 0.0;
    for (int r = 0; r < n; ++r) a += (double)x[(size_t)r * c + ch];
    out[ch] = (float)a;
  } else {
    __shared__ double sm[16];
    const int ch = blockIdx.x;
    double a = 0.0;
    for (int r = 0; r < n; ++r) {
      const float* p = x + ((size_t)r * c + ch) * s;
      for (int i = threadIdx.x; i < s; i += blockDim.x) a += (double)p[i];
    }
    a = block_sum(a, sm);
    if (threadIdx.x == 0) out[ch] = (float)a;
  }
}

// ---- BYOL loss: 2 - 2 <x/|x|, y/|y|>; one wave per row -------------------------------------------
__global__ void byol_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ loss, int b,
                                int f) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* xp = x + (size_t)row * f;
  const float* yp = y + (size_t)row * f;
  float xx = 0.f, yy = 0.f, xy = 0.f;
  for (int i = lane; i < f; i += 64) { const float a = xp[i], c = yp[i]; xx += a * a; yy += c * c; xy += a * c; }
  xx = wave_sum(xx); yy = wave_sum(yy); xy = wave_sum(xy);
  if (lane == 0) {
    const float nx = fmaxf(sqrtf(xx), 1e-12f), ny = fmaxf(sqrtf(yy), 1e-12f);
    loss[row] = 2.f - 2.f * (xy / (nx * ny));
  }
}

__global__ void byol_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dloss,
                                float* __restrict__ dx, int b, int f) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* xp = x + (size_t)row * f;
  const float* yp = y + (size_t)row * f;
  float xx = 0.f, yy = 0.f, xy = 0.f;
  for (int i = lane; i < f; i += 64) { const float a = xp[i], c = yp[i]; xx += a * a; yy += c * c; xy += a * c; }
  xx = wave_sum_all(xx); yy = wave_sum_all(yy); xy = wave_sum_all(xy);
  const float nx = fmaxf(sqrtf(xx), 1e-12f), ny = fmaxf(sqrtf(yy), 1e-12f);
  const float cosv = xy / (nx * ny);
  const float g = -2.f * dloss[row] / nx;
  for (int i = lane; i < f; i += 64) dx[(size_t)row * f + i] = g * (yp[i] / ny - cosv * xp[i] / nx);
}

// ---- F.normalize(x, p=2, dim=1) (r21d_byol.py:396): y = x / max(|x|, eps); one wave per row -------
__global__ void l2norm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ norm, int f,
                                  float eps) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* xp = x + (size_t)row * f;
  float a = 0.f;
  for (int i = lane; i < f; i += 64) a += xp[i] * xp[i];
  a = wave_sum_all(a);
  const float nrm = fmaxf(sqrtf(a), eps);
  if (lane == 0) norm[row] = nrm;
  const float inv = 1.0f / nrm;
  for (int i = lane; i < f; i += 64) y[(size_t)row * f + i] = xp[i] * inv;
}

// dx = (dy - y <y, dy>) / max(|x|, eps)   (rows with |x| < eps: dx = dy / eps, as the clamp has zero slope)
__global__ void l2norm_bwd_kernel(const float* __restrict__ y, const float* __restrict__ norm, const float* __restrict__ dy,
                                  float* __restrict__ dx, int f, float eps) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* yp = y + (size_t)row * f;
  const float* gp = dy + (size_t)row * f;
  float d = 0.f;
  for (int i = lane; i < f; i += 64) d += yp[i] * gp[i];
  d = wave_sum_all(d);
  const float nrm = norm[row];
  if (!(nrm > eps)) d = 0.f;
  const float inv = 1.0f / nrm;
  for (int i = lane; i < f; i += 64) dx[(size_t)row * f + i] = (gp[i] - yp[i] * d) * inv;
}

// ---- CrossEntropyLoss(mean) ----------------------------------------------------------------------
__global__ void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, float* __restrict__ loss,
                              int b, int k) {
  __shared__ double sm[16];
  double a = 0.0;
  for (int r = threadIdx.x; r < b; r += blockDim.x) {
    const float* p = logits + (size_t)r * k;
    float mx = p[0];
    for (int j = 1; j < k; ++j) mx = fmaxf(mx, p[j]);
    float se = 0.f;
    for (int j = 0; j < k; ++j) se += expf(p[j] - mx);
    a += (double)(logf(se) + (mx - p[labels[r]]));      // (mx - p first: a large common offset of the logits costs no digits)
  }
  a = block_sum(a, sm);
  if (threadIdx.x == 0) loss[0] = (float)(a / b);
}

__global__ void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                              const float* __restrict__ dloss, float* __restrict__ dlogits, int b, int k) {
  const float gscale = dloss[0] / (float)b;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < b; r += gridDim.x * blockDim.x) {
    const float* p = logits + (size_t)r * k;
    float mx = p[0];
    for (int j = 1; j < k; ++j) mx = fmaxf(mx, p[j]);
    float se = 0.f;
    for (int j = 0; j < k; ++j) se += expf(p[j] - mx);
    const int lab = (int)labels[r];
    for (int j = 0; j < k; ++j) dlogits[(size_t)r * k + j] = gscale * (expf(p[j] - mx) / se - (j == lab ? 1.f : 0.f));
  }
}

// ---- soft-target CrossEntropy(mean): label smoothing and two weighted targets per row (mixup / CutMix) ----------------
// q[r][c] = (1-eps)*(lam[r]*[c==ta[r]] + (1-lam[r])*[c==tb[r]]) + eps/k;  loss = mean_r -sum_c q[r][c]*log_softmax(logits[r])[c].
// One wave per row with the 64 lanes along k (k is 51 / 101 / 400 here); the row statistics come out of xor-shuffles, whose
// order is fixed, so equal inputs give equal bits.  A target outside [0, k) carries no one-hot mass and is never an index.
// tb == NULL: tb = ta;  lam == NULL: lam = 1.
// Row statistics: mx = max_c p, se = sum_c exp(p - mx), sp = sum_c (p - mx).  Everything the loss adds is taken relative to mx,
// so a common offset of the row's logits, however large, costs none of the loss's digits.
__device__ __forceinline__ void soft_ce_row_stats(const float* __restrict__ p, int k, int lane, float& mx, float& se, float& sp) {
  float m = -INFINITY;
  for (int j = lane; j < k; j += 64) m = fmaxf(m, p[j]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  float e = 0.f, s = 0.f;
  for (int j = lane; j < k; j += 64) { const float v = p[j] - m; e += expf(v); s += v; }
  mx = m;
  se = wave_sum_all(e);
  sp = wave_sum_all(s);
}

// one block of 1024 threads: wave w takes rows w, w + 16, ...; the batch mean is accumulated in double (as ce_fwd_kernel does)
__global__ void __launch_bounds__(1024) soft_ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ ta,
                                                           const int64_t* __restrict__ tb, const float* __restrict__ lam,
                                                           float eps, float* __restrict__ loss, int b, int k) {
  __shared__ double sm[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double a = 0.0;
  for (int r = wave; r < b; r += nw) {
    const float* p = logits + (size_t)r * k;
    float mx, se, sp;
    soft_ce_row_stats(p, k, lane, mx, se, sp);
    if (lane == 0) {
      const float lg = logf(se);                       // the log-sum-exp relative to mx
      const int64_t a_ = ta[r], b_ = tb ? tb[r] : a_;
      const float l = lam ? lam[r] : 1.f;
      const float na = (a_ >= 0 && a_ < k) ? lg + (mx - p[a_]) : 0.f;
      const float nb = (b_ >= 0 && b_ < k) ? lg + (mx - p[b_]) : 0.f;
      a += (double)((1.f - eps) * (l * na + (1.f - l) * nb) + eps * (lg - sp / (float)k));
    }
  }
  a = block_sum(a, sm);
  if (threadIdx.x == 0) loss[0] = (float)(a / b);
}

// dlogits = dloss[0] * (softmax * sum_c q - q) / b (sum_c q = 1 unless a target lies outside); four rows per block, one wave each
__global__ void __launch_bounds__(256) soft_ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ ta,
                                                          const int64_t* __restrict__ tb, const float* __restrict__ lam,
                                                          float eps, const float* __restrict__ dloss,
                                                          float* __restrict__ dlogits, int b, int k) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= b) return;
  const float* p = logits + (size_t)r * k;
  float mx, se, sp;
  soft_ce_row_stats(p, k, lane, mx, se, sp);
  const float gscale = dloss[0] / (float)b, inv = 1.f / se;
  const int64_t a_ = ta[r], b_ = tb ? tb[r] : a_;
  const float l = lam ? lam[r] : 1.f;
  const float wa = (1.f - eps) * l, wb = (1.f - eps) * (1.f - l), u = eps / (float)k;
  // sum_c q: exactly 1 with both targets inside [0, k); a target outside takes its mass out of the row (and of softmax's weight)
  const float qs = 1.f - ((a_ >= 0 && a_ < k) ? 0.f : wa) - ((b_ >= 0 && b_ < k) ? 0.f : wb);
  for (int j = lane; j < k; j += 64) {
    const float q = (j == a_ ? wa : 0.f) + (j == b_ ? wb : 0.f) + u;
    dlogits[(size_t)r * k + j] = gscale * (qs * (expf(p[j] - mx) * inv) - q);
  }
}

// ---- NT-Xent ---------------------------------------------------------------------------------------
// ws layout (floats): norms[2n] | lse[2n] | sim[2n*2n] | G[2n*2n]
__global__ void ntx_norm_kernel(const float* __restrict__ reps, float* __restrict__ norms, int two_n, int f) {
  const int row = blockIdx.x, lane = threadIdx.x;
  float a = 0.f;
  for (int i = lane; i < f; i += 64) { const float v = reps[(size_t)row * f + i]; a += v * v; }
  a = wave_sum(a);
  if (lane == 0) norms[row] = sqrtf(a);
}

// one block (256 threads = 4 waves) per row i; wave w handles columns j = w, w+4, ...
__global__ void ntx_sim_kernel(const float* __restrict__ reps, const float* __restrict__ norms, float* __restrict__ sim,
                               int two_n, int f) {
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* ri = reps + (size_t)i * f;
  for (int j = wave; j < two_n; j += 4) {
    const float* rj = reps + (size_t)j * f;
    float a = 0.f;
    for (int q = lane; q < f; q += 64) a += ri[q] * rj[q];
    a = wave_sum(a);
    if (lane == 0) sim[(size_t)i * two_n + j] = a / fmaxf(norms[i] * norms[j], 1e-8f);
  }
}

__global__ void ntx_loss_kernel(const float* __restrict__ sim, float* __restrict__ lse, float* __restrict__ loss, int two_n,
                                float inv_t) {
  __shared__ double sm[16];
  const int n = two_n >> 1;
  double a = 0.0;
  for (int i = threadIdx.x; i < two_n; i += blockDim.x) {
    const float* p = sim + (size_t)i * two_n;
    float mx = -3.0e38f;
    for (int j = 0; j < two_n; ++j) if (j != i) mx = fmaxf(mx, p[j] * inv_t);
    float se = 0.f;
    for (int j = 0; j < two_n; ++j) if (j != i) se += expf(p[j] * inv_t - mx);
    const float l = logf(se) + mx;
    lse[i] = l;
    const int pos = (i + n) % two_n;
    a += (double)(l - p[pos] * inv_t);
  }
  a = block_sum(a, sm);
  if (threadIdx.x == 0) loss[0] = (float)(a / two_n);
}

__global__ void ntx_g_kernel(const float* __restrict__ sim, const float* __restrict__ lse, const float* __restrict__ dloss,
                             float* __restrict__ G, int two_n, float inv_t) {
  const int n = two_n >> 1;
  const float sc = dloss[0] * inv_t / (float)two_n;
  const int total = two_n * two_n;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int i = e / two_n, j = e - i * two_n;
    float g = 0.f;
    if (j != i) {
      g = expf(sim[e] * inv_t - lse[i]);
      if (j == (i + n) % two_n) g -= 1.f;
      g *= sc;
    }
    G[e] = g;
  }
}

// one block per row i: d_hat = sum_j (G_ij + G_ji) rhat_j ; dreps_i = (d_hat - rhat_i <rhat_i, d_hat>) / |r_i|
__global__ void ntx_bwd_kernel(const float* __restrict__ reps, const float* __restrict__ norms, const float* __restrict__ G,
                               float* __restrict__ dreps, int two_n, int f) {
  __shared__ float sm[16];
  const int i = blockIdx.x;
  const float ni = fmaxf(norms[i], 1e-8f);
  float dot = 0.f;
  // each thread owns features q = tid, tid+256, ... (f <= 256*8 supported)
  float dh[8];
  int cnt = 0;
  for (int q = threadIdx.x; q < f && cnt < 8; q += blockDim.x, ++cnt) {
    float a = 0.f;
    for (int j = 0; j < two_n; ++j) {
      const float w = G[(size_t)i * two_n + j] + G[(size_t)j * two_n + i];
      a += w * reps[(size_t)j * f + q] / fmaxf(norms[j], 1e-8f);
    }
    dh[cnt] = a;
    dot += a * reps[(size_t)i * f + q] / ni;
  }
  dot = block_sum(dot, sm);
  __shared__ float bdot;
  if (threadIdx.x == 0) bdot = dot;
  __syncthreads();
  dot = bdot;
  cnt = 0;
  for (int q = threadIdx.x; q < f && cnt < 8; q += blockDim.x, ++cnt)
    dreps[(size_t)i * f + q] = (dh[cnt] - reps[(size_t)i * f + q] / ni * dot) / ni;
}

// ---- flat-arena utilities ---------------------------------------------------------------------------
__global__ void ema_kernel(float* __restrict__ t, const float* __restrict__ o, size_t n, float m, float om) {
  const size_t n4 = n >> 2;
  float4* t4 = reinterpret_cast<float4*>(t);
  const float4* o4 = reinterpret_cast<const float4*>(o);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 a = t4[i];
    const float4 b = o4[i];
    a.x = a.x * m + b.x * om; a.y = a.y * m + b.y * om; a.z = a.z * m + b.z * om; a.w = a.w * m + b.w * om;
    t4[i] = a;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = (n4 << 2) + threadIdx.x;
    t[i] = t[i] * m + o[i] * om;
  }
}

__global__ void sumsq_partial_kernel(const float* __restrict__ g, size_t n, double* __restrict__ part) {
  __shared__ double sm[16];
  double a = 0.0;
  const size_t n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = g4[i];
    a += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[(n4 << 2) + threadIdx.x]; a += (double)v * v; }
  a = block_sum(a, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}

__global__ void sumsq_final_kernel(const double* __restrict__ part, int nb, float* __restrict__ out) {
  __shared__ double sm[16];
  double a = 0.0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) a += part[i];
  a = block_sum(a, sm);
  if (threadIdx.x == 0) out[0] = (float)a;
}

__global__ void clip_coef_kernel(const float* __restrict__ sumsq, float max_norm, float* __restrict__ coef,
                                 float* __restrict__ norm_out) {
  const float nrm = sqrtf(sumsq[0]);
  const float c = max_norm / (nrm + 1e-6f);
  coef[0] = c < 1.f ? c : 1.f;
  if (norm_out != nullptr) norm_out[0] = nrm;
}

__global__ void sgd_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, size_t n,
                           const float* __restrict__ lr_p, float momentum, float wd, const float* __restrict__ coef_p,
                           int first_step, int write_back) {
  const float lr = lr_p[0];
  const float coef = coef_p != nullptr ? coef_p[0] : 1.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float gr = g[i] * coef;
    if (write_back) g[i] = gr;
    const float pv = p[i];
    gr = gr + wd * pv;
    const float b = first_step ? gr : momentum * buf[i] + gr;
    buf[i] = b;
    p[i] = pv - lr * b;
  }
}

// torch.optim.Adam / AdamW (no amsgrad), bias corrections passed in as 1 - beta^t
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            size_t n, const float* __restrict__ lr_p, float b1, float b2, float eps, float wd, int decoupled,
                            float bc1, float bc2_sqrt) {
  const float lr = lr_p[0];
  const float step_size = lr / bc1;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    float pv = p[i], gr = g[i];
    if (decoupled) pv *= (1.f - lr * wd);
    else gr += wd * pv;
    const float mi = b1 * m[i] + (1.f - b1) * gr;
    const float vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi;
    v[i] = vi;
    p[i] = pv - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
  }
}

static inline int stream_grid(size_t n) {
  size_t b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace cstp

using namespace cstp;

extern "C" int cstp_abi_version(void) { return CSTP_ABI_VERSION; }
extern "C" const char* cstp_last_error(void) { return g_err; }

// the fp32 pooling grid rules (pool.h: PoolBlocks): max-pool forward and backward, average backward
static unsigned maxpool_blocks(size_t n) { return (unsigned)stream_grid(n) * 8; }
static unsigned avgpool_blocks(size_t n) { return (unsigned)stream_grid(n); }

extern "C" int cstp_avgpool_forward(void* stream, const float* x, float* y, int32_t rows, int32_t s) {
  CSTP_REQUIRE(x && y && rows > 0 && s > 0, "bad argument");
  return avgpool_forward(stream, x, y, rows, s);
}

extern "C" int cstp_avgpool_backward(void* stream, const float* dy, float* dx, int32_t rows, int32_t s) {
  CSTP_REQUIRE(dy && dx && rows > 0 && s > 0, "bad argument");
  return avgpool_backward(stream, avgpool_blocks, dy, dx, rows, s);
}

extern "C" int cstp_channel_sum(void* stream, const float* x, float* out, int32_t n, int32_t c, int32_t s, void* ws,
                                size_t ws_bytes) {
  (void)ws; (void)ws_bytes;
  CSTP_REQUIRE(x && out && n > 0 && c > 0 && s > 0, "bad argument");
  if (s == 1) hipLaunchKernelGGL(channel_sum_kernel, dim3(cdiv(c, 64)), dim3(64), 0, as_stream(stream), x, out, n, c, s);
  else hipLaunchKernelGGL(channel_sum_kernel, dim3(c), dim3(256), 0, as_stream(stream), x, out, n, c, s);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_byol_loss_forward(void* stream, const float* x, const float* y, float* loss, int32_t b, int32_t f) {
  CSTP_REQUIRE(x && y && loss && b > 0 && f > 0, "bad argument");
  hipLaunchKernelGGL(byol_fwd_kernel, dim3(b), dim3(64), 0, as_stream(stream), x, y, loss, b, f);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_byol_loss_backward(void* stream, const float* x, const float* y, const float* dloss, float* dx,
                                       int32_t b, int32_t f) {
  CSTP_REQUIRE(x && y && dloss && dx && b > 0 && f > 0, "bad argument");
  hipLaunchKernelGGL(byol_bwd_kernel, dim3(b), dim3(64), 0, as_stream(stream), x, y, dloss, dx, b, f);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_l2_normalize_forward(void* stream, const float* x, float* y, float* norm, int32_t rows, int32_t f,
                                         float eps) {
  CSTP_REQUIRE(x && y && norm && rows > 0 && f > 0, "bad argument");
  hipLaunchKernelGGL(l2norm_fwd_kernel, dim3(rows), dim3(64), 0, as_stream(stream), x, y, norm, f, eps);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_l2_normalize_backward(void* stream, const float* y, const float* norm, const float* dy, float* dx,
                                          int32_t rows, int32_t f, float eps) {
  CSTP_REQUIRE(y && norm && dy && dx && rows > 0 && f > 0, "bad argument");
  hipLaunchKernelGGL(l2norm_bwd_kernel, dim3(rows), dim3(64), 0, as_stream(stream), y, norm, dy, dx, f, eps);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_cross_entropy_forward(void* stream, const float* logits, const int64_t* labels, float* loss,
                                          int32_t b, int32_t k) {
  CSTP_REQUIRE(logits && labels && loss && b > 0 && k > 0, "bad argument");
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(1), dim3(256), 0, as_stream(stream), logits, labels, loss, b, k);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_cross_entropy_backward(void* stream, const float* logits, const int64_t* labels, const float* dloss,
                                           float* dlogits, int32_t b, int32_t k) {
  CSTP_REQUIRE(logits && labels && dloss && dlogits && b > 0 && k > 0, "bad argument");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(cdiv(b, 256)), dim3(256), 0, as_stream(stream), logits, labels, dloss, dlogits, b, k);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_soft_cross_entropy_forward(void* stream, const float* logits, const int64_t* ta, const int64_t* tb,
                                               const float* lam, float eps, float* loss, int32_t b, int32_t k) {
  CSTP_REQUIRE(logits && ta && loss, "null argument");
  CSTP_REQUIRE(b > 0 && k > 0 && (int64_t)b * k <= INT32_MAX, "bad shape");
  CSTP_REQUIRE(eps >= 0.f && eps < 1.f, "label smoothing outside [0, 1)");
  hipLaunchKernelGGL(soft_ce_fwd_kernel, dim3(1), dim3(1024), 0, as_stream(stream), logits, ta, tb, lam, eps, loss, b, k);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_soft_cross_entropy_backward(void* stream, const float* logits, const int64_t* ta, const int64_t* tb,
                                                const float* lam, float eps, const float* dloss, float* dlogits, int32_t b,
                                                int32_t k) {
  CSTP_REQUIRE(logits && ta && dloss && dlogits, "null argument");
  CSTP_REQUIRE(b > 0 && k > 0 && (int64_t)b * k <= INT32_MAX, "bad shape");
  CSTP_REQUIRE(eps >= 0.f && eps < 1.f, "label smoothing outside [0, 1)");
  CSTP_REQUIRE(dlogits != logits, "dlogits must not alias logits");
  hipLaunchKernelGGL(soft_ce_bwd_kernel, dim3(cdiv(b, 4)), dim3(256), 0, as_stream(stream), logits, ta, tb, lam, eps, dloss,
                     dlogits, b, k);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cstp_ntxent_workspace_bytes(int32_t two_n, int32_t f) {
  (void)f;
  if (two_n <= 0) return 0;
  return align_up(((size_t)2 * two_n + (size_t)2 * two_n * two_n) * sizeof(float), 256);
}

extern "C" int cstp_ntxent_forward(void* stream, const float* reps, float* loss, int32_t two_n, int32_t f,
                                   float temperature, void* ws, size_t ws_bytes) {
  CSTP_REQUIRE(reps && loss && ws, "null argument");
  CSTP_REQUIRE(two_n >= 4 && (two_n % 2) == 0 && f > 0 && temperature > 0.f, "bad shape");
  CSTP_REQUIRE(ws_bytes >= cstp_ntxent_workspace_bytes(two_n, f), "workspace too small");
  hipStream_t s = as_stream(stream);
  float* norms = reinterpret_cast<float*>(ws);
  float* lse = norms + two_n;
  float* sim = lse + two_n;
  hipLaunchKernelGGL(ntx_norm_kernel, dim3(two_n), dim3(64), 0, s, reps, norms, two_n, f);
  hipLaunchKernelGGL(ntx_sim_kernel, dim3(two_n), dim3(256), 0, s, reps, norms, sim, two_n, f);
  hipLaunchKernelGGL(ntx_loss_kernel, dim3(1), dim3(256), 0, s, sim, lse, loss, two_n, 1.f / temperature);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_ntxent_backward(void* stream, const float* reps, const float* dloss, float* dreps, int32_t two_n,
                                    int32_t f, float temperature, void* ws, size_t ws_bytes) {
  CSTP_REQUIRE(reps && dloss && dreps && ws, "null argument");
  CSTP_REQUIRE(two_n >= 4 && (two_n % 2) == 0 && f > 0 && f <= 2048 && temperature > 0.f, "bad shape");
  CSTP_REQUIRE(ws_bytes >= cstp_ntxent_workspace_bytes(two_n, f), "workspace too small");
  hipStream_t s = as_stream(stream);
  float* norms = reinterpret_cast<float*>(ws);
  float* lse = norms + two_n;
  float* sim = lse + two_n;
  float* G = sim + (size_t)two_n * two_n;
  hipLaunchKernelGGL(ntx_g_kernel, dim3(cdiv(two_n * two_n, 256)), dim3(256), 0, s, sim, lse, dloss, G, two_n, 1.f / temperature);
  hipLaunchKernelGGL(ntx_bwd_kernel, dim3(two_n), dim3(256), 0, s, reps, norms, G, dreps, two_n, f);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_ema_update(void* stream, float* target, const float* online, size_t n, double m) {
  CSTP_REQUIRE(target && online && n > 0, "bad argument");
  CSTP_REQUIRE((reinterpret_cast<uintptr_t>(target) & 15) == 0 && (reinterpret_cast<uintptr_t>(online) & 15) == 0,
               "arenas must be 16-byte aligned");
  hipLaunchKernelGGL(ema_kernel, dim3(stream_grid(n / 4 + 1)), dim3(256), 0, as_stream(stream), target, online, n, (float)m,
                     (float)(1.0 - m));
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_sumsq(void* stream, const float* g, size_t n, float* out, void* ws, size_t ws_bytes) {
  CSTP_REQUIRE(g && out && ws && n > 0, "bad argument");
  CSTP_REQUIRE(ws_bytes >= 8192, "workspace too small (need 8 KiB)");
  CSTP_REQUIRE((reinterpret_cast<uintptr_t>(g) & 15) == 0, "arena must be 16-byte aligned");
  int nb = stream_grid(n / 4 + 1);
  if (nb > 1024) nb = 1024;
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, as_stream(stream), g, n, part);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, as_stream(stream), part, nb, out);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_coef(void* stream, const float* sumsq, float max_norm, float* coef, float* norm_out) {
  CSTP_REQUIRE(sumsq && coef, "null argument");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, as_stream(stream), sumsq, max_norm, coef, norm_out);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_sgd_step(void* stream, float* p, float* g, float* buf, size_t n, const float* lr, float momentum,
                             float weight_decay, const float* coef, int32_t first_step, int32_t write_back_grad) {
  CSTP_REQUIRE(p && g && buf && lr && n > 0, "bad argument");
  hipLaunchKernelGGL(sgd_kernel, dim3(stream_grid(n)), dim3(256), 0, as_stream(stream), p, g, buf, n, lr, momentum,
                     weight_decay, coef, first_step, write_back_grad);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_adam_step(void* stream, float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n,
                              const float* lr, float beta1, float beta2, float eps, float weight_decay, int32_t decoupled,
                              int32_t step) {
  CSTP_REQUIRE(p && g && exp_avg && exp_avg_sq && lr && n > 0 && step > 0, "bad argument");
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(n)), dim3(256), 0, as_stream(stream), p, g, exp_avg, exp_avg_sq, n, lr,
                     beta1, beta2, eps, weight_decay, decoupled, (float)bc1, (float)sqrt(bc2));
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_maxpool3d_forward(void* stream, const float* x, float* y, int32_t* argmax, int32_t rows, int32_t d, int32_t h,
                                      int32_t w, const int32_t* kernel3, const int32_t* stride3, const int32_t* pad3) {
  CSTP_REQUIRE(x && y && argmax && kernel3 && stride3 && pad3 && rows > 0, "bad argument");
  return maxpool3d_forward(stream, maxpool_blocks, x, y, argmax, rows, d, h, w, kernel3, stride3, pad3);
}

extern "C" int cstp_maxpool3d_backward(void* stream, const float* dy, const int32_t* argmax, float* dx, int32_t rows, int32_t d,
                                       int32_t h, int32_t w, const int32_t* kernel3, const int32_t* stride3, const int32_t* pad3) {
  CSTP_REQUIRE(dy && argmax && dx && kernel3 && stride3 && pad3 && rows > 0, "bad argument");
  return maxpool3d_backward(stream, maxpool_blocks, dy, argmax, dx, rows, d, h, w, kernel3, stride3, pad3);
}

#include "lars.h"
#include "optim_table.h"
#include "reg.h"
