// I3D inception ("Mixed") tail and TensorFlow-SAME pooling (models/BE/i3d_byol.py:170-220), forward and backward.
//
// 1. SAME max-pool: MaxPool3d(k, s, ceil_mode=True) over ConstantPad3d(get_padding_shape(k, s), 0) without the padded copy.
//    A window position inside the one-sided zero padding is a candidate of value 0, one beyond the padded extent (ceil mode)
//    is none.  Volumes that fit LDS (every pooling inside and between the Mixed blocks) are staged there, several (n, c)
//    volumes per block when they are small, so the 27 reads per output of the 3x3x3 / stride 1 pool are LDS reads; larger
//    volumes (the first 1x3x3 pool behind the stem) read through L1 / L2.  Backward is a gather over the covering windows,
//    with the argmax and dy volumes staged in LDS in the same way.
// 2. BatchNorm + ReLU of the four branches written straight into the block's concat tensor: statistics (only for branches whose
//    convolution left no partial sums), finalize (one wave per channel, the arithmetic of bn_finalize_fwd_wide_kernel), apply.
//    Backward: (sum g, sum g * xhat) per (channel, group), then dx / dgamma / dbeta, dy read through the channel offsets.
// 3. AvgPool3d(k, stride 1) (valid windows) for the fine-tune head.
// No float atomics; every reduction has a fixed order.  The only atomics are the integer maxima of the absmax cells.
#include "common.h"

namespace cstp {
namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// SAME max-pool
// ---------------------------------------------------------------------------------------------------------------------------
struct PoolGeom {
  int D, H, W, Do, Ho, Wo;
  int kd, kh, kw, sd, sh, sw;
  int fd, fh, fw;        // front padding
  int pD, pH, pW;        // padded extents
};

constexpr int POOL_LDS_FLOATS = 12288;     // 48 KiB of staged input per block
constexpr int POOL_PAD_WON = -1;           // argmax value when a padding zero is the maximum

// one output element; `src` is the (n, c) volume, in LDS or in global memory.  K3S1: the 3x3x3 / stride 1 pool of the Mixed blocks
// (front padding 1, no window beyond the padded extent) with constant trip counts (the compiler unrolls its 27 taps); otherwise the geometry is read from `g`
template <bool K3S1>
__device__ __forceinline__ void pool_same_one(const float* src, const PoolGeom& g, int od, int oh, int ow, float& best, int& bi) {
  const int kd = K3S1 ? 3 : g.kd, kh = K3S1 ? 3 : g.kh, kw = K3S1 ? 3 : g.kw;
  const int sd = K3S1 ? 1 : g.sd, sh = K3S1 ? 1 : g.sh, sw = K3S1 ? 1 : g.sw;
  const int fd = K3S1 ? 1 : g.fd, fh = K3S1 ? 1 : g.fh, fw = K3S1 ? 1 : g.fw;
  best = 0.f;
  bi = -2;               // no candidate yet
  for (int a = 0; a < kd; ++a) {
    const int pd = od * sd + a;
    if (!K3S1 && pd >= g.pD) break;
    const int id = pd - fd;
    const bool din = (unsigned)id < (unsigned)g.D;
    for (int b = 0; b < kh; ++b) {
      const int ph = oh * sh + b;
      if (!K3S1 && ph >= g.pH) break;
      const int ih = ph - fh;
      const bool hin = din && (unsigned)ih < (unsigned)g.H;
      for (int c = 0; c < kw; ++c) {
        const int pw = ow * sw + c;
        if (!K3S1 && pw >= g.pW) break;
        const int iw = pw - fw;
        const bool in = hin && (unsigned)iw < (unsigned)g.W;
        const int fi = in ? (id * g.H + ih) * g.W + iw : POOL_PAD_WON;
        const float v = in ? src[fi] : 0.f;
        if (v > best || v != v || bi == -2) { best = v; bi = fi; }
      }
    }
  }
}

// R consecutive (n, c) volumes per block, staged in LDS
template <bool K3S1>
__global__ void __launch_bounds__(256) pool_same_lds_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            int32_t* __restrict__ idx, int rows, int R, PoolGeom g) {
  extern __shared__ float tile[];
  const int vol = g.D * g.H * g.W, ovol = g.Do * g.Ho * g.Wo;
  const int r0 = blockIdx.x * R;
  const int nr = rows - r0 < R ? rows - r0 : R;
  const float* xp = x + (size_t)r0 * vol;
  for (int i = threadIdx.x; i < nr * vol; i += 256) tile[i] = xp[i];
  __syncthreads();
  for (int o = threadIdx.x; o < nr * ovol; o += 256) {
    const int r = o / ovol;
    int q = o - r * ovol;
    const int ow = q % g.Wo; q /= g.Wo;
    const int oh = q % g.Ho;
    const int od = q / g.Ho;
    float best;
    int bi;
    pool_same_one<K3S1>(tile + r * vol, g, od, oh, ow, best, bi);
    const size_t dst = (size_t)r0 * ovol + o;
    y[dst] = best;
    if (idx != nullptr) idx[dst] = bi;
  }
}

__global__ void __launch_bounds__(256) pool_same_direct_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               int32_t* __restrict__ idx, int rows, PoolGeom g) {
  const size_t ovol = (size_t)g.Do * g.Ho * g.Wo, total = (size_t)rows * ovol;
  const size_t vol = (size_t)g.D * g.H * g.W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    size_t r = i;
    const int ow = (int)(r % g.Wo); r /= g.Wo;
    const int oh = (int)(r % g.Ho); r /= g.Ho;
    const int od = (int)(r % g.Do);
    const size_t row = r / g.Do;
    float best;
    int bi;
    pool_same_one<false>(x + row * vol, g, od, oh, ow, best, bi);
    y[i] = best;
    if (idx != nullptr) idx[i] = bi;
  }
}

// backward as a gather: dx[p] = sum of dy over the windows that cover p and whose argmax is p (a padding zero that won keeps
// POOL_PAD_WON, which no input element matches: its gradient is dropped)
template <bool K3S1>
__global__ void __launch_bounds__(256) pool_same_bwd_kernel(const float* __restrict__ dy, const int32_t* __restrict__ idx,
                                                            float* __restrict__ dx, int rows, PoolGeom gg) {
  PoolGeom g = gg;
  if (K3S1) { g.kd = g.kh = g.kw = 3; g.sd = g.sh = g.sw = 1; g.fd = g.fh = g.fw = 1; }      // constants: the divisions fold away
  const size_t vol = (size_t)g.D * g.H * g.W, total = (size_t)rows * vol;
  const size_t ovol = (size_t)g.Do * g.Ho * g.Wo;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    size_t r = i;
    const int w = (int)(r % g.W); r /= g.W;
    const int h = (int)(r % g.H); r /= g.H;
    const int d = (int)(r % g.D);
    const size_t row = r / g.D;
    const int fi = (d * g.H + h) * g.W + w;
    const int pd = d + g.fd, ph = h + g.fh, pw = w + g.fw;     // padded coordinates; windows o with o*s <= p <= o*s + k - 1
    const int d_lo = pd - g.kd + g.sd > 0 ? (pd - g.kd + g.sd) / g.sd : 0, d_hi = pd / g.sd < g.Do - 1 ? pd / g.sd : g.Do - 1;
    const int h_lo = ph - g.kh + g.sh > 0 ? (ph - g.kh + g.sh) / g.sh : 0, h_hi = ph / g.sh < g.Ho - 1 ? ph / g.sh : g.Ho - 1;
    const int w_lo = pw - g.kw + g.sw > 0 ? (pw - g.kw + g.sw) / g.sw : 0, w_hi = pw / g.sw < g.Wo - 1 ? pw / g.sw : g.Wo - 1;
    const size_t obase = row * ovol;
    float acc = 0.f;
    for (int a = d_lo; a <= d_hi; ++a)
      for (int b = h_lo; b <= h_hi; ++b)
        for (int c = w_lo; c <= w_hi; ++c) {
          const size_t o = obase + ((size_t)a * g.Ho + b) * g.Wo + c;
          if (idx[o] == fi) acc += dy[o];
        }
    dx[i] = acc;
  }
}

// ... the same gather with the argmax and dy of R consecutive (n, c) volumes staged in LDS (every pooling of the Mixed stages):
// the up to 27 (idx, dy) pairs an input element looks at are LDS reads; HBM sees each of idx, dy once and dx once
template <bool K3S1>
__global__ void __launch_bounds__(256) pool_same_bwd_lds_kernel(const float* __restrict__ dy, const int32_t* __restrict__ idx,
                                                                float* __restrict__ dx, int rows, int R, PoolGeom gg) {
  extern __shared__ float tile[];
  PoolGeom g = gg;
  if (K3S1) { g.kd = g.kh = g.kw = 3; g.sd = g.sh = g.sw = 1; g.fd = g.fh = g.fw = 1; }
  const int vol = g.D * g.H * g.W, ovol = g.Do * g.Ho * g.Wo;
  const int r0 = blockIdx.x * R;
  const int nr = rows - r0 < R ? rows - r0 : R;
  float* sdy = tile;
  int* sidx = reinterpret_cast<int*>(tile + R * ovol);
  const float* gp = dy + (size_t)r0 * ovol;
  const int32_t* ip = idx + (size_t)r0 * ovol;
  for (int i = threadIdx.x; i < nr * ovol; i += 256) { sdy[i] = gp[i]; sidx[i] = ip[i]; }
  __syncthreads();
  for (int i = threadIdx.x; i < nr * vol; i += 256) {
    const int r = i / vol;
    const int fi = i - r * vol;
    int q = fi;
    const int w = q % g.W; q /= g.W;
    const int h = q % g.H;
    const int d = q / g.H;
    const int pd = d + g.fd, ph = h + g.fh, pw = w + g.fw;
    const int d_lo = pd - g.kd + g.sd > 0 ? (pd - g.kd + g.sd) / g.sd : 0, d_hi = pd / g.sd < g.Do - 1 ? pd / g.sd : g.Do - 1;
    const int h_lo = ph - g.kh + g.sh > 0 ? (ph - g.kh + g.sh) / g.sh : 0, h_hi = ph / g.sh < g.Ho - 1 ? ph / g.sh : g.Ho - 1;
    const int w_lo = pw - g.kw + g.sw > 0 ? (pw - g.kw + g.sw) / g.sw : 0, w_hi = pw / g.sw < g.Wo - 1 ? pw / g.sw : g.Wo - 1;
    const int obase = r * ovol;
    float acc = 0.f;
    for (int a = d_lo; a <= d_hi; ++a)
      for (int b = h_lo; b <= h_hi; ++b)
        for (int c = w_lo; c <= w_hi; ++c) {            // the order of pool_same_bwd_kernel: the same sum, bit for bit
          const int o = obase + (a * g.Ho + b) * g.Wo + c;
          if (sidx[o] == fi) acc += sdy[o];
        }
    dx[(size_t)r0 * vol + i] = acc;
  }
}

inline int same_out(int n, int k, int s, int* front, int* padded) {
  const int pad = k - s > 0 ? k - s : 0;
  *front = pad / 2;
  *padded = n + pad;
  int o = (n + pad - k + s - 1) / s + 1;   // n + pad - k >= 1 - s: the numerator is never negative
  if ((o - 1) * s >= n + pad) --o;       // the last window must start inside the padded tensor (ATen's ceil-mode rule)
  return o;
}

int make_pool(int d, int h, int w, const int32_t* k, const int32_t* st, PoolGeom* g) {
  CSTP_REQUIRE(k != nullptr && st != nullptr && d > 0 && h > 0 && w > 0, "bad pooling geometry");
  for (int i = 0; i < 3; ++i) CSTP_REQUIRE(k[i] > 0 && st[i] > 0 && k[i] <= 64 && st[i] <= 64, "bad pooling geometry");
  g->D = d; g->H = h; g->W = w;
  g->kd = k[0]; g->kh = k[1]; g->kw = k[2];
  g->sd = st[0]; g->sh = st[1]; g->sw = st[2];
  g->Do = same_out(d, k[0], st[0], &g->fd, &g->pD);
  g->Ho = same_out(h, k[1], st[1], &g->fh, &g->pH);
  g->Wo = same_out(w, k[2], st[2], &g->fw, &g->pW);
  CSTP_REQUIRE(g->Do > 0 && g->Ho > 0 && g->Wo > 0, "bad pooling geometry");
  CSTP_REQUIRE((size_t)d * h * w < (1ull << 31) && (size_t)g->Do * g->Ho * g->Wo < (1ull << 31), "plane too large for int32 argmax");
  return 0;
}

inline bool pool_k3s1(const PoolGeom& g) {
  return g.kd == 3 && g.kh == 3 && g.kw == 3 && g.sd == 1 && g.sh == 1 && g.sw == 1;
}

inline unsigned flat_grid(size_t total) {
  const size_t b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > (1u << 20) ? (1u << 20) : b));
}

// ---------------------------------------------------------------------------------------------------------------------------
// AvgPool3d(k, stride 1), valid windows
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) avgwin_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int D,
                                                         int H, int W, int kd, int kh, int kw) {
  const int Do = D - kd + 1, Ho = H - kh + 1, Wo = W - kw + 1;
  const size_t total = (size_t)rows * Do * Ho * Wo;
  const float inv = 1.f / (float)(kd * kh * kw);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    size_t r = i;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho); r /= Ho;
    const int od = (int)(r % Do);
    const float* xp = x + (r / Do) * (size_t)D * H * W;
    float acc = 0.f;
    for (int a = 0; a < kd; ++a)
      for (int b = 0; b < kh; ++b)
        for (int c = 0; c < kw; ++c) acc += xp[((od + a) * H + oh + b) * W + ow + c];
    y[i] = acc * inv;
  }
}

__global__ void __launch_bounds__(256) avgwin_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int rows, int D,
                                                         int H, int W, int kd, int kh, int kw) {
  const int Do = D - kd + 1, Ho = H - kh + 1, Wo = W - kw + 1;
  const size_t total = (size_t)rows * D * H * W;
  const float inv = 1.f / (float)(kd * kh * kw);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    size_t r = i;
    const int w = (int)(r % W); r /= W;
    const int h = (int)(r % H); r /= H;
    const int d = (int)(r % D);
    const float* gp = dy + (r / D) * (size_t)Do * Ho * Wo;
    const int d_lo = d - kd + 1 > 0 ? d - kd + 1 : 0, d_hi = d < Do - 1 ? d : Do - 1;
    const int h_lo = h - kh + 1 > 0 ? h - kh + 1 : 0, h_hi = h < Ho - 1 ? h : Ho - 1;
    const int w_lo = w - kw + 1 > 0 ? w - kw + 1 : 0, w_hi = w < Wo - 1 ? w : Wo - 1;
    float acc = 0.f;
    for (int a = d_lo; a <= d_hi; ++a)
      for (int b = h_lo; b <= h_hi; ++b)
        for (int c = w_lo; c <= w_hi; ++c) acc += gp[(a * Ho + b) * Wo + c];
    dx[i] = acc * inv;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// BatchNorm + ReLU into the concat
// ---------------------------------------------------------------------------------------------------------------------------
struct BncSet {
  cstp_bnc_branch br[CSTP_BNC_MAX_BRANCHES];
  int off[CSTP_BNC_MAX_BRANCHES + 1];    // channel offsets in the concat tensor; off[nb] = C
  int nb;
};

__device__ __forceinline__ int bnc_branch(const BncSet& bs, int ch) {
  int i = 0;
#pragma unroll
  for (int j = 1; j < CSTP_BNC_MAX_BRANCHES; ++j)
    if (j < bs.nb && ch >= bs.off[j]) i = j;
  return i;
}

__device__ __forceinline__ unsigned bnc_umax(unsigned a, unsigned b) { return a > b ? a : b; }

constexpr int BNC_WAVES = 4;
constexpr int BNC_APPLY_MAX_BLOCKS = 2048;

// ---- forward 0 (only when a branch brings no sums): (sum x, sum x^2) per (channel, group), one block each, fp64, fixed order
__global__ void __launch_bounds__(256) bnc_stats_kernel(BncSet bs, int npg, int s, int groups, double* __restrict__ part) {
  __shared__ double sm[16];
  const int ch = blockIdx.x, grp = blockIdx.y;
  const int i = bnc_branch(bs, ch);
  if (bs.br[i].part != nullptr) return;          // block-uniform: the convolution left this branch's sums
  const int c = bs.br[i].c, k = ch - bs.off[i];
  double a0 = 0.0, a1 = 0.0;
  // thread t takes elements t, t + 256, ... of the group's npg * s values (the samples' rows back to back): at the small maps
  // (s = 32) all 256 lanes work instead of 32, and the samples are not walked one after the other
  const float* xb = bs.br[i].x + ((size_t)grp * npg * c + k) * s;
  const size_t rstride = (size_t)c * s;
  for (int e = threadIdx.x; e < npg * s; e += 256) {
    const int rr = e / s, j = e - rr * s;
    const float v = xb[rr * rstride + j];
    a0 += (double)v;
    a1 += (double)v * v;
  }
  a0 = block_sum(a0, sm);
  a1 = block_sum(a1, sm);
  if (threadIdx.x == 0) {
    part[((size_t)ch * groups + grp) * 2 + 0] = a0;
    part[((size_t)ch * groups + grp) * 2 + 1] = a1;
  }
}

// ---- forward 1: one wave per concat channel folds the partial sums -- the convolution's (around its pivot) or the ones above
//      -- in the order and with the arithmetic of bn_finalize_fwd_wide_kernel; zeroes the absmax cell
__global__ void __launch_bounds__(64) bnc_finalize_kernel(BncSet bs, int ctot, int groups, double count, float eps,
                                                          float momentum, const double* __restrict__ own,
                                                          float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                          float2* __restrict__ ss, unsigned* __restrict__ cell) {
  const int ch = blockIdx.x, lane = threadIdx.x;
  if (ch == 0 && lane == 0 && cell != nullptr) *cell = 0;
  const int i = bnc_branch(bs, ch);
  const cstp_bnc_branch& b = bs.br[i];
  const int c = b.c, k = ch - bs.off[i];
  const bool pre = b.part != nullptr;
  const int nsplit = pre ? b.nsplit : 1;
  const double pivot = pre ? b.part[(size_t)c * groups * nsplit * 2 + k] : 0.0;
  float rm = 0.f, rv = 0.f;
  if (b.running_mean != nullptr) { rm = b.running_mean[k]; rv = b.running_var[k]; }
  const float ga = b.gamma[k], be = b.beta[k];
  for (int g = 0; g < groups; ++g) {
    double s0 = 0.0, s1 = 0.0;
    const double* p = pre ? b.part + ((size_t)k * groups + g) * nsplit * 2 : own + ((size_t)ch * groups + g) * 2;
    for (int j = lane; j < nsplit; j += 64) { s0 += p[2 * j]; s1 += p[2 * j + 1]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
    const double dm = s0 / count;
    const double mu = pivot + dm;
    double var = s1 / count - dm * dm;
    if (var < 0.0) var = 0.0;
    const float isf = (float)(1.0 / sqrt(var + (double)eps));
    if (lane == 0) {
      save_mean[g * ctot + ch] = (float)mu;
      save_invstd[g * ctot + ch] = isf;
      const float scl = isf * ga;
      ss[g * ctot + ch] = make_float2(scl, be - (float)mu * scl);
    }
    const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
    rm = (float)((1.0 - momentum) * rm + momentum * mu);      // group after group, like successive calls
    rv = (float)((1.0 - momentum) * rv + momentum * unb);
  }
  if (lane == 0 && b.running_mean != nullptr) { b.running_mean[k] = rm; b.running_var[k] = rv; }
}

// eval mode: the running statistics are the statistics (bn_eval_prepare_kernel + bn_apply_fwd_kernel's table)
__global__ void __launch_bounds__(64) bnc_eval_table_kernel(BncSet bs, int ctot, float eps, float2* __restrict__ ss,
                                                            unsigned* __restrict__ cell) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  if (ch == 0 && cell != nullptr) *cell = 0;
  if (ch >= ctot) return;
  const int i = bnc_branch(bs, ch);
  const int k = ch - bs.off[i];
  const float is = 1.0f / sqrtf(bs.br[i].running_var[k] + eps);
  const float sc = is * bs.br[i].gamma[k];
  ss[ch] = make_float2(sc, bs.br[i].beta[k] - bs.br[i].running_mean[k] * sc);
}

// ---- forward 2: y[n][off_i + k][:] = relu(x_i * scale + shift), one wave per (sample, channel) row
template <bool VEC4>
__global__ void __launch_bounds__(256) bnc_apply_kernel(BncSet bs, int rows, int ctot, int s, int npg,
                                                        const float2* __restrict__ ss, float* __restrict__ y,
                                                        unsigned* __restrict__ cell) {
  __shared__ unsigned red[BNC_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mx = 0;
  for (int r = blockIdx.x * BNC_WAVES + wave; r < rows; r += gridDim.x * BNC_WAVES) {
    const int ns = r / ctot, ch = r - ns * ctot;
    const int i = bnc_branch(bs, ch);
    const int c = bs.br[i].c, k = ch - bs.off[i];
    const float2 t2 = ss[(ns / npg) * ctot + ch];
    const float sc = t2.x, sh = t2.y;
    const float* x = bs.br[i].x + ((size_t)ns * c + k) * s;
    float* yr = y + (size_t)r * s;
    if (VEC4) {
      const float4* x4 = reinterpret_cast<const float4*>(x);
      float4* y4 = reinterpret_cast<float4*>(yr);
      for (int j = lane; j < (s >> 2); j += 64) {
        float4 v = x4[j];
        v.x = v.x * sc + sh; v.y = v.y * sc + sh; v.z = v.z * sc + sh; v.w = v.w * sc + sh;
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        y4[j] = v;
        mx = bnc_umax(mx, bnc_umax(bnc_umax(abs_bits(v.x), abs_bits(v.y)), bnc_umax(abs_bits(v.z), abs_bits(v.w))));
      }
    } else {
      for (int j = lane; j < s; j += 64) {
        float v = x[j] * sc + sh;
        v = fmaxf(v, 0.f);
        yr[j] = v;
        mx = bnc_umax(mx, abs_bits(v));
      }
    }
  }
  if (cell == nullptr) return;        // grid-uniform
  mx = wave_umax(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned a = bnc_umax(bnc_umax(red[0], red[1]), bnc_umax(red[2], red[3]));
    if (a != 0) atomicMax(cell, a);
  }
}

// ---- backward 1: (sum g, sum g * xhat) per (channel, group), g = dy masked by relu'(x * scale + shift); fp64, fixed order
__global__ void __launch_bounds__(256) bnc_bwd_reduce_kernel(BncSet bs, int ctot, int npg, int s, int groups,
                                                             const float* __restrict__ dy, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float2* __restrict__ ss,
                                                             double* __restrict__ part) {
  __shared__ double sm[16];
  const int ch = blockIdx.x, grp = blockIdx.y;
  const int i = bnc_branch(bs, ch);
  const int c = bs.br[i].c, k = ch - bs.off[i];
  if (ch == 0 && grp == 0 && threadIdx.x < bs.nb && bs.br[threadIdx.x].dx_absmax != nullptr) *bs.br[threadIdx.x].dx_absmax = 0;
  const int gc = grp * ctot + ch;
  const float mu = mean[gc], is = invstd[gc];
  const float2 t2 = ss[gc];
  const float sc = t2.x, sh = t2.y;
  double a0 = 0.0, a1 = 0.0;
  const float* xb = bs.br[i].x + ((size_t)grp * npg * c + k) * s;
  const float* gb = dy + ((size_t)grp * npg * ctot + ch) * s;
  const size_t xstride = (size_t)c * s, gstride = (size_t)ctot * s;
  for (int e = threadIdx.x; e < npg * s; e += 256) {          // flattened (sample, position), as bnc_stats_kernel
    const int rr = e / s, j = e - rr * s;
    const float v = xb[rr * xstride + j];
    float g = gb[rr * gstride + j];
    if (!((v * sc + sh) > 0.f)) g = 0.f;
    a0 += (double)g;
    a1 += (double)(g * ((v - mu) * is));
  }
  a0 = block_sum(a0, sm);
  a1 = block_sum(a1, sm);
  if (threadIdx.x == 0) {
    part[(size_t)gc * 2 + 0] = a0;
    part[(size_t)gc * 2 + 1] = a1;
  }
}

// ---- backward 2: dx_i = gamma * invstd * (g - sum_g / cnt - xhat * sum_gx / cnt); the wave of a channel's first row also
//      writes (or adds) dgamma / dbeta, summed over the groups in group order
template <bool VEC4>
__global__ void __launch_bounds__(256) bnc_bwd_apply_kernel(BncSet bs, int rows, int ctot, int s, int npg, int groups,
                                                            float inv_count, const float* __restrict__ dy,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float2* __restrict__ ss, const double* __restrict__ part,
                                                            int accumulate) {
  __shared__ unsigned red[BNC_WAVES][CSTP_BNC_MAX_BRANCHES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mx[CSTP_BNC_MAX_BRANCHES] = {0, 0, 0, 0};
  for (int r = blockIdx.x * BNC_WAVES + wave; r < rows; r += gridDim.x * BNC_WAVES) {
    const int ns = r / ctot, ch = r - ns * ctot;
    const int i = bnc_branch(bs, ch);
    const int c = bs.br[i].c, k = ch - bs.off[i];
    const int gc = (ns / npg) * ctot + ch;
    if (ns == 0 && lane == 0) {
      double t0 = 0.0, t1 = 0.0;
      for (int g = 0; g < groups; ++g) { t0 += part[((size_t)g * ctot + ch) * 2]; t1 += part[((size_t)g * ctot + ch) * 2 + 1]; }
      float* db = bs.br[i].dbeta + k;
      float* dg = bs.br[i].dgamma + k;
      *db = (accumulate ? *db : 0.f) + (float)t0;
      *dg = (accumulate ? *dg : 0.f) + (float)t1;
    }
    const float sum_g = (float)part[(size_t)gc * 2], sum_gx = (float)part[(size_t)gc * 2 + 1];
    const float mu = mean[gc], is = invstd[gc];
    const float kk = bs.br[i].gamma[k] * is;
    const float mb = sum_g * inv_count, mg = sum_gx * inv_count;
    const float2 t2 = ss[gc];
    const float sc = t2.x, sh = t2.y;
    const float* x = bs.br[i].x + ((size_t)ns * c + k) * s;
    const float* gp = dy + (size_t)r * s;
    float* dx = bs.br[i].dx + ((size_t)ns * c + k) * s;
    unsigned m = 0;
    if (VEC4) {
      const float4* x4 = reinterpret_cast<const float4*>(x);
      const float4* g4 = reinterpret_cast<const float4*>(gp);
      float4* o4 = reinterpret_cast<float4*>(dx);
      for (int j = lane; j < (s >> 2); j += 64) {
        const float4 v = x4[j];
        float4 g = g4[j];
        g.x = (v.x * sc + sh) > 0.f ? g.x : 0.f; g.y = (v.y * sc + sh) > 0.f ? g.y : 0.f;
        g.z = (v.z * sc + sh) > 0.f ? g.z : 0.f; g.w = (v.w * sc + sh) > 0.f ? g.w : 0.f;
        float4 o;
        o.x = kk * (g.x - mb - (v.x - mu) * is * mg);
        o.y = kk * (g.y - mb - (v.y - mu) * is * mg);
        o.z = kk * (g.z - mb - (v.z - mu) * is * mg);
        o.w = kk * (g.w - mb - (v.w - mu) * is * mg);
        o4[j] = o;
        m = bnc_umax(m, bnc_umax(bnc_umax(abs_bits(o.x), abs_bits(o.y)), bnc_umax(abs_bits(o.z), abs_bits(o.w))));
      }
    } else {
      for (int j = lane; j < s; j += 64) {
        const float v = x[j];
        float g = gp[j];
        if (!((v * sc + sh) > 0.f)) g = 0.f;
        const float o = kk * (g - mb - (v - mu) * is * mg);
        dx[j] = o;
        m = bnc_umax(m, abs_bits(o));
      }
    }
#pragma unroll
    for (int j = 0; j < CSTP_BNC_MAX_BRANCHES; ++j)
      if (j == i) mx[j] = bnc_umax(mx[j], m);
  }
#pragma unroll
  for (int j = 0; j < CSTP_BNC_MAX_BRANCHES; ++j) {
    const unsigned a = wave_umax(mx[j]);
    if (lane == 0) red[wave][j] = a;
  }
  __syncthreads();
  if (threadIdx.x < bs.nb) {
    const int j = threadIdx.x;
    const unsigned a = bnc_umax(bnc_umax(red[0][j], red[1][j]), bnc_umax(red[2][j], red[3][j]));
    if (a != 0 && bs.br[j].dx_absmax != nullptr) atomicMax(bs.br[j].dx_absmax, a);
  }
}


// mode 0: train forward, 1: eval forward, 2: backward
int make_bnc(const cstp_bnc_branch* br, int nb, int n, int s, int groups, int mode, BncSet* bs, bool* vec4, bool* need_stats) {
  CSTP_REQUIRE(br != nullptr && nb >= 1 && nb <= CSTP_BNC_MAX_BRANCHES, "bad branch table");
  CSTP_REQUIRE(n > 0 && s > 0 && groups > 0 && (n % groups) == 0, "bad shape");
  memset(bs, 0, sizeof(*bs));
  bs->nb = nb;
  bool v = (s & 3) == 0, need = false;
  long ctot = 0;
  for (int i = 0; i < nb; ++i) {
    const cstp_bnc_branch& b = br[i];
    CSTP_REQUIRE(b.x != nullptr && b.gamma != nullptr && b.c > 0, "null argument");
    if (mode != 2) CSTP_REQUIRE(b.beta != nullptr, "null argument");      // backward does not read beta
    CSTP_REQUIRE((b.running_mean == nullptr) == (b.running_var == nullptr), "running stats must come as a pair");
    if (mode == 1) CSTP_REQUIRE(b.running_mean != nullptr, "eval mode needs the running statistics");
    if (mode == 2) CSTP_REQUIRE(b.dx != nullptr && b.dgamma != nullptr && b.dbeta != nullptr, "null argument");
    if (mode == 0 && b.part != nullptr) CSTP_REQUIRE(b.nsplit > 0, "partial sums without their split count");
    if (mode == 0 && b.part == nullptr) need = true;
    v = v && al16(b.x) && (mode != 2 || al16(b.dx));
    bs->br[i] = b;
    bs->off[i] = (int)ctot;
    ctot += b.c;
  }
  CSTP_REQUIRE(ctot * n < (1L << 31) && ctot * groups < 65536L * 16 && groups < 65536, "tensor too large");
  for (int i = nb; i <= CSTP_BNC_MAX_BRANCHES; ++i) bs->off[i] = (int)ctot;
  *vec4 = v;
  *need_stats = need;
  return 0;
}

inline unsigned bnc_apply_grid(int rows) {
  const int b = cdiv(rows, BNC_WAVES);
  return (unsigned)(b < BNC_APPLY_MAX_BLOCKS ? b : BNC_APPLY_MAX_BLOCKS);
}

}  // namespace
}  // namespace cstp

using namespace cstp;

extern "C" int cstp_maxpool3d_same_out(int32_t n, int32_t k, int32_t s) {
  if (n <= 0 || k <= 0 || s <= 0) return 0;
  int f, p;
  return same_out(n, k, s, &f, &p);
}

extern "C" int cstp_maxpool3d_same_forward(void* stream, const float* x, float* y, int32_t* argmax, int32_t rows, int32_t d,
                                           int32_t h, int32_t w, const int32_t* kernel3, const int32_t* stride3) {
  CSTP_REQUIRE(x && y && rows > 0, "bad argument");
  PoolGeom g;
  if (make_pool(d, h, w, kernel3, stride3, &g)) return 1;
  const size_t vol = (size_t)d * h * w, ovol = (size_t)g.Do * g.Ho * g.Wo;
  hipStream_t st = as_stream(stream);
  if (vol <= (size_t)POOL_LDS_FLOATS) {
    // several small volumes per block: at least ~2048 staged values where the batch allows it
    int R = (int)(2048 / vol);
    if (R < 1) R = 1;
    if (R > rows) R = rows;
    if (pool_k3s1(g))
      hipLaunchKernelGGL(pool_same_lds_kernel<true>, dim3(cdiv(rows, R)), dim3(256), (size_t)R * vol * sizeof(float), st, x, y,
                         argmax, rows, R, g);
    else
      hipLaunchKernelGGL(pool_same_lds_kernel<false>, dim3(cdiv(rows, R)), dim3(256), (size_t)R * vol * sizeof(float), st, x, y,
                         argmax, rows, R, g);
  } else {
    hipLaunchKernelGGL(pool_same_direct_kernel, dim3(flat_grid((size_t)rows * ovol)), dim3(256), 0, st, x, y, argmax, rows, g);
  }
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_maxpool3d_same_backward(void* stream, const float* dy, const int32_t* argmax, float* dx, int32_t rows,
                                            int32_t d, int32_t h, int32_t w, const int32_t* kernel3, const int32_t* stride3) {
  CSTP_REQUIRE(dy && argmax && dx && rows > 0, "bad argument");
  PoolGeom g;
  if (make_pool(d, h, w, kernel3, stride3, &g)) return 1;
  const size_t vol = (size_t)d * h * w, ovol = (size_t)g.Do * g.Ho * g.Wo;
  if (2 * ovol <= (size_t)POOL_LDS_FLOATS) {
    // several small volumes per block, as in the forward: at least ~2048 input elements where the batch allows it
    int R = (int)(2048 / vol);
    if (R < 1) R = 1;
    if ((size_t)R * 2 * ovol > (size_t)POOL_LDS_FLOATS) R = (int)((size_t)POOL_LDS_FLOATS / (2 * ovol));
    if (R > rows) R = rows;
    const size_t lds = (size_t)R * ovol * (sizeof(float) + sizeof(int32_t));
    if (pool_k3s1(g))
      hipLaunchKernelGGL(pool_same_bwd_lds_kernel<true>, dim3(cdiv(rows, R)), dim3(256), lds, as_stream(stream), dy, argmax, dx,
                         rows, R, g);
    else
      hipLaunchKernelGGL(pool_same_bwd_lds_kernel<false>, dim3(cdiv(rows, R)), dim3(256), lds, as_stream(stream), dy, argmax, dx,
                         rows, R, g);
    CSTP_LAUNCH_CHECK();
    return 0;
  }
  const dim3 grid(flat_grid((size_t)rows * d * h * w));
  if (pool_k3s1(g)) hipLaunchKernelGGL(pool_same_bwd_kernel<true>, grid, dim3(256), 0, as_stream(stream), dy, argmax, dx, rows, g);
  else hipLaunchKernelGGL(pool_same_bwd_kernel<false>, grid, dim3(256), 0, as_stream(stream), dy, argmax, dx, rows, g);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_avgpool3d_window_forward(void* stream, const float* x, float* y, int32_t rows, int32_t d, int32_t h,
                                             int32_t w, const int32_t* kernel3) {
  CSTP_REQUIRE(x && y && kernel3 && rows > 0 && d > 0 && h > 0 && w > 0, "bad argument");
  CSTP_REQUIRE(kernel3[0] > 0 && kernel3[1] > 0 && kernel3[2] > 0 && kernel3[0] <= d && kernel3[1] <= h && kernel3[2] <= w,
               "average-pool window larger than its input");
  CSTP_REQUIRE((size_t)d * h * w < (1ull << 31), "plane too large");
  const size_t total = (size_t)rows * (d - kernel3[0] + 1) * (h - kernel3[1] + 1) * (w - kernel3[2] + 1);
  hipLaunchKernelGGL(avgwin_fwd_kernel, dim3(flat_grid(total)), dim3(256), 0, as_stream(stream), x, y, rows, d, h, w, kernel3[0],
                     kernel3[1], kernel3[2]);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_avgpool3d_window_backward(void* stream, const float* dy, float* dx, int32_t rows, int32_t d, int32_t h,
                                              int32_t w, const int32_t* kernel3) {
  CSTP_REQUIRE(dy && dx && kernel3 && rows > 0 && d > 0 && h > 0 && w > 0, "bad argument");
  CSTP_REQUIRE(kernel3[0] > 0 && kernel3[1] > 0 && kernel3[2] > 0 && kernel3[0] <= d && kernel3[1] <= h && kernel3[2] <= w,
               "average-pool window larger than its input");
  CSTP_REQUIRE((size_t)d * h * w < (1ull << 31), "plane too large");
  hipLaunchKernelGGL(avgwin_bwd_kernel, dim3(flat_grid((size_t)rows * d * h * w)), dim3(256), 0, as_stream(stream), dy, dx, rows, d,
                     h, w, kernel3[0], kernel3[1], kernel3[2]);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cstp_bnrelu_concat_workspace_bytes(int32_t ctot, int32_t groups) {
  if (ctot <= 0 || groups <= 0) return 0;
  return align_up((size_t)ctot * groups * 2 * sizeof(double), 256);      // [C][groups][2] (forward) / [groups][C][2] (backward)
}

extern "C" int cstp_bnrelu_concat_forward(void* stream, const cstp_bnc_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                                          int32_t groups, float eps, float momentum, float* y, float* save_mean,
                                          float* save_invstd, float* scale_shift, void* ws, size_t ws_bytes, uint32_t* y_absmax) {
  BncSet bs;
  bool v4 = false, need = false;
  if (make_bnc(branches, nbranch, n, s, groups, 0, &bs, &v4, &need)) return 1;
  CSTP_REQUIRE(y != nullptr && save_mean != nullptr && save_invstd != nullptr && scale_shift != nullptr, "null argument");
  const int npg = n / groups;
  CSTP_REQUIRE((size_t)npg * s > 1, "train-mode BatchNorm needs more than 1 value per channel");
  const int ctot = bs.off[bs.nb], rows = n * ctot;
  v4 = v4 && al16(y);
  hipStream_t st = as_stream(stream);
  double* own = reinterpret_cast<double*>(ws);
  if (need) {
    CSTP_REQUIRE(ws != nullptr && ws_bytes >= cstp_bnrelu_concat_workspace_bytes(ctot, groups), "workspace too small");
    hipLaunchKernelGGL(bnc_stats_kernel, dim3(ctot, groups), dim3(256), 0, st, bs, npg, s, groups, own);
    CSTP_LAUNCH_CHECK();
  }
  float2* ss = reinterpret_cast<float2*>(scale_shift);
  hipLaunchKernelGGL(bnc_finalize_kernel, dim3(ctot), dim3(64), 0, st, bs, ctot, groups, (double)npg * s, eps, momentum, own,
                     save_mean, save_invstd, ss, y_absmax);
  CSTP_LAUNCH_CHECK();
  if (v4) hipLaunchKernelGGL(bnc_apply_kernel<true>, dim3(bnc_apply_grid(rows)), dim3(256), 0, st, bs, rows, ctot, s, npg, ss, y, y_absmax);
  else hipLaunchKernelGGL(bnc_apply_kernel<false>, dim3(bnc_apply_grid(rows)), dim3(256), 0, st, bs, rows, ctot, s, npg, ss, y, y_absmax);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_bnrelu_concat_eval(void* stream, const cstp_bnc_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                                       float eps, float* y, float* scale_shift, uint32_t* y_absmax) {
  BncSet bs;
  bool v4 = false, need = false;
  if (make_bnc(branches, nbranch, n, s, 1, 1, &bs, &v4, &need)) return 1;
  CSTP_REQUIRE(y != nullptr && scale_shift != nullptr, "null argument");
  const int ctot = bs.off[bs.nb], rows = n * ctot;
  v4 = v4 && al16(y);
  hipStream_t st = as_stream(stream);
  float2* ss = reinterpret_cast<float2*>(scale_shift);
  hipLaunchKernelGGL(bnc_eval_table_kernel, dim3(cdiv(ctot, 64)), dim3(64), 0, st, bs, ctot, eps, ss, y_absmax);
  CSTP_LAUNCH_CHECK();
  // one "group" spanning the whole batch: the table is indexed by channel alone
  if (v4) hipLaunchKernelGGL(bnc_apply_kernel<true>, dim3(bnc_apply_grid(rows)), dim3(256), 0, st, bs, rows, ctot, s, n, ss, y, y_absmax);
  else hipLaunchKernelGGL(bnc_apply_kernel<false>, dim3(bnc_apply_grid(rows)), dim3(256), 0, st, bs, rows, ctot, s, n, ss, y, y_absmax);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_bnrelu_concat_backward(void* stream, const cstp_bnc_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                                           int32_t groups, const float* dy, const float* save_mean, const float* save_invstd,
                                           const float* scale_shift, void* ws, size_t ws_bytes, int32_t accumulate) {
  BncSet bs;
  bool v4 = false, need = false;
  if (make_bnc(branches, nbranch, n, s, groups, 2, &bs, &v4, &need)) return 1;
  CSTP_REQUIRE(dy != nullptr && save_mean != nullptr && save_invstd != nullptr && scale_shift != nullptr, "null argument");
  const int npg = n / groups;
  const int ctot = bs.off[bs.nb], rows = n * ctot;
  CSTP_REQUIRE(ws != nullptr && ws_bytes >= cstp_bnrelu_concat_workspace_bytes(ctot, groups), "workspace too small");
  v4 = v4 && al16(dy);
  hipStream_t st = as_stream(stream);
  double* part = reinterpret_cast<double*>(ws);
  const float2* ss = reinterpret_cast<const float2*>(scale_shift);
  hipLaunchKernelGGL(bnc_bwd_reduce_kernel, dim3(ctot, groups), dim3(256), 0, st, bs, ctot, npg, s, groups, dy, save_mean,
                     save_invstd, ss, part);
  CSTP_LAUNCH_CHECK();
  const float inv_count = (float)(1.0 / ((double)npg * s));
  if (v4) hipLaunchKernelGGL(bnc_bwd_apply_kernel<true>, dim3(bnc_apply_grid(rows)), dim3(256), 0, st, bs, rows, ctot, s, npg, groups, inv_count, dy, save_mean, save_invstd, ss, part, accumulate ? 1 : 0);
  else hipLaunchKernelGGL(bnc_bwd_apply_kernel<false>, dim3(bnc_apply_grid(rows)), dim3(256), 0, st, bs, rows, ctot, s, npg, groups, inv_count, dy, save_mean, save_invstd, ss, part, accumulate ? 1 : 0);
  CSTP_LAUNCH_CHECK();
  return 0;
}
