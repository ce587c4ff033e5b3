// NT-Xent with a queue of extra negatives (cstp_ntxq_forward / _backward / _push, spec in include/cstp_hip.h): the loss of
// misc.hip's cstp_ntxent_* with n_valid constant unit rows appended to every row's denominator, without ever building the
// [R][n_valid] score matrix.  Included from retrieve.hip: the walk is simtopk_kernel's (same tiles, same LDS image, same MFMA,
// so a score is the same f32 fmaf chain in feature order whatever tile or split computes it) with another epilogue.
//
//   c_ik = <reps_i, queue_k> / max(|reps_i|, 1e-8)            (the queue's rows are unit length by contract: cstp_ntxq_push)
//   lse_i = log( sum_{j != i} exp(s_ij / T) + sum_{k < n_valid} exp(c_ik / T) )
//
// Forward: cstp_ntxent_forward fills its own workspace block (norms, in-batch sim, in-batch lse); ntxq_fwd_kernel (block = 64
// rows x one contiguous share of the queue tiles) keeps a running (max, sum exp) of c_ik / T per row -- one wave owns 16 rows,
// 128 scores of a row are two per lane -- and writes one pair per (split, row); ntxq_fwd_combine_kernel folds the in-batch row
// and the pairs in split order, overwrites lse in the ntxent block and writes the loss.  The maximum is subtracted everywhere.
// Backward: ntxq_bwd_kernel (grid.z = slices of NQ_FS = 256 features) recomputes a tile's scores, turns them into
// p_ik = exp(c_ik / T - lse_i) in LDS and multiplies P [64][128] by the tile's queue rows [128][slice] on the same MFMA: wave w
// owns features [64 w, 64 w + 64) of the slice, four 32x32 accumulators that live in registers across the whole share.  The
// partial sums [split][R][f] go to the workspace; cstp_ntxent_backward then gives the in-batch gradient with the new lse and
// ntxq_bwd_combine_kernel adds the splits in order through the derivative of the normalisation, scaled by dloss / (R T).
// No atomics.  Every global index is formed from a row < R / < n_valid and a feature < f that were compared first; what is
// masked is a zero operand or a zero probability, never a large negative: queue rows from n_valid on are not read at all.
#pragma once
#include <math.h>

#include "common.h"

namespace cstp {
namespace {

constexpr int NQ_FS = 256;                                  // backward: features per slice (4 waves x 2 x 32)
constexpr int NQ_MAX_F = 2048;
constexpr size_t NQ_PART_FLOATS = (size_t)4 << 20;          // [split][R][f] partial gradients: 16 MiB at the most (or one split)
constexpr int NQ_MAX_SPLIT = 256, NQ_MIN_TILES = 2;         // R <= 64 is one row tile: the queue alone has to fill the CUs

// the logit of a queue score: one expression for forward and backward
__device__ __forceinline__ float nq_logit(float dot, float norm, float inv_t) { return dot / fmaxf(norm, 1e-8f) * inv_t; }

// simtopk_kernel's staging: thread tid holds features 4 (tid & 7) .. + 3 of rows (tid >> 3) + 32 p of a 32-feature chunk
template <bool VEC4, int NP>
__device__ __forceinline__ void nq_load_rows(const float* __restrict__ base, int row0, int nrows, int d, int c0, float4* dst) {
  const int srow = threadIdx.x >> 3, sc4 = (threadIdx.x & 7) * 4;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int row = row0 + srow + 32 * p, c = c0 + sc4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows) {
      const float* src = base + (size_t)row * d + c;
      if (VEC4) {
        if (c < d) v = *reinterpret_cast<const float4*>(src);     // d % 4 == 0: the four features are in or out together
      } else {
        if (c < d) v.x = src[0];
        if (c + 1 < d) v.y = src[1];
        if (c + 2 < d) v.z = src[2];
        if (c + 3 < d) v.w = src[3];
      }
    }
    dst[p] = v;
  }
}

template <int NP>
__device__ __forceinline__ void nq_store_rows(float* dst, int ld, const float4* src) {
  const int srow = threadIdx.x >> 3, sc4 = (threadIdx.x & 7) * 4;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float* o = dst + sc4 * ld + srow + 32 * p;
    o[0] = src[p].x;
    o[ld] = src[p].y;
    o[2 * ld] = src[p].z;
    o[3 * ld] = src[p].w;
  }
}

// The raw dot products of rows [q0, q0 + 64) with queue rows [g0, g0 + 128) into smem as [64][SQ_LDS].  qa / ga hold chunk 0 of
// this tile on entry and chunk 0 of the next tile (if there is one) on exit.  Ends on a barrier: the scores are visible.
template <bool VEC4>
__device__ __forceinline__ void nq_score_tile(float* smem, const float* __restrict__ reps, const float* __restrict__ queue, int R,
                                              int n_valid, int d, int q0, int g0, bool next_tile, float4* qa, float4* ga) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane >> 5, lcol = lane & 31;
  const int nchunk = (d + SQ_BK - 1) / SQ_BK;
  floatx16 acc0 = {0}, acc1 = {0};
  nq_store_rows<2>(smem, SQ_LDA, qa);
  nq_store_rows<4>(smem + SQ_BK * SQ_LDA, SQ_LDB, ga);
  __syncthreads();
  int buf = 0;
  for (int kc = 0; kc < nchunk; ++kc) {
    const bool have_next = kc + 1 < nchunk;
    if (have_next) {
      nq_load_rows<VEC4, 2>(reps, q0, R, d, (kc + 1) * SQ_BK, qa);
      nq_load_rows<VEC4, 4>(queue, g0, n_valid, d, (kc + 1) * SQ_BK, ga);
    } else if (next_tile) {
      nq_load_rows<VEC4, 2>(reps, q0, R, d, 0, qa);
      nq_load_rows<VEC4, 4>(queue, g0 + SQ_TG, n_valid, d, 0, ga);
    }
    const float* Ab = smem + buf * SQ_BUF + lrow * SQ_LDA + lcol;
    const float* Bb = smem + buf * SQ_BUF + SQ_BK * SQ_LDA + lrow * SQ_LDB + wave * 32 + lcol;
#pragma unroll
    for (int kk = 0; kk < SQ_BK; kk += 2) {
      const float b = Bb[kk * SQ_LDB];
      const float a0 = Ab[kk * SQ_LDA], a1 = Ab[kk * SQ_LDA + 32];
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
    }
    if (have_next) {
      float* nb = smem + (buf ^ 1) * SQ_BUF;
      nq_store_rows<2>(nb, SQ_LDA, qa);
      nq_store_rows<4>(nb + SQ_BK * SQ_LDA, SQ_LDB, ga);
    }
    __syncthreads();
    buf ^= 1;
  }
  // every wave is past its last fragment read: the scores go over the operand image
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = (r & 3) + 8 * (r >> 2) + 4 * lrow;
    smem[m * SQ_LDS + wave * 32 + lcol] = acc0[r];
    smem[(m + 32) * SQ_LDS + wave * 32 + lcol] = acc1[r];
  }
  __syncthreads();
}

__device__ __forceinline__ float nq_wave_max_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

template <bool VEC4>
__global__ void __launch_bounds__(256)
ntxq_fwd_kernel(const float* __restrict__ reps, const float* __restrict__ queue, const float* __restrict__ norms, int R,
                int n_valid, int d, float inv_t, int tiles_per_split, float* __restrict__ pm, float* __restrict__ ps) {
  __shared__ float smem[SQ_SMEM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.x * SQ_TQ;
  const int gtiles = (n_valid + SQ_TG - 1) / SQ_TG;
  const int t_begin = blockIdx.y * tiles_per_split;
  const int t_end = t_begin + tiles_per_split < gtiles ? t_begin + tiles_per_split : gtiles;

  float rm[16], rs[16], rn[16];                      // wave-uniform: the running maximum and sum of the wave's 16 rows
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = q0 + wave * 16 + r;
    rm[r] = -INFINITY;
    rs[r] = 0.f;
    rn[r] = i < R ? norms[i] : 1.f;
  }
  float4 qa[2], ga[4];
  if (t_begin < t_end) {
    nq_load_rows<VEC4, 2>(reps, q0, R, d, 0, qa);
    nq_load_rows<VEC4, 4>(queue, t_begin * SQ_TG, n_valid, d, 0, ga);
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int g0 = t * SQ_TG;
    nq_score_tile<VEC4>(smem, reps, queue, R, n_valid, d, q0, g0, t + 1 < t_end, qa, ga);
    const bool ok0 = g0 + lane < n_valid, ok1 = g0 + 64 + lane < n_valid;     // g0 < n_valid: lane 0's first score always counts
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 16 + r;
      if (q0 + row < R) {                                                     // wave-uniform
        const float x0 = nq_logit(smem[row * SQ_LDS + lane], rn[r], inv_t);
        const float x1 = nq_logit(smem[row * SQ_LDS + 64 + lane], rn[r], inv_t);
        const float tm = nq_wave_max_all(fmaxf(ok0 ? x0 : -INFINITY, ok1 ? x1 : -INFINITY));
        const float mn = fmaxf(rm[r], tm);
        const float e = wave_sum_all((ok0 ? expf(x0 - mn) : 0.f) + (ok1 ? expf(x1 - mn) : 0.f));
        rs[r] = (rm[r] == -INFINITY ? 0.f : rs[r] * expf(rm[r] - mn)) + e;
        rm[r] = mn;
      }
    }
    __syncthreads();                                                          // the next tile's stores overwrite the scores
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = q0 + wave * 16 + r;
      if (i < R) {
        pm[(size_t)blockIdx.y * R + i] = rm[r];
        ps[(size_t)blockIdx.y * R + i] = rs[r];
      }
    }
  }
}

// one block: row i's in-batch terms (ntx_loss_kernel's arithmetic on the sim table) and then the queue's pairs, split ascending
__global__ void __launch_bounds__(256)
ntxq_fwd_combine_kernel(const float* __restrict__ sim, const float* __restrict__ pm, const float* __restrict__ ps, int nsplit,
                        float* __restrict__ lse, float* __restrict__ loss, int R, float inv_t) {
  __shared__ double sm[16];
  const int n = R >> 1;
  double a = 0.0;
  for (int i = threadIdx.x; i < R; i += blockDim.x) {
    const float* p = sim + (size_t)i * R;
    float mx = -INFINITY;                                                     // R >= 4: a row has in-batch terms
    for (int j = 0; j < R; ++j) if (j != i) mx = fmaxf(mx, p[j] * inv_t);
    float se = 0.f;
    for (int j = 0; j < R; ++j) if (j != i) se += expf(p[j] * inv_t - mx);
    for (int s = 0; s < nsplit; ++s) {
      const float m2 = pm[(size_t)s * R + i], s2 = ps[(size_t)s * R + i];
      if (s2 > 0.f) {                                                         // (a split that saw nothing holds (-inf, 0))
        const float mn = fmaxf(mx, m2);
        se = se * expf(mx - mn) + s2 * expf(m2 - mn);
        mx = mn;
      }
    }
    const float l = logf(se) + mx;
    lse[i] = l;
    a += (double)(l - p[(i + n) % R] * inv_t);
  }
  a = block_sum(a, sm);
  if (threadIdx.x == 0) loss[0] = (float)(a / R);
}

template <bool VEC4>
__global__ void __launch_bounds__(256)
ntxq_bwd_kernel(const float* __restrict__ reps, const float* __restrict__ queue, const float* __restrict__ norms,
                const float* __restrict__ lse, int R, int n_valid, int d, float inv_t, int tiles_per_split,
                float* __restrict__ part) {
  __shared__ float smem[SQ_SMEM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lrow = lane >> 5, lcol = lane & 31;
  const int q0 = blockIdx.x * SQ_TQ;
  const int gtiles = (n_valid + SQ_TG - 1) / SQ_TG;
  const int t_begin = blockIdx.y * tiles_per_split;
  const int t_end = t_begin + tiles_per_split < gtiles ? t_begin + tiles_per_split : gtiles;
  const int fc0 = blockIdx.z * NQ_FS + wave * 64 + lcol, fc1 = fc0 + 32;      // this lane's two feature columns
  const bool f0_ok = fc0 < d, f1_ok = fc1 < d;

  floatx16 acc[2][2] = {{{0}, {0}}, {{0}, {0}}};                              // [row half][feature half]
  float4 qa[2], ga[4];
  if (t_begin < t_end) {
    nq_load_rows<VEC4, 2>(reps, q0, R, d, 0, qa);
    nq_load_rows<VEC4, 4>(queue, t_begin * SQ_TG, n_valid, d, 0, ga);
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int g0 = t * SQ_TG;
    nq_score_tile<VEC4>(smem, reps, queue, R, n_valid, d, q0, g0, t + 1 < t_end, qa, ga);
    // scores -> probabilities in place, each wave its 16 rows; rows from R on and columns from n_valid on are exact zeros
    const bool ok0 = g0 + lane < n_valid, ok1 = g0 + 64 + lane < n_valid;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 16 + r, i = q0 + row;
      float p0 = 0.f, p1 = 0.f;
      if (i < R) {                                                            // wave-uniform
        const float ni = norms[i], li = lse[i];
        if (ok0) p0 = expf(nq_logit(smem[row * SQ_LDS + lane], ni, inv_t) - li);
        if (ok1) p1 = expf(nq_logit(smem[row * SQ_LDS + 64 + lane], ni, inv_t) - li);
      }
      smem[row * SQ_LDS + lane] = p0;
      smem[row * SQ_LDS + 64 + lane] = p1;
    }
    __syncthreads();
    // acc += P [64][128] x queue[g0 .. g0 + 128)[slice]: A fragments from LDS (row stride 129: no conflicts), B from global,
    // 32 lanes on one 128-byte line
    const float* Pa = smem + lcol * SQ_LDS + lrow;
#pragma unroll 8
    for (int kk = 0; kk < SQ_TG; kk += 2) {
      const int krow = g0 + kk + lrow;
      float b0 = 0.f, b1 = 0.f;
      if (krow < n_valid) {
        const float* src = queue + (size_t)krow * d;
        if (f0_ok) b0 = src[fc0];
        if (f1_ok) b1 = src[fc1];
      }
      const float a0 = Pa[kk], a1 = Pa[32 * SQ_LDS + kk];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();                                                          // the next tile's stores overwrite P
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = q0 + 32 * h + (r & 3) + 8 * (r >> 2) + 4 * lrow;
      if (i < R) {
        float* o = part + ((size_t)blockIdx.y * R + i) * d;
        if (f0_ok) o[fc0] = acc[h][0][r];
        if (f1_ok) o[fc1] = acc[h][1][r];
      }
    }
  }
}

// one block per row i: dq = sc * sum_splits part (split ascending); dreps_i += (dq - rhat_i <rhat_i, dq>) / |r_i|
__global__ void __launch_bounds__(256)
ntxq_bwd_combine_kernel(const float* __restrict__ reps, const float* __restrict__ norms, const float* __restrict__ part,
                        const float* __restrict__ dloss, float* __restrict__ dreps, int R, int f, int nsplit, float inv_t) {
  __shared__ float sm[16];
  __shared__ float bdot;
  const int i = blockIdx.x;
  const float ni = fmaxf(norms[i], 1e-8f);
  const float sc = dloss[0] * inv_t / (float)R;
  float dh[NQ_MAX_F / 256];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < NQ_MAX_F / 256; ++c) {
    const int q = threadIdx.x + 256 * c;
    float a = 0.f;
    if (q < f) {
      for (int s = 0; s < nsplit; ++s) a += part[((size_t)s * R + i) * f + q];
      a *= sc;
      dot += a * reps[(size_t)i * f + q] / ni;
    }
    dh[c] = a;
  }
  dot = block_sum(dot, sm);
  if (threadIdx.x == 0) bdot = dot;
  __syncthreads();
  dot = bdot;
#pragma unroll
  for (int c = 0; c < NQ_MAX_F / 256; ++c) {
    const int q = threadIdx.x + 256 * c;
    if (q < f) dreps[(size_t)i * f + q] += (dh[c] - reps[(size_t)i * f + q] / ni * dot) / ni;
  }
}

// one wave per row: queue[ptr + i] = reps[i] / max(|reps[i]|, 1e-8).  The sum of squares is taken in double, so the norm is the
// correctly rounded one and an element is two fp32 roundings from the exact quotient: the rows are unit length to 1 ulp.
__global__ void __launch_bounds__(64)
ntxq_push_kernel(const float* __restrict__ reps, float* __restrict__ queue, int f, int ptr) {
  const int row = blockIdx.x, lane = threadIdx.x;
  const float* src = reps + (size_t)row * f;
  double a = 0.0;
  for (int q = lane; q < f; q += 64) a += (double)src[q] * (double)src[q];
  a = wave_sum_all(a);
  const float nrm = fmaxf((float)sqrt(a), 1e-8f);
  float* dst = queue + ((size_t)ptr + row) * f;
  for (int q = lane; q < f; q += 64) dst[q] = src[q] / nrm;
}

// blocks along the queue per row tile and the tiles each walks (none is left without one); 0 with an empty queue
int nq_split_of(int R, int f, int n_valid, int* tiles_per_split) {
  *tiles_per_split = 0;
  if (n_valid <= 0) return 0;
  const int qtiles = cdiv(R, SQ_TQ), gtiles = cdiv(n_valid, SQ_TG);
  int ns = SQ_FILL_BLOCKS / qtiles;
  if (ns > gtiles / NQ_MIN_TILES) ns = gtiles / NQ_MIN_TILES;
  if (ns > NQ_MAX_SPLIT) ns = NQ_MAX_SPLIT;
  const size_t fit = NQ_PART_FLOATS / ((size_t)R * f);
  if ((size_t)ns > fit) ns = (int)fit;
  if (ns < 1) ns = 1;
  const int per = cdiv(gtiles, ns);
  *tiles_per_split = per;
  return cdiv(gtiles, per);
}

inline bool nq_shape_ok(int R, int f, int n_valid) {
  return R >= 4 && (R & 1) == 0 && R <= 8192 && f >= 1 && f <= NQ_MAX_F && n_valid >= 0 && n_valid <= (1 << 30);
}

// ws: [cstp_ntxent's block: norms | lse | sim | G] [pm: ns R] [ps: ns R] [part: ns R f]
struct NqLayout {
  size_t ntx_bytes, total;
  float *norms, *lse, *sim, *pm, *ps, *part;
  int ns, per;
};

NqLayout nq_layout(void* ws, int R, int f, int n_valid) {
  NqLayout l;
  l.ns = nq_split_of(R, f, n_valid, &l.per);
  l.ntx_bytes = cstp_ntxent_workspace_bytes(R, f);
  l.total = l.ntx_bytes + (size_t)l.ns * R * (2 + (size_t)f) * sizeof(float);
  l.norms = reinterpret_cast<float*>(ws);
  l.lse = l.norms + R;
  l.sim = l.lse + R;
  l.pm = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + l.ntx_bytes);
  l.ps = l.pm + (size_t)l.ns * R;
  l.part = l.ps + (size_t)l.ns * R;
  return l;
}

}  // namespace
}  // namespace cstp

extern "C" size_t cstp_ntxq_workspace_bytes(int32_t R, int32_t f, int32_t n_valid) {
  if (!cstp::nq_shape_ok(R, f, n_valid)) return 0;
  return cstp::nq_layout(nullptr, R, f, n_valid).total;
}

#define CSTP_NTXQ_CHECK_ARGS()                                                                                  \
  CSTP_REQUIRE(R >= 4 && (R % 2) == 0 && R <= 8192, "R must be even and in 4..8192");                             \
  CSTP_REQUIRE(f >= 1 && f <= cstp::NQ_MAX_F, "f must be in 1..2048");                                          \
  CSTP_REQUIRE(temperature > 0.f, "temperature must be positive");                                             \
  CSTP_REQUIRE(cap >= 0 && cap <= (1 << 30) && n_valid >= 0 && n_valid <= cap, "n_valid must be in [0, cap]"); \
  CSTP_REQUIRE(ws_bytes >= cstp_ntxq_workspace_bytes(R, f, n_valid), "workspace too small")

extern "C" int cstp_ntxq_forward(void* stream, const float* reps, const float* queue, float* loss, int32_t R, int32_t f,
                                 int32_t cap, int32_t n_valid, float temperature, void* ws, size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(reps != nullptr && queue != nullptr && loss != nullptr && ws != nullptr, "null argument");
  CSTP_NTXQ_CHECK_ARGS();
  const NqLayout l = nq_layout(ws, R, f, n_valid);
  if (const int e = cstp_ntxent_forward(stream, reps, loss, R, f, temperature, ws, l.ntx_bytes)) return e;
  hipStream_t st = as_stream(stream);
  const float inv_t = 1.f / temperature;
  if (l.ns > 0) {
    const bool v4 = (f & 3) == 0 && ((reinterpret_cast<uintptr_t>(reps) | reinterpret_cast<uintptr_t>(queue)) & 15u) == 0;
    const dim3 grid(cdiv(R, SQ_TQ), l.ns);
    if (v4) hipLaunchKernelGGL(ntxq_fwd_kernel<true>, grid, dim3(256), 0, st, reps, queue, l.norms, R, n_valid, f, inv_t, l.per, l.pm, l.ps);
    else hipLaunchKernelGGL(ntxq_fwd_kernel<false>, grid, dim3(256), 0, st, reps, queue, l.norms, R, n_valid, f, inv_t, l.per, l.pm, l.ps);
    CSTP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ntxq_fwd_combine_kernel, dim3(1), dim3(256), 0, st, l.sim, l.pm, l.ps, l.ns, l.lse, loss, R, inv_t);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_ntxq_backward(void* stream, const float* reps, const float* queue, const float* dloss, float* dreps,
                                  int32_t R, int32_t f, int32_t cap, int32_t n_valid, float temperature, void* ws,
                                  size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(reps != nullptr && queue != nullptr && dloss != nullptr && dreps != nullptr && ws != nullptr, "null argument");
  CSTP_NTXQ_CHECK_ARGS();
  const NqLayout l = nq_layout(ws, R, f, n_valid);
  hipStream_t st = as_stream(stream);
  const float inv_t = 1.f / temperature;
  if (l.ns > 0) {
    const bool v4 = (f & 3) == 0 && ((reinterpret_cast<uintptr_t>(reps) | reinterpret_cast<uintptr_t>(queue)) & 15u) == 0;
    const dim3 grid(cdiv(R, SQ_TQ), l.ns, cdiv(f, NQ_FS));
    if (v4) hipLaunchKernelGGL(ntxq_bwd_kernel<true>, grid, dim3(256), 0, st, reps, queue, l.norms, l.lse, R, n_valid, f, inv_t, l.per, l.part);
    else hipLaunchKernelGGL(ntxq_bwd_kernel<false>, grid, dim3(256), 0, st, reps, queue, l.norms, l.lse, R, n_valid, f, inv_t, l.per, l.part);
    CSTP_LAUNCH_CHECK();
  }
  if (const int e = cstp_ntxent_backward(stream, reps, dloss, dreps, R, f, temperature, ws, l.ntx_bytes)) return e;
  if (l.ns > 0) {
    hipLaunchKernelGGL(ntxq_bwd_combine_kernel, dim3(R), dim3(256), 0, st, reps, l.norms, l.part, dloss, dreps, R, f, l.ns, inv_t);
    CSTP_LAUNCH_CHECK();
  }
  return 0;
}
#undef CSTP_NTXQ_CHECK_ARGS

extern "C" int cstp_ntxq_push(void* stream, const float* reps, float* queue, int32_t R, int32_t f, int32_t cap, int32_t ptr) {
  using namespace cstp;
  CSTP_REQUIRE(reps != nullptr && queue != nullptr, "null argument");
  CSTP_REQUIRE(R >= 1 && R <= 8192 && f >= 1 && f <= NQ_MAX_F, "bad shape");
  CSTP_REQUIRE(cap >= 1 && cap <= (1 << 30) && ptr >= 0 && ptr <= cap - R, "rows [ptr, ptr + R) must lie inside the queue");
  hipLaunchKernelGGL(ntxq_push_kernel, dim3(R), dim3(64), 0, as_stream(stream), reps, queue, f, ptr);
  CSTP_LAUNCH_CHECK();
  return 0;
}
