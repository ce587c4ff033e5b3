// Label-free collapse metrics on cached features (cstp_feat_gram / cstp_pair_potential, spec in include/cstp_hip.h): the two
// reductions over x [n][d] that cstp_amd/health.py turns into rank, spread and uniformity figures.  No [n][n] tensor, no atomics,
// nothing read back; two calls on equal inputs give equal bits.
//
//   1. featgram_kernel<VEC4>  G = x^T x.  block = 256 threads = 4 waves owns features [a0, a0 + 64) x [b0, b0 + 128) of G and
//      walks ALL rows, in slabs of GR_SLAB = 32.  The reduction runs over the rows, so a chunk of 32 rows x 64 (x 128) features
//      of row-major x already IS the [k][row] operand image of simtopk_kernel's buffers: it is copied there as it lies, no
//      transposing store, and sq_mma_chunk (retrieve.hip) multiplies it -- the fragments, strides and the accumulator layout of
//      the similarity kernels.  Inside a slab a pair (a, b) is therefore ONE fp32 fmaf chain over ascending rows; at the end of a
//      slab the 32 x 32 x 2 accumulators are widened and added to fp64 registers, slabs ascending:
//          G[a][b] = ((0 + (double)P_0[a][b]) + (double)P_1[a][b]) + ...,  P_s[a][b] = fmaf chain over rows [32 s, 32 s + 32)
//      a function of (x, n, d) alone -- there is no split to choose.  WHY 32 AND NOT MORE: the features of an encoder are mostly
//      of one sign (ReLU, pooling), so a chain's rounding errors do not cancel and grow with its length; the small eigenvalues of
//      G, which rankme takes the square root of, feel an ABSOLUTE error of G.  Emulated on the CPU for a 1100 x 100 input, slabs of
//      1024 rows leave G 8e-7 and rankme 7e-6 off the fp64 answer (a vendor fp32 GEMM: 2e-7 and 1e-6), slabs of 32 rows 3e-8 and
//      2e-7.  The price is 32 conversions and 32 fp64 additions per lane beside 32 MFMAs.
//      Every tile of G is computed, also below the diagonal: x[i][a] * x[i][b] and x[i][b] * x[i][a] are the same product, so the chains of (a, b) and (b, a) hold the same bits and
//      G == G^T without a mirror pass.  Rows past a slab's end and features past d are zeros (fmaf(0, 0, acc) leaves acc).
//   2. colsum_part_kernel  one thread per feature and part of CS_ROWS = 1024 rows adds the part's rows in fp64, ascending; the
//      blocks of featgram_kernel with b0 == 0 then add the partials of their 64 features in ascending order.  The partials are
//      the workspace.
//   3. pairpot_kernel<VEC4>  rowsum[i] = sum_{j != i} expf(2t (s_ij - 1)).  simtopk_kernel's walk (sq_tile_scores) with x as
//      queries and gallery: block = 64 rows, gallery tiles of 128, s_ij the bits ops.sim_topk gives.  The gallery tiles are dealt
//      into nseg <= SQ_MAX_SPLIT SEGMENTS of tiles_per_seg tiles, a function of n alone.  Within a segment lane l of the wave
//      that owns row i adds its terms (columns g0 + l, then g0 + 64 + l, tiles ascending; the diagonal left out by index) to one
//      fp64 register; at the segment's end the 64 lanes go through wave_sum's fixed tree into part[seg][i].  A block walks
//      segs_per_block consecutive segments -- that, the gallery split of the grid, is a scheduling choice (few row tiles: more
//      blocks per row tile) and changes no bit, because no sum crosses a segment inside the kernel.
//   4. pairpot_fold_kernel  rowsum[i] = ((0 + part[0][i]) + part[1][i]) + ..., segments ascending.
// Every global index is formed from a row < n and a feature < d that were checked first.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace cstp {
namespace {

constexpr int HL_MAX_D = 4096;
constexpr int GR_SLAB = SQ_BK;                             // rows per fp32 chain of cstp_feat_gram: one chunk of the operand buffers
constexpr int CS_ROWS = 1024;                              // rows per partial of its column sums

template <bool VEC4>
__global__ void __launch_bounds__(256)
featgram_kernel(const float* __restrict__ x, int n, int d, int npart, const double* __restrict__ cs_part, double* __restrict__ gram,
                double* __restrict__ colsum) {
  __shared__ float smem[2 * SQ_BUF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int a0 = blockIdx.x * SQ_TQ, b0 = blockIdx.y * SQ_TG;

  double g0[16], g1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) g0[r] = g1[r] = 0.0;

  // staging: a chunk is 32 rows; thread tid holds features 4 (tid & 15) .. + 3 of A rows tid >> 4 and + 16, and features
  // 4 (tid & 31) .. + 3 of B rows (tid >> 5) + 8 p
  const int arow = tid >> 4, ac4 = (tid & 15) * 4, brow = tid >> 5, bc4 = (tid & 31) * 4;
  float4 fa[2], fb[4];
  auto load_feats = [&](int row, int c) __attribute__((always_inline)) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n) {
      const float* src = x + (size_t)row * d + c;
      if (VEC4) {
        if (c < d) v = *reinterpret_cast<const float4*>(src);             // d % 4 == 0: the four features are in or out together
      } else {
        if (c < d) v.x = src[0];
        if (c + 1 < d) v.y = src[1];
        if (c + 2 < d) v.z = src[2];
        if (c + 3 < d) v.w = src[3];
      }
    }
    return v;
  };
  auto load_chunk = [&](int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 2; ++p) fa[p] = load_feats(i0 + arow + 16 * p, a0 + ac4);
#pragma unroll
    for (int p = 0; p < 4; ++p) fb[p] = load_feats(i0 + brow + 8 * p, b0 + bc4);
  };
  auto store_chunk = [&](float* buf) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float* o = buf + (arow + 16 * p) * SQ_LDA + ac4;
      o[0] = fa[p].x;
      o[1] = fa[p].y;
      o[2] = fa[p].z;
      o[3] = fa[p].w;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      float* o = buf + SQ_BK * SQ_LDA + (brow + 8 * p) * SQ_LDB + bc4;
      o[0] = fb[p].x;
      o[1] = fb[p].y;
      o[2] = fb[p].z;
      o[3] = fb[p].w;
    }
  };

  const int nslab = (n + GR_SLAB - 1) / GR_SLAB;
  load_chunk(0);
  store_chunk(smem);
  __syncthreads();
  int buf = 0;
  for (int s = 0; s < nslab; ++s) {                     // a slab is one chunk of the operand buffers
    const bool have_next = s + 1 < nslab;
    if (have_next) load_chunk((s + 1) * GR_SLAB);
    floatx16 acc0 = {0}, acc1 = {0};
    sq_mma_chunk(smem + buf * SQ_BUF, lrow, lcol, wave, acc0, acc1);
    if (have_next) store_chunk(smem + (buf ^ 1) * SQ_BUF);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      g0[r] += (double)acc0[r];
      g1[r] += (double)acc1[r];
    }
    __syncthreads();
    buf ^= 1;
  }

  const int b = b0 + wave * 32 + lcol;
  if (b < d) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int a = a0 + (r & 3) + 8 * (r >> 2) + 4 * lrow;
      if (a < d) gram[(size_t)a * d + b] = g0[r];
      if (a + 32 < d) gram[(size_t)(a + 32) * d + b] = g1[r];
    }
  }
  if (blockIdx.y == 0 && tid < SQ_TQ && a0 + tid < d) {
    double sum = 0.0;
    for (int s = 0; s < npart; ++s) sum += cs_part[(size_t)s * d + a0 + tid];
    colsum[a0 + tid] = sum;
  }
}

__global__ void __launch_bounds__(256)
colsum_part_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ cs_part) {
  const int a = blockIdx.y * 256 + threadIdx.x, s = blockIdx.x;
  if (a >= d) return;
  const int i_lo = s * CS_ROWS, i_end = i_lo + CS_ROWS < n ? i_lo + CS_ROWS : n;
  double sum = 0.0;
#pragma unroll 8
  for (int i = i_lo; i < i_end; ++i) sum += (double)x[(size_t)i * d + a];
  cs_part[(size_t)s * d + a] = sum;
}

template <bool VEC4>
__global__ void __launch_bounds__(256)
pairpot_kernel(const float* __restrict__ x, int n, int d, float two_t, int tiles_per_seg, int nseg, int segs_per_block,
               double* __restrict__ part) {
  __shared__ float smem[SQ_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * SQ_TQ;
  const int gtiles = (n + SQ_TG - 1) / SQ_TG;
  const int seg_begin = blockIdx.y * segs_per_block;
  const int seg_end = seg_begin + segs_per_block < nseg ? seg_begin + segs_per_block : nseg;
  const int t_begin = seg_begin * tiles_per_seg;
  const int t_end = seg_end * tiles_per_seg < gtiles ? seg_end * tiles_per_seg : gtiles;

  double acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0;

  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  float4 qa[2], ga[4];
  if (t_begin < t_end) {
    sq_load_rows<VEC4>(x, q0, n, 0, d, srow, sc4, qa, 2);
    sq_load_rows<VEC4>(x, t_begin * SQ_TG, n, 0, d, srow, sc4, ga, 4);
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int g0 = t * SQ_TG;
    sq_tile_scores<VEC4>(smem, x, q0, n, x, g0, n, t + 1 < t_end ? g0 + SQ_TG : -1, d, qa, ga);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 16 + r, i = q0 + row;
      if (i < n) {                                                        // wave-uniform
#pragma unroll
        for (int h = 0; h < SQ_TG; h += 64) {
          const int j = g0 + h + lane;
          const float e = expf(two_t * (smem[row * SQ_LDS + h + lane] - 1.0f));
          if (j < n && j != i) acc[r] += (double)e;                       // the diagonal is left out by index
        }
      }
    }
    __syncthreads();                                                      // the next tile's stores overwrite the scores
    if ((t + 1) % tiles_per_seg == 0 || t + 1 == t_end) {                 // block-uniform: the segment ends here
      const int seg = t / tiles_per_seg;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = q0 + wave * 16 + r;
        if (i < n) {
          const double v = wave_sum(acc[r]);
          if (lane == 0) part[(size_t)seg * n + i] = v;
        }
        acc[r] = 0.0;
      }
    }
  }
}

__global__ void __launch_bounds__(256)
pairpot_fold_kernel(const double* __restrict__ part, int n, int nseg, double* __restrict__ rowsum) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double sum = 0.0;
  for (int s = 0; s < nseg; ++s) sum += part[(size_t)s * n + i];
  rowsum[i] = sum;
}

inline bool health_shape_ok(int n, int d) { return n >= 1 && d >= 1 && d <= HL_MAX_D && (long)n * d < (1L << 31); }

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

struct PairpotPlan { int tiles_per_seg, nseg, segs_per_block, nsplit; };

// tiles_per_seg and nseg depend on n alone and fix every sum's order; segs_per_block / nsplit only deal the segments to blocks
inline PairpotPlan pairpot_plan(int n) {
  PairpotPlan p;
  const int gtiles = cdiv(n, SQ_TG);
  p.tiles_per_seg = cdiv(gtiles, SQ_MAX_SPLIT);
  p.nseg = cdiv(gtiles, p.tiles_per_seg);
  int ns = SQ_FILL_BLOCKS / cdiv(n, SQ_TQ);
  if (const char* e = getenv("CSTP_PAIRPOT_NSPLIT")) {                    // developer override (tests show it changes no bit)
    const int v = atoi(e);
    if (v >= 1 && v <= SQ_MAX_SPLIT) ns = v;
  }
  if (ns > p.nseg) ns = p.nseg;
  if (ns < 1) ns = 1;
  p.segs_per_block = cdiv(p.nseg, ns);
  p.nsplit = cdiv(p.nseg, p.segs_per_block);
  return p;
}

}  // namespace
}  // namespace cstp

extern "C" size_t cstp_feat_gram_workspace_bytes(int32_t n, int32_t d) {
  if (!cstp::health_shape_ok(n, d)) return 0;
  return (size_t)cstp::cdiv(n, cstp::CS_ROWS) * d * sizeof(double) + 256;
}

extern "C" int cstp_feat_gram(void* stream, const float* x, int32_t n, int32_t d, double* gram, double* colsum, void* ws,
                              size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && gram != nullptr && colsum != nullptr && ws != nullptr, "null argument");
  CSTP_REQUIRE(n >= 1, "n must be at least 1");
  CSTP_REQUIRE(d >= 1 && d <= HL_MAX_D, "d must be in 1..4096");
  CSTP_REQUIRE((long)n * d < (1L << 31), "n * d must be below 2^31");
  CSTP_REQUIRE(aligned8(gram) && aligned8(colsum) && aligned8(ws), "gram, colsum and the workspace must be 8-byte aligned");
  CSTP_REQUIRE(ws_bytes >= cstp_feat_gram_workspace_bytes(n, d), "workspace too small");
  const int npart = cdiv(n, CS_ROWS);
  double* cs_part = reinterpret_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(colsum_part_kernel, dim3(npart, cdiv(d, 256)), dim3(256), 0, st, x, n, d, cs_part);
  CSTP_LAUNCH_CHECK();
  const dim3 grid(cdiv(d, SQ_TQ), cdiv(d, SQ_TG));
  if ((d & 3) == 0 && pr_aligned16(x)) hipLaunchKernelGGL(featgram_kernel<true>, grid, dim3(256), 0, st, x, n, d, npart, cs_part, gram, colsum);
  else hipLaunchKernelGGL(featgram_kernel<false>, grid, dim3(256), 0, st, x, n, d, npart, cs_part, gram, colsum);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t cstp_pair_potential_workspace_bytes(int32_t n, int32_t d) {
  if (!cstp::health_shape_ok(n, d)) return 0;
  return (size_t)cstp::pairpot_plan(n).nseg * n * sizeof(double) + 256;
}

extern "C" int cstp_pair_potential(void* stream, const float* x, int32_t n, int32_t d, float t, double* rowsum, void* ws,
                                   size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && rowsum != nullptr && ws != nullptr, "null argument");
  CSTP_REQUIRE(n >= 1, "n must be at least 1");
  CSTP_REQUIRE(d >= 1 && d <= HL_MAX_D, "d must be in 1..4096");
  CSTP_REQUIRE((long)n * d < (1L << 31), "n * d must be below 2^31");
  CSTP_REQUIRE(isfinite(t) && t > 0.f && isfinite(2.0f * t), "t must be finite and positive");
  CSTP_REQUIRE(aligned8(rowsum) && aligned8(ws), "rowsum and the workspace must be 8-byte aligned");
  CSTP_REQUIRE(ws_bytes >= cstp_pair_potential_workspace_bytes(n, d), "workspace too small");
  const PairpotPlan p = pairpot_plan(n);
  double* part = reinterpret_cast<double*>(ws);
  hipStream_t st = as_stream(stream);
  const dim3 grid(cdiv(n, SQ_TQ), p.nsplit);
  if ((d & 3) == 0 && pr_aligned16(x))
    hipLaunchKernelGGL(pairpot_kernel<true>, grid, dim3(256), 0, st, x, n, d, 2.0f * t, p.tiles_per_seg, p.nseg, p.segs_per_block, part);
  else
    hipLaunchKernelGGL(pairpot_kernel<false>, grid, dim3(256), 0, st, x, n, d, 2.0f * t, p.tiles_per_seg, p.nseg, p.segs_per_block, part);
  CSTP_LAUNCH_CHECK();
  hipLaunchKernelGGL(pairpot_fold_kernel, dim3((unsigned)(((long)n + 255) / 256)), dim3(256), 0, st, part, n, p.nseg, rowsum);
  CSTP_LAUNCH_CHECK();
  return 0;
}
