// Spherical k-means on cached features (cstp_kmeans_assign / cstp_kmeans_update, spec in include/cstp_hip.h): Lloyd's iteration
// for R restarts at once, the restart being a grid dimension.  No [n][c] similarity table, no atomics, nothing read back.
//
//   1. kmeans_assign_kernel<VEC4>  block = 256 threads = 4 waves owns SQ_TQ = 64 rows of x and one restart, and walks that
//      restart's centroids in tiles of SQ_TG = 128 -- simtopk_kernel's walk, staging and MFMA fragments (sq_tile_scores), so a (row, centroid)
//      similarity is the same fmaf chain over ascending features and holds the bits ops.sim_topk gives.  The 64 x 128 scores go
//      over the operand image; a wave then owns 16 rows and lane l looks at centroids g0 + l and g0 + 64 + l: each lane keeps its
//      own running (best, id) per row in registers, replaced only by a strictly larger value -- centroids arrive in ascending
//      order, so a lane keeps the lowest id among equal values.  After the last tile a 6-step butterfly per row picks the
//      largest value, the lower id among equal ones: (similarity descending, id ascending).  Lanes 0..15 of a wave write the
//      rows' assign / best and compare with prev; wave 0 then adds the tile's 64 best values in double (rows past n as 0) and
//      the 64 moved flags, each in one fixed shuffle tree, into the workspace: one partial per (restart, row tile).
//   2. kmeans_fold_kernel  one block per restart: thread t adds partials t, t + 256, ... in that order, then one fixed tree.
//      score[r] and moved[r] therefore depend on (n, best[r], assign[r], prev[r]) alone -- not on R, not on the grid.
//   3. kmeans_update_kernel  one block per (cluster j, restart).  It scans assign[r][0..n) in chunks of KM_CHUNK = 1024 rows;
//      thread t looks at rows i0 + 4 t .. + 3 and a block-wide exclusive scan of the match counts compacts the rows with
//      assign == j into an LDS list IN ASCENDING ROW ORDER.  Thread t owns features t, t + 256, ... (d <= 4096: 16 registers)
//      and adds the listed rows one by one:
//          THE ORDER OF EVERY SUM: s[j][f] = (((0 + x[i_1][f]) + x[i_2][f]) + ...), i_1 < i_2 < ... the rows with assign == j,
//      one fp32 chain per (cluster, feature), a function of (n, assign) and nothing else.  Then
//          ss = sum_f s[f]^2: per thread fmaf over its features ascending (f = t, t + 256, ...), the 256 partials through
//               block_sum's fixed tree (64-lane shuffle tree per wave, the four wave sums through one more) -- a function of d;
//          cent_out[j][f] = s[f] * (1.0f / sqrtf(ss))   (division and square root correctly rounded).
//      counts[r][j] = the number of listed rows.  A cluster without rows, or with ss not > 0, copies cent_in[r][j].  An assign value
//      outside 0..c-1 equals no block's j: it is compared, never used to form an address.
//      COST: every block reads all of assign[r] (c * n * 4 bytes per restart out of L2, three barriers per chunk) and x once.
//      That suits the evaluation's sizes (n ~ 10^4 - 10^5, c ~ 10^2: 105 MB at n = 65 536, c = 400).  The limits below are what the
//      indexing supports, not what this kernel is meant for: at n = 2^24, c = 4096, r = 32 it is 131 072 blocks reading 64 MB
//      each, a launch of many seconds.  Sizes far beyond the evaluation's want the rows bucketed once per restart first.
// Every global index is formed from a row < n, a centroid < c and a feature < d that were checked first; masked operand
// elements are zeros.
#pragma once
#include <math.h>

#include "common.h"

namespace cstp {
namespace {

constexpr int KM_MAX_N = 1 << 24, KM_MAX_D = 4096, KM_MAX_C = 4096, KM_MAX_R = 32;
constexpr int KM_CHUNK = 1024;                             // rows of assign scanned per step of the update kernel
constexpr int KM_FQ = KM_MAX_D / 256;                      // features per thread of the update kernel, at most

template <bool VEC4>
__global__ void __launch_bounds__(256)
kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ cent_all, const int* __restrict__ prev_all, int n, int d,
                     int c, int* __restrict__ assign_all, float* __restrict__ best_all, double* __restrict__ part_score,
                     int* __restrict__ part_moved) {
  __shared__ float smem[SQ_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * SQ_TQ, rs = blockIdx.y;
  const float* __restrict__ g = cent_all + (size_t)rs * c * d;
  const int gtiles = (c + SQ_TG - 1) / SQ_TG;

  float bv[16];
  int bi[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bv[r] = -INFINITY;
    bi[r] = -1;
  }

  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  float4 qa[2], ga[4];
  sq_load_rows<VEC4>(x, q0, n, 0, d, srow, sc4, qa, 2);
  sq_load_rows<VEC4>(g, 0, c, 0, d, srow, sc4, ga, 4);
  for (int t = 0; t < gtiles; ++t) {
    const int g0 = t * SQ_TG;
    sq_tile_scores<VEC4>(smem, x, q0, n, g, g0, c, t + 1 < gtiles ? g0 + SQ_TG : -1, d, qa, ga);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 16 + r;
#pragma unroll
      for (int h = 0; h < SQ_TG; h += 64) {
        const int j = g0 + h + lane;
        const float v = smem[row * SQ_LDS + h + lane];
        if (j < c && v > bv[r]) {                       // j ascending per lane: the first of equal values stays
          bv[r] = v;
          bi[r] = j;
        }
      }
    }
    __syncthreads();                                    // the next tile's stores overwrite the scores
  }

  // per row: the largest value over the 64 lanes, the lower centroid id among equal ones (-1 = "none" compares as the highest)
  float ov = 0.f;
  int oi = -1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = bv[r];
    int j = bi[r];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float pv = __shfl_xor(v, off, 64);
      const int pj = __shfl_xor(j, off, 64);
      if (pv > v || (pv == v && (unsigned)pj < (unsigned)j)) {
        v = pv;
        j = pj;
      }
    }
    if (lane == r) {
      ov = v;
      oi = j;
    }
  }
  const int i = q0 + wave * 16 + lane;                  // lanes 0..15: row wave * 16 + lane of the tile
  int mv = 0;
  if (lane < 16) {
    if (i < n) {
      const size_t o = (size_t)rs * n + i;
      assign_all[o] = oi;
      best_all[o] = ov;
      mv = prev_all != nullptr ? (prev_all[o] != oi ? 1 : 0) : 1;
    } else {
      ov = 0.f;
    }
    smem[wave * 16 + lane] = ov;
    reinterpret_cast<int*>(smem)[64 + wave * 16 + lane] = mv;
  }
  __syncthreads();
  if (wave == 0) {
    const double s = wave_sum((double)smem[lane]);
    const int m = wave_sum(reinterpret_cast<const int*>(smem)[64 + lane]);
    if (lane == 0) {
      const size_t o = (size_t)rs * gridDim.x + blockIdx.x;
      part_score[o] = s;
      part_moved[o] = m;
    }
  }
}

__global__ void __launch_bounds__(256)
kmeans_fold_kernel(const double* __restrict__ part_score, const int* __restrict__ part_moved, int tiles, double* __restrict__ score,
                   int* __restrict__ moved) {
  __shared__ double sd[16];
  __shared__ int si[16];
  const int tid = threadIdx.x, rs = blockIdx.x;
  double s = 0.0;
  int m = 0;
  for (int k = tid; k < tiles; k += 256) {
    s += part_score[(size_t)rs * tiles + k];
    m += part_moved[(size_t)rs * tiles + k];
  }
  s = block_sum(s, sd);
  m = block_sum(m, si);
  if (tid == 0) {
    score[rs] = s;
    moved[rs] = m;
  }
}

__global__ void __launch_bounds__(256)
kmeans_update_kernel(const float* __restrict__ x, const int* __restrict__ assign_all, const float* __restrict__ cent_in,
                     int n, int d, int c, float* __restrict__ cent_out, int* __restrict__ counts) {
  __shared__ int list[KM_CHUNK];
  __shared__ int wtot[4];
  __shared__ float sf[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.x, rs = blockIdx.y;
  const int* __restrict__ assign = assign_all + (size_t)rs * n;
  float acc[KM_FQ];
#pragma unroll
  for (int q = 0; q < KM_FQ; ++q) acc[q] = 0.f;
  int total = 0;

  for (int i0 = 0; i0 < n; i0 += KM_CHUNK) {
    const int ib = i0 + 4 * tid;
    int hit[4], cnt = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      hit[e] = (ib + e < n && assign[ib + e] == j) ? 1 : 0;
      cnt += hit[e];
    }
    int incl = cnt;                                     // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    __syncthreads();                                    // the previous chunk's list has been summed
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int pos = incl - cnt, m = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) pos += wtot[w];
      m += wtot[w];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (hit[e]) list[pos++] = ib + e;                 // pos < m <= KM_CHUNK; ascending rows
    __syncthreads();
    total += m;
    int k = 0;
    for (; k + 4 <= m; k += 4) {                        // four rows' loads in flight, added in list order
      const size_t r0 = (size_t)list[k] * d, r1 = (size_t)list[k + 1] * d, r2 = (size_t)list[k + 2] * d,
                   r3 = (size_t)list[k + 3] * d;
#pragma unroll
      for (int q = 0; q < KM_FQ; ++q) {
        const int f = q * 256 + tid;
        if (f < d) {
          const float v0 = x[r0 + f], v1 = x[r1 + f], v2 = x[r2 + f], v3 = x[r3 + f];
          acc[q] = ((acc[q] + v0) + v1) + v2;
          acc[q] += v3;
        }
      }
    }
    for (; k < m; ++k) {
      const size_t r0 = (size_t)list[k] * d;
#pragma unroll
      for (int q = 0; q < KM_FQ; ++q) {
        const int f = q * 256 + tid;
        if (f < d) acc[q] += x[r0 + f];
      }
    }
  }

  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < KM_FQ; ++q) ss = fmaf(acc[q], acc[q], ss);          // features past d hold 0
  ss = block_sum(ss, sf);
  if (tid == 0) sf[0] = ss;
  __syncthreads();
  ss = sf[0];
  const bool keep = total == 0 || !(ss > 0.f);                            // block-uniform
  const float inv = keep ? 0.f : 1.0f / sqrtf(ss);
  const size_t o = ((size_t)rs * c + j) * d;
#pragma unroll
  for (int q = 0; q < KM_FQ; ++q) {
    const int f = q * 256 + tid;
    if (f < d) cent_out[o + f] = keep ? cent_in[o + f] : acc[q] * inv;
  }
  if (tid == 0) counts[(size_t)rs * c + j] = total;
}

inline bool kmeans_shape_ok(int n, int d, int c, int r) {
  return n >= 1 && n <= KM_MAX_N && d >= 1 && d <= KM_MAX_D && c >= 1 && c <= KM_MAX_C && c <= n && r >= 1 && r <= KM_MAX_R;
}

struct KmeansWs { size_t score, moved, total; };

inline KmeansWs kmeans_layout(int n, int r) {
  const size_t parts = (size_t)r * cdiv(n, SQ_TQ);
  KmeansWs o;
  o.score = 0;
  o.moved = align_up(parts * sizeof(double), 16);
  o.total = o.moved + align_up(parts * sizeof(int32_t), 16);
  return o;
}

}  // namespace
}  // namespace cstp

extern "C" size_t cstp_kmeans_workspace_bytes(int32_t n, int32_t d, int32_t c, int32_t r) {
  if (!cstp::kmeans_shape_ok(n, d, c, r)) return 0;
  return cstp::kmeans_layout(n, r).total;
}

extern "C" int cstp_kmeans_assign(void* stream, const float* x, const float* cent, const int32_t* prev, int32_t n, int32_t d,
                                  int32_t c, int32_t r, int32_t* assign, float* best, int32_t* moved, double* score, void* ws,
                                  size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && cent != nullptr && assign != nullptr && best != nullptr && moved != nullptr && score != nullptr &&
                   ws != nullptr, "null argument");
  CSTP_REQUIRE(r >= 1 && r <= KM_MAX_R, "r must be in 1..32");
  CSTP_REQUIRE(d >= 1 && d <= KM_MAX_D, "d must be in 1..4096");
  CSTP_REQUIRE(c >= 1 && c <= KM_MAX_C, "c must be in 1..4096");
  CSTP_REQUIRE(n >= 1 && n <= KM_MAX_N, "n must be in 1..2^24");
  CSTP_REQUIRE(c <= n, "c must not exceed n");
  const size_t ab = (size_t)r * n * sizeof(int32_t);
  CSTP_REQUIRE(prev == nullptr || !pr_overlap(prev, ab, assign, ab), "assign must not alias prev");
  CSTP_REQUIRE(pr_aligned16(ws), "workspace must be 16-byte aligned");
  const KmeansWs lay = kmeans_layout(n, r);
  CSTP_REQUIRE(ws_bytes >= lay.total, "workspace too small");
  char* base = reinterpret_cast<char*>(ws);
  double* ps = reinterpret_cast<double*>(base + lay.score);
  int* pm = reinterpret_cast<int*>(base + lay.moved);
  const int tiles = cdiv(n, SQ_TQ);
  const bool v4 = (d & 3) == 0 && pr_aligned16(x) && pr_aligned16(cent);
  hipStream_t st = as_stream(stream);
  const dim3 grid(tiles, r);
  if (v4) hipLaunchKernelGGL(kmeans_assign_kernel<true>, grid, dim3(256), 0, st, x, cent, prev, n, d, c, assign, best, ps, pm);
  else hipLaunchKernelGGL(kmeans_assign_kernel<false>, grid, dim3(256), 0, st, x, cent, prev, n, d, c, assign, best, ps, pm);
  CSTP_LAUNCH_CHECK();
  hipLaunchKernelGGL(kmeans_fold_kernel, dim3(r), dim3(256), 0, st, ps, pm, tiles, score, moved);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_kmeans_update(void* stream, const float* x, const int32_t* assign, const float* cent_in, int32_t n, int32_t d,
                                  int32_t c, int32_t r, float* cent_out, int32_t* counts) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && assign != nullptr && cent_in != nullptr && cent_out != nullptr && counts != nullptr, "null argument");
  CSTP_REQUIRE(r >= 1 && r <= KM_MAX_R, "r must be in 1..32");
  CSTP_REQUIRE(d >= 1 && d <= KM_MAX_D, "d must be in 1..4096");
  CSTP_REQUIRE(c >= 1 && c <= KM_MAX_C, "c must be in 1..4096");
  CSTP_REQUIRE(n >= 1 && n <= KM_MAX_N, "n must be in 1..2^24");
  CSTP_REQUIRE(c <= n, "c must not exceed n");
  const size_t cb = (size_t)r * c * d * sizeof(float);
  CSTP_REQUIRE(!pr_overlap(cent_out, cb, cent_in, cb), "cent_out must not alias cent_in");
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(c, r), dim3(256), 0, as_stream(stream), x, assign, cent_in, n, d, c, cent_out, counts);
  CSTP_LAUNCH_CHECK();
  return 0;
}
