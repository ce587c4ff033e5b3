// Few-shot episodic evaluation on cached features (cstp_fewshot_episodes, spec in include/cstp_hip.h): N-way K-shot episodes
// scored by the cosine nearest-centroid classifier.  No [E][N (K + Q)][d] gather, no similarity table, no atomics, no workspace,
// one launch; two calls on equal inputs give equal bits, and an episode's bits do not depend on the episodes around it.
//
// fewshot_kernel: block = 256 threads = 4 waves owns ONE episode and walks d in slices of FS_W = 128 features.
//   A. prototypes  thread t takes feature t & 127 of the slice and the class slots c = (t >> 7), (t >> 7) + 2, ...: it adds the
//      class's support rows in column order j = 0, 1, ... into one register and stores the running sum into P[s][c][feature]
//      (LDS) each time j + 1 reaches shot count s -- the shot counts are nested prefixes, and the prototype of shot count k is the
//      same chain of k additions whatever other counts are in the list.  A wave's loads are 256 contiguous bytes of one row.
//   B. norms and scores  the block is 16 GROUPS of 16 lanes (a DPP row); lane g of a group holds features g, g + 16, ..., g + 112
//      of the slice.  Group r squares and adds P[sc] for sc = r, r + 16, ... and takes the queries q = r, r + 16, ...: the
//      query's 8 features go to registers once (16 lanes read 64 contiguous bytes, 8 times) and are multiplied with every
//      P[sc] from LDS (the four groups of a wave read the same 16 addresses: broadcast, no bank conflict).  A lane's 8 products
//      are one fmaf chain, feature ascending; the 16 lanes go through row16_sum's fixed tree -- four DPP moves inside the row,
//      no trip through the LDS crossbar -- and one lane adds the slice's term to acc[q][sc] / nrm[sc] in LDS, slices ascending
//      (four prototypes go through the chains and trees side by side, which hides their latency and changes no bit):
//          dot(q, sc) = ((0 + T_0) + T_1) + ...,  T_i = tree over g of (fmaf chain over the 8 features of lane g in slice i)
//      a function of the rows and d alone.  Features past d are zeros on both sides (fmaf(0, 0, a) leaves a).
//   C. after the last slice thread u takes one (shot count, query): score = dot / sqrtf(norm2) (0 where norm2 == 0), the
//      arg-max over the class slots with the lowest slot winning a tie, the optional score / pred stores, a hit flag in LDS;
//      thread s < S counts the flags of shot count s and writes hits[s][e].
//
// WHY 128: LDS holds P [S N][128], acc [N Q][S N], nrm [S N] and the episode's two index rows.  At the limits (S N = 80,
// N Q = 320) that is 40 KiB + 100 KiB + 2.8 KiB = 146 272 bytes of gfx950's 160 KiB: one block per CU; slices of 256 features
// would need 186 KiB.  The allocation is dynamic and sized by the call, not by the limits: the usual 5-way (1, 5)-shot 15-query
// episode takes 8.6 KiB, so the 32 waves per CU (8 blocks; the kernel needs fewer than 64 VGPRs) bound the occupancy there and
// the row gathers of eight episodes are in flight on a CU at once.  The slice width is a constant so that no sum's order depends
// on the shape of the call.
//
// The kernel trusts the index tables (ops.fewshot_episodes range-checks host tables before the upload).  Rows are read with
// 4-byte loads only: d need not be a multiple of anything and no pointer 16-byte aligned.
#pragma once
#include <math.h>

#include "common.h"

namespace cstp {
namespace {

constexpr int FS_W = 128;                                  // features per slice
constexpr int FS_FPL = FS_W / 16;                          // features per lane of a 16-lane group
constexpr int FS_MAX_WAY = 20, FS_MAX_QUERY = 32, FS_MAX_NQ = 320, FS_MAX_SHOTS = 4, FS_MAX_SHOT = 16;
constexpr int FS_MAX_D = 8192, FS_MAX_E = 1 << 20;

// the sum of a DPP row (16 lanes) in every lane of it: quads, then the two quads of a half row, then the two half rows.  Every
// step adds two values that hold the same pair of partial sums in either order, so all 16 lanes end with the same bits.
template <int CTRL>
__device__ __forceinline__ float row_move(float x) {
  const int i = __builtin_bit_cast(int, x);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float row16_sum(float v) {
  v += row_move<0xB1>(v);                                  // quad_perm:[1,0,3,2]
  v += row_move<0x4E>(v);                                  // quad_perm:[2,3,0,1]
  v += row_move<0x141>(v);                                 // row_half_mirror
  v += row_move<0x140>(v);                                 // row_mirror
  return v;
}

inline size_t fewshot_lds_bytes(int n_way, int n_query, int n_shots, int kmax) {
  const size_t sn = (size_t)n_shots * n_way, nq = (size_t)n_way * n_query;
  return (sn * FS_W + nq * sn + sn + (size_t)n_way * kmax + nq + 2 * FS_MAX_SHOTS) * sizeof(float);
}

__global__ void __launch_bounds__(256)
fewshot_kernel(const float* __restrict__ xs, const float* __restrict__ xq, int d, const int* __restrict__ sup_idx,
               const int* __restrict__ qry_idx, int episodes, int n_way, int n_query, int n_shots, int kmax, int k0, int k1, int k2,
               int k3, int* __restrict__ hits, int* __restrict__ pred, float* __restrict__ score) {
  extern __shared__ float fs_smem[];
  const int tid = threadIdx.x, e = blockIdx.x;
  const int NQ = n_way * n_query, SN = n_shots * n_way;
  float* P = fs_smem;                                      // [SN][FS_W]
  float* acc = P + SN * FS_W;                              // [NQ][SN]
  float* nrm = acc + NQ * SN;                              // [SN]
  int* sidx = reinterpret_cast<int*>(nrm + SN);            // [n_way][kmax]
  int* qidx = sidx + n_way * kmax;                         // [NQ]
  int* shot = qidx + NQ;                                   // [2 * FS_MAX_SHOTS]: the counts, then zeros

  for (int i = tid; i < NQ * SN + SN; i += 256) acc[i] = 0.f;             // acc and nrm lie side by side
  for (int i = tid; i < n_way * kmax; i += 256) sidx[i] = sup_idx[(size_t)e * n_way * kmax + i];
  for (int i = tid; i < NQ; i += 256) qidx[i] = qry_idx[(size_t)e * NQ + i];
  if (tid == 0) {
    shot[0] = k0;
    shot[1] = k1;
    shot[2] = k2;
    shot[3] = k3;
    shot[4] = shot[5] = shot[6] = shot[7] = 0;
  }
  __syncthreads();

  const int g = tid & 15, grp = tid >> 4;                  // B: lane of the group, group of the block
  const int fl = tid & (FS_W - 1), half = tid >> 7;        // A: feature of the slice, parity of the class slots

  for (int f0 = 0; f0 < d; f0 += FS_W) {
    // A. the prototypes of this slice
    const bool fin = f0 + fl < d;
    for (int c = half; c < n_way; c += 2) {
      float p = 0.f;
      int s = 0;
#pragma unroll 4
      for (int j = 0; j < kmax; ++j) {
        const float v = fin ? xs[(size_t)sidx[c * kmax + j] * d + f0 + fl] : 0.f;
        p += v;                                                           // column order
        if (j + 1 == shot[s]) {                                           // block-uniform; shot[n_shots - 1] == kmax ends the loop
          P[(s * n_way + c) * FS_W + fl] = p;
          ++s;
        }
      }
    }
    __syncthreads();

    // B. square norms of the prototypes, then every query against every prototype
    for (int sc = grp; sc < SN; sc += 16) {
      const float* pr = P + sc * FS_W + g;
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < FS_FPL; ++i) a = fmaf(pr[16 * i], pr[16 * i], a);
      a = row16_sum(a);
      if (g == 0) nrm[sc] += a;
    }
    for (int q0 = 0; q0 < NQ; q0 += 16) {
      const int q = q0 + grp;
      const bool live = q < NQ;                                           // uniform over the group: a DPP row is all in or all out
      const float* row = xq + (size_t)qidx[live ? q : 0] * d + f0 + g;
      float qv[FS_FPL];
#pragma unroll
      for (int i = 0; i < FS_FPL; ++i) qv[i] = (live && f0 + g + 16 * i < d) ? row[16 * i] : 0.f;
      int sc = 0;
      for (; sc + 4 <= SN; sc += 4) {                                     // four prototypes at a time: four independent chains and
        const float* pr = P + sc * FS_W + g;                              // trees in flight, each the arithmetic of the loop below
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
        for (int i = 0; i < FS_FPL; ++i) {
          a0 = fmaf(qv[i], pr[16 * i], a0);
          a1 = fmaf(qv[i], pr[FS_W + 16 * i], a1);
          a2 = fmaf(qv[i], pr[2 * FS_W + 16 * i], a2);
          a3 = fmaf(qv[i], pr[3 * FS_W + 16 * i], a3);
        }
        a0 = row16_sum(a0);
        a1 = row16_sum(a1);
        a2 = row16_sum(a2);
        a3 = row16_sum(a3);
        if (live && g < 4) acc[q * SN + sc + g] += g == 0 ? a0 : g == 1 ? a1 : g == 2 ? a2 : a3;   // every lane holds all four
      }
      for (; sc < SN; ++sc) {
        const float* pr = P + sc * FS_W + g;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < FS_FPL; ++i) a = fmaf(qv[i], pr[16 * i], a);
        a = row16_sum(a);
        if (live && g == 0) acc[q * SN + sc] += a;
      }
    }
    __syncthreads();                                                      // the next slice's prototypes overwrite P
  }

  // C. divide, arg-max, count
  int* flag = reinterpret_cast<int*>(P);                                  // n_shots * NQ <= SN * FS_W: n_query <= 32 < FS_W
  for (int u = tid; u < n_shots * NQ; u += 256) {
    const int s = u / NQ, q = u - s * NQ;
    const size_t o = ((size_t)s * episodes + e) * NQ + q;
    int best = 0;
    float bv = 0.f;
    for (int c = 0; c < n_way; ++c) {
      const float n2 = nrm[s * n_way + c];
      const float v = n2 > 0.f ? acc[q * SN + s * n_way + c] / sqrtf(n2) : 0.f;
      if (score != nullptr) score[o * n_way + c] = v;
      if (c == 0 || v > bv) {                                             // strictly greater: the lowest slot keeps a tie
        bv = v;
        best = c;
      }
    }
    if (pred != nullptr) pred[o] = best;
    flag[u] = best == q / n_query ? 1 : 0;
  }
  __syncthreads();
  if (tid < n_shots) {
    int h = 0;
    for (int q = 0; q < NQ; ++q) h += flag[tid * NQ + q];
    hits[(size_t)tid * episodes + e] = h;
  }
}

}  // namespace
}  // namespace cstp

extern "C" int cstp_fewshot_episodes(void* stream, const float* xs, int32_t ns, const float* xq, int32_t nq, int32_t d,
                                     const int32_t* sup_idx, const int32_t* qry_idx, int32_t episodes, int32_t n_way,
                                     int32_t n_query, const int32_t* shots, int32_t n_shots, int32_t* hits, int32_t* pred,
                                     float* score) {
  using namespace cstp;
  CSTP_REQUIRE(xs != nullptr && xq != nullptr && sup_idx != nullptr && qry_idx != nullptr && shots != nullptr && hits != nullptr,
               "null argument");
  CSTP_REQUIRE(ns >= 1 && nq >= 1, "ns and nq must be at least 1");
  CSTP_REQUIRE(d >= 1 && d <= FS_MAX_D, "d must be in 1..8192");
  CSTP_REQUIRE(episodes >= 1 && episodes <= FS_MAX_E, "episodes must be in 1..2^20");
  CSTP_REQUIRE(n_way >= 2 && n_way <= FS_MAX_WAY, "n_way must be in 2..20");
  CSTP_REQUIRE(n_query >= 1 && n_query <= FS_MAX_QUERY, "n_query must be in 1..32");
  CSTP_REQUIRE(n_way * n_query <= FS_MAX_NQ, "n_way * n_query must be at most 320");
  CSTP_REQUIRE(n_shots >= 1 && n_shots <= FS_MAX_SHOTS, "n_shots must be in 1..4");
  int k[FS_MAX_SHOTS] = {0, 0, 0, 0};
  for (int i = 0; i < n_shots; ++i) {
    CSTP_REQUIRE(shots[i] >= 1 && shots[i] <= FS_MAX_SHOT, "shots must lie in 1..16");
    CSTP_REQUIRE(i == 0 || shots[i] > shots[i - 1], "shots must be strictly ascending");
    k[i] = shots[i];
  }
  const int kmax = k[n_shots - 1];
  const size_t lds = fewshot_lds_bytes(n_way, n_query, n_shots, kmax);
  if (lds > 64 * 1024) {                                                  // above the default cap of a dynamic allocation
    const hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(fewshot_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)lds);
    if (e_ != hipSuccess) return fail("hipFuncSetAttribute failed: %s (line %ld)", hipGetErrorString(e_), __LINE__);
  }
  hipLaunchKernelGGL(fewshot_kernel, dim3((unsigned)episodes), dim3(256), lds, as_stream(stream), xs, xq, d, sup_idx, qry_idx,
                     episodes, n_way, n_query, n_shots, kmax, k[0], k[1], k[2], k[3], hits, pred, score);
  CSTP_LAUNCH_CHECK();
  return 0;
}
