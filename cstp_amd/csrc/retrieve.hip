// Streaming similarity top-k for nearest-neighbour video retrieval: for every query row the k most similar gallery rows,
// without ever materialising the [nq][ng] similarity matrix.
//
//   sim(i, j) = sum_c q[i][c] * g[j][c]      (fp32 products, fp32 accumulation, c ascending: one fmaf chain per pair, the
//                                             arithmetic of v_mfma_f32_32x32x2_f32, so a pair's similarity does not depend
//                                             on the tile or the split it is computed in)
//
// simtopk_kernel: block = 256 threads = 4 waves owns SQ_TQ = 64 queries and walks its share of the gallery in tiles of
// SQ_TG = 128 rows.  Both operands stream through a double-buffered LDS image in chunks of SQ_BK = 32 features (global ->
// registers -> LDS, transposed to [feature][row] so that the MFMA fragments are conflict-free 32-lane reads); the query
// chunk is re-read per gallery tile from L2, where a 64 x d tile (<= 512 KiB at d = 2048) stays resident -- 64 x 2048
// floats do not fit the LDS, and one kernel serves every d.  Wave w multiplies the 64 queries by gallery columns
// [32w, 32w + 32): two 32x32 accumulators.  After the last chunk the 64 x 128 scores are written over the operand image and
// each wave selects for 16 of the query rows: a row's running list lives in one register pair per lane (lane l = slot l,
// sorted by similarity descending, then gallery index ascending; empty slots are (-inf, -1)).  64 candidates are compared at
// once against the row's k-th value -- one ballot, most die there -- and the survivors are inserted one by one, lowest
// gallery index first, at the slot a second ballot gives.  Candidates arrive in ascending gallery order, so "insert behind
// every slot that is >=" is the (similarity, index) order.
//
// With few query tiles the gallery is split over nsplit <= 32 blocks per query tile, each block writes its list to the
// workspace ([nsplit][nq][k] values, then indices) and simtopk_merge_kernel (one wave per query) pushes the lists through the
// same insertion in split order.  The k best under a total order are unique, so the answer does not depend on nsplit.
// No atomics of any kind: two calls give the same bits.  Every global index is formed from a row < nq / < ng and a feature
// < d that were checked first; masked elements are zeros (fmaf(0, 0, acc) leaves acc as it is).
//
// knn_vote_kernel: the weighted k-nearest-neighbour vote on such lists (include/cstp_hip.h: cstp_knn_vote).  One wave per
// query, four per block, lane j = slot j.  A lane's class sum is a k-step loop over the slots (readlane of the slot's label and
// weight, added where the label is the lane's own): slot order, so every slot of a class holds the same bits, and no class
// table in LDS or memory -- the number of classes is unbounded.  The first slot of a class represents it; the n_top answers are
// n_top wave-wide arg-max rounds over the representatives by (score descending, class ascending).
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace cstp {
namespace {

constexpr int SQ_TQ = 64, SQ_TG = 128, SQ_BK = 32;
constexpr int SQ_LDA = SQ_TQ + 1, SQ_LDB = SQ_TG + 1;      // odd row strides: the transposing stores spread over the banks
constexpr int SQ_LDS = SQ_TG + 1;                          // score image [64][129]
constexpr int SQ_BUF = SQ_BK * (SQ_LDA + SQ_LDB);          // floats per operand buffer
constexpr int SQ_SMEM = 2 * SQ_BUF > SQ_TQ * SQ_LDS ? 2 * SQ_BUF : SQ_TQ * SQ_LDS;
constexpr int SQ_MAX_K = 64, SQ_MAX_SPLIT = 32;
constexpr int SQ_FILL_BLOCKS = 256;                        // one block per CU
constexpr int SQ_MIN_TILES = 4;                            // gallery tiles per split block, at least

typedef float floatx16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float lane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// lane l receives lane l - 1's value (lane 0 keeps its own): one DPP move, no trip through the LDS crossbar
__device__ __forceinline__ int lane_up1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

// Offers one candidate per lane (ok: the lane holds one) to a row's sorted list (sv, si: slot = lane).  Candidates of one call
// and of successive calls must come in ascending index order, and after every index already in the list.
__device__ __forceinline__ void topk_push(float& sv, int& si, float v, int j, bool ok, int k, int lane) {
  float thr = lane_f(sv, k - 1);
  unsigned long long m = __ballot(ok && v > thr);
  while (m != 0) {
    const int b = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    m &= m - 1;
    const float cv = lane_f(v, b);
    const int cj = __builtin_amdgcn_readlane(j, b);
    if (!(cv > thr)) continue;                                  // the list moved on since the ballot
    const int p = __popcll(__ballot(sv >= cv));                 // sorted list: the slots that stay in front are a prefix, p < k
    const float uv = __builtin_bit_cast(float, lane_up1(__builtin_bit_cast(int, sv)));
    const int ui = lane_up1(si);
    if (lane == p) {
      sv = cv;
      si = cj;
    } else if (lane > p) {
      sv = uv;
      si = ui;
    }
    thr = lane_f(sv, k - 1);
  }
}

// ---- the walk that simtopk_kernel, kmeans_assign_kernel (kmeans.h) and pairpot_kernel (health.h) share ------------------------
// staging: element e = tid + 256 p of a chunk is row e >> 3 (srow = tid >> 3), features 4 (e & 7) .. + 3 (sc4 = 4 (tid & 7))
template <bool VEC4>
__device__ __forceinline__ void sq_load_rows(const float* __restrict__ base, int row0, int nrows, int c0, int d, int srow, int sc4,
                                             float4* dst, int np) {
#pragma unroll
  for (int p = 0; p < np; ++p) {
    const int row = row0 + srow + 32 * p, c = c0 + sc4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nrows) {
      const float* src = base + (size_t)row * d + c;
      if (VEC4) {
        if (c < d) v = *reinterpret_cast<const float4*>(src);   // d % 4 == 0: the four features are in or out together
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

__device__ __forceinline__ void sq_store_rows(float* dst, int ld, const float4* src, int np, int srow, int sc4) {
#pragma unroll
  for (int p = 0; p < np; ++p) {
    float* o = dst + sc4 * ld + srow + 32 * p;
    o[0] = src[p].x;
    o[ld] = src[p].y;
    o[2 * ld] = src[p].z;
    o[3 * ld] = src[p].w;
  }
}

// one chunk of SQ_BK steps from an operand buffer ([k][64 A rows] at stride SQ_LDA, then [k][128 B rows] at stride SQ_LDB): wave w
// multiplies the 64 A rows by B rows [32 w, 32 w + 32), k ascending
__device__ __forceinline__ void sq_mma_chunk(const float* buf, int lrow, int lcol, int wave, floatx16& acc0, floatx16& acc1) {
  const float* Ab = buf + lrow * SQ_LDA + lcol;
  const float* Bb = buf + SQ_BK * SQ_LDA + lrow * SQ_LDB + wave * 32 + lcol;
#pragma unroll
  for (int kk = 0; kk < SQ_BK; kk += 2) {
    const float b = Bb[kk * SQ_LDB];
    const float a0 = Ab[kk * SQ_LDA], a1 = Ab[kk * SQ_LDA + 32];
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
  }
}

// The 64 x 128 similarities of rows [q0, q0 + 64) of q and rows [g0, g0 + 128) of g -> smem[row * SQ_LDS + column], behind a
// barrier.  On entry qa / ga hold chunk 0 of this tile; on exit chunk 0 of the tile at g_next (< 0: there is none), its loads
// still in flight.  The caller puts a barrier between its reads of the scores and the next call.
template <bool VEC4>
__device__ __forceinline__ void sq_tile_scores(float* smem, const float* __restrict__ q, int q0, int nq, const float* __restrict__ g,
                                               int g0, int ng, int g_next, int d, float4* qa, float4* ga) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lrow = lane >> 5, lcol = lane & 31;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  const int nchunk = (d + SQ_BK - 1) / SQ_BK;
  floatx16 acc0 = {0}, acc1 = {0};
  sq_store_rows(smem, SQ_LDA, qa, 2, srow, sc4);        // chunk 0 of this tile: loaded during the last chunk of the tile before
  sq_store_rows(smem + SQ_BK * SQ_LDA, SQ_LDB, ga, 4, srow, sc4);
  __syncthreads();
  int buf = 0;
  for (int kc = 0; kc < nchunk; ++kc) {
    const bool have_next = kc + 1 < nchunk;
    if (have_next) {
      sq_load_rows<VEC4>(q, q0, nq, (kc + 1) * SQ_BK, d, srow, sc4, qa, 2);
      sq_load_rows<VEC4>(g, g0, ng, (kc + 1) * SQ_BK, d, srow, sc4, ga, 4);
    } else if (g_next >= 0) {                           // in flight across the caller's work on the scores
      sq_load_rows<VEC4>(q, q0, nq, 0, d, srow, sc4, qa, 2);
      sq_load_rows<VEC4>(g, g_next, ng, 0, d, srow, sc4, ga, 4);
    }
    sq_mma_chunk(smem + buf * SQ_BUF, lrow, lcol, wave, acc0, acc1);
    if (have_next) {
      float* nb = smem + (buf ^ 1) * SQ_BUF;
      sq_store_rows(nb, SQ_LDA, qa, 2, srow, sc4);
      sq_store_rows(nb + SQ_BK * SQ_LDA, SQ_LDB, ga, 4, srow, sc4);
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

template <bool VEC4>
__global__ void __launch_bounds__(256)
simtopk_kernel(const float* __restrict__ q, const float* __restrict__ g, int nq, int ng, int d, int k, int exclude_self,
               int tiles_per_split, float* __restrict__ out_val, int* __restrict__ out_idx) {
  __shared__ float smem[SQ_SMEM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * SQ_TQ;
  const int gtiles = (ng + SQ_TG - 1) / SQ_TG;
  const int t_begin = blockIdx.y * tiles_per_split;
  const int t_end = t_begin + tiles_per_split < gtiles ? t_begin + tiles_per_split : gtiles;
  float lv[16];
  int li[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    lv[r] = -INFINITY;
    li[r] = -1;
  }

  const int srow = tid >> 3, sc4 = (tid & 7) * 4;
  float4 qa[2], ga[4];
  if (t_begin < t_end) {
    sq_load_rows<VEC4>(q, q0, nq, 0, d, srow, sc4, qa, 2);
    sq_load_rows<VEC4>(g, t_begin * SQ_TG, ng, 0, d, srow, sc4, ga, 4);
  }
  for (int t = t_begin; t < t_end; ++t) {
    const int g0 = t * SQ_TG;
    sq_tile_scores<VEC4>(smem, q, q0, nq, g, g0, ng, t + 1 < t_end ? g0 + SQ_TG : -1, d, qa, ga);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 16 + r, i = q0 + row;
      if (i < nq) {                                                       // wave-uniform
#pragma unroll
        for (int h = 0; h < SQ_TG; h += 64) {
          const int j = g0 + h + lane;
          const bool ok = j < ng && !(exclude_self != 0 && j == i);
          topk_push(lv[r], li[r], smem[row * SQ_LDS + h + lane], j, ok, k, lane);
        }
      }
    }
    __syncthreads();                                                      // the next tile's stores overwrite the scores
  }

  if (lane < k) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = q0 + wave * 16 + r;
      if (i < nq) {
        const size_t o = ((size_t)blockIdx.y * nq + i) * k + lane;
        out_val[o] = lv[r];
        out_idx[o] = li[r];
      }
    }
  }
}

// one wave per query: the nsplit partial lists (each sorted, split s holding lower gallery rows than split s + 1) -> the answer
__global__ void __launch_bounds__(256)
simtopk_merge_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int nq, int k, int nsplit,
                     float* __restrict__ val, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nq) return;                                                    // wave-uniform
  float sv = -INFINITY;
  int si = -1;
  for (int s = 0; s < nsplit; ++s) {
    float v = -INFINITY;
    int j = -1;
    if (lane < k) {
      const size_t o = ((size_t)s * nq + i) * k + lane;
      v = pv[o];
      j = pi[o];
    }
    topk_push(sv, si, v, j, j >= 0, k, lane);
  }
  if (lane < k) {
    val[(size_t)i * k + lane] = sv;
    idx[(size_t)i * k + lane] = si;
  }
}

constexpr int KV_MAX_TOP = 8;

// one wave per query: val / idx [nq][k] as simtopk writes them -> the n_top best classes of the weighted vote
__global__ void __launch_bounds__(256)
knn_vote_kernel(const float* __restrict__ val, const int* __restrict__ idx, const int* __restrict__ g_labels, int nq, int ng,
                int k, float inv_t, int n_top, int* __restrict__ pred, float* __restrict__ score) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nq) return;                                                  // wave-uniform
  float v = -INFINITY;
  int j = -1;
  if (lane < k) {
    v = val[(size_t)row * k + lane];
    j = idx[(size_t)row * k + lane];
  }
  const bool live = j >= 0 && j < ng;                                     // lanes >= k kept j = -1
  const int lab = live ? g_labels[j] : -1;                                // a dead slot's idx never forms an address
  const float v0 = lane_f(v, 0);                                          // the row's largest value: w_0 = 1, no overflow
  const float w = live ? expf((v - v0) * inv_t) : 0.f;
  float sum = 0.f;
  bool rep = live;                                                        // the first slot of a class stands for it
  for (int s = 0; s < k; ++s) {
    const int ls = __builtin_amdgcn_readlane(lab, s);
    const float ws = lane_f(w, s);
    if (ls == lab) {
      sum += ws;                                                          // s ascending: one order for every slot of the class
      if (s < lane) rep = false;
    }
  }
  int out_c = -1;
  float out_s = 0.f;
  for (int r = 0; r < n_top; ++r) {
    float bs = rep ? sum : -1.f;                                          // scores are >= 0: -1 is "no candidate"
    int bc = rep ? lab : 0x7fffffff;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off, 64);
      const int oc = __shfl_xor(bc, off, 64);
      if (os > bs || (os == bs && oc < bc)) {
        bs = os;
        bc = oc;
      }
    }
    if (bs < 0.f) break;                                                  // wave-uniform: the distinct classes ran out
    if (lane == r) {
      out_c = bc;
      out_s = bs;
    }
    if (rep && lab == bc) rep = false;
  }
  if (lane < n_top) {
    pred[(size_t)row * n_top + lane] = out_c;
    score[(size_t)row * n_top + lane] = out_s;
  }
}

inline bool shape_ok(int nq, int ng, int d, int k) {
  return nq >= 1 && ng >= 1 && d >= 1 && k >= 1 && k <= SQ_MAX_K && (long)ng + SQ_TG < (1L << 31) &&
         (long)nq + SQ_TQ < (1L << 31);
}

// blocks along the gallery per query tile, and the gallery tiles each of them walks (none is left without a tile)
int split_of(int nq, int ng, int* tiles_per_split) {
  const int qtiles = cdiv(nq, SQ_TQ), gtiles = cdiv(ng, SQ_TG);
  int ns = SQ_FILL_BLOCKS / qtiles;
  if (ns > gtiles / SQ_MIN_TILES) ns = gtiles / SQ_MIN_TILES;
  if (ns > SQ_MAX_SPLIT) ns = SQ_MAX_SPLIT;
  if (const char* e = getenv("CSTP_SIMTOPK_NSPLIT")) {                    // developer override (tests pin the unsplit path)
    const int v = atoi(e);
    if (v >= 1 && v <= SQ_MAX_SPLIT) ns = v < gtiles ? v : gtiles;
  }
  if (ns < 1) ns = 1;
  const int per = cdiv(gtiles, ns);
  *tiles_per_split = per;
  return cdiv(gtiles, per);
}

inline size_t partial_bytes(int nsplit, int nq, int k) {
  return nsplit > 1 ? align_up((size_t)nsplit * nq * k * sizeof(float), 256) : 0;     // one of the two planes
}

}  // namespace
}  // namespace cstp

using namespace cstp;

extern "C" size_t cstp_simtopk_workspace_bytes(int32_t nq, int32_t ng, int32_t d, int32_t k) {
  if (!shape_ok(nq, ng, d, k)) return 0;
  int per = 0;
  const int ns = split_of(nq, ng, &per);
  return 2 * partial_bytes(ns, nq, k) + 256;
}

extern "C" int cstp_simtopk(void* stream, const float* q, const float* g, int32_t nq, int32_t ng, int32_t d, int32_t k,
                            int32_t exclude_self, float* val, int32_t* idx, void* ws, size_t ws_bytes) {
  CSTP_REQUIRE(k >= 1 && k <= SQ_MAX_K, "k must be in 1..64");
  CSTP_REQUIRE(shape_ok(nq, ng, d, k), "bad shape");
  CSTP_REQUIRE(q != nullptr && g != nullptr && val != nullptr && idx != nullptr && ws != nullptr, "null argument");
  CSTP_REQUIRE(ws_bytes >= cstp_simtopk_workspace_bytes(nq, ng, d, k), "workspace too small");
  int per = 0;
  const int ns = split_of(nq, ng, &per);
  float* pv = ns > 1 ? reinterpret_cast<float*>(ws) : val;
  int* pi = ns > 1 ? reinterpret_cast<int*>(reinterpret_cast<char*>(ws) + partial_bytes(ns, nq, k)) : idx;
  const bool v4 = (d & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(g)) & 15u) == 0;
  hipStream_t st = as_stream(stream);
  const dim3 grid(cdiv(nq, SQ_TQ), ns);
  if (v4) hipLaunchKernelGGL(simtopk_kernel<true>, grid, dim3(256), 0, st, q, g, nq, ng, d, k, exclude_self, per, pv, pi);
  else hipLaunchKernelGGL(simtopk_kernel<false>, grid, dim3(256), 0, st, q, g, nq, ng, d, k, exclude_self, per, pv, pi);
  CSTP_LAUNCH_CHECK();
  if (ns > 1) {
    hipLaunchKernelGGL(simtopk_merge_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, st, pv, pi, nq, k, ns, val, idx);
    CSTP_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int cstp_knn_vote(void* stream, const float* val, const int32_t* idx, const int32_t* g_labels, int32_t nq, int32_t ng,
                             int32_t k, float inv_t, int32_t n_top, int32_t* pred, float* score) {
  CSTP_REQUIRE(val != nullptr && idx != nullptr && g_labels != nullptr && pred != nullptr && score != nullptr, "null argument");
  CSTP_REQUIRE(nq >= 1 && ng >= 1, "bad shape");
  CSTP_REQUIRE(k >= 1 && k <= SQ_MAX_K, "k must be in 1..64");
  CSTP_REQUIRE(n_top >= 1 && n_top <= KV_MAX_TOP, "n_top must be in 1..8");
  CSTP_REQUIRE(isfinite(inv_t) && inv_t > 0.f, "inv_t must be finite and positive");
  const unsigned blocks = (unsigned)(((long)nq + 3) / 4);
  hipLaunchKernelGGL(knn_vote_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), val, idx, g_labels, nq, ng, k, inv_t, n_top,
                     pred, score);
  CSTP_LAUNCH_CHECK();
  return 0;
}

#include "probe.h"  // the linear probe on cached features: cstp_probe_step, cstp_probe_predict
#include "ntxq.h"   // NT-Xent with a queue of negatives: cstp_ntxq_forward, cstp_ntxq_backward, cstp_ntxq_push
#include "kmeans.h"  // spherical k-means on cached features: cstp_kmeans_assign, cstp_kmeans_update
#include "health.h"  // label-free collapse metrics on cached features: cstp_feat_gram, cstp_pair_potential
#include "fewshot.h"  // few-shot episodic evaluation on cached features: cstp_fewshot_episodes
