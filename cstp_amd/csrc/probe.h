// Linear probe on cached features (cstp_probe_step / cstp_probe_predict, spec in include/cstp_hip.h): a softmax classifier on
// rows gathered from a feature matrix x [n][d], standardised on load -- no standardised copy, no logits table in memory.
//
// The operand that streams is the activation matrix (1 000 - 10 000 rows), the classes are few (<= 1024) and the arithmetic
// (2 m d c FLOP) is small next to the launches and the traffic, so both products are plain fp32 FMA tiles through LDS:
//   1. probe_logits_kernel<MODE>  block = 256 threads owns PR_TM = 8 rows.  Per tile of PR_CT = 128 classes it walks d in chunks
//      of PR_BK = 32 (global -> registers -> LDS, the next chunk in flight while the current one is multiplied); lane = class,
//      wave = row pair, one fmaf chain per (row, class) in feature order.  The slab's logits stay in LDS ([8][c] floats); a wave
//      then owns two rows: arg-max (lowest class id first), soft-max about the row maximum, and
//        STEP:    g = (p - onehot) / m as [m][cpad] into the workspace (cpad = c rounded up to 4, padding zero), row loss, row hit
//        score:   row loss and row hit only
//        predict: n_top rounds of a wave-wide arg-max over what comes after the previous pick in (logit desc, class asc)
//   2. probe_wgrad_kernel   block owns a 64 class x 64 feature tile of dw and one slice of the rows; 16 rows of g and of the
//      standardised x per LDS chunk, thread = 4 x 4 outputs, one fmaf chain per output over the slice's rows ascending.  The
//      blocks of the first feature tile also sum g over their rows: the slice's db.
//   3. probe_fold_kernel    dw = the slices' partials added in slice order (skipped with one slice: launch 2 wrote dw itself);
//      its last block folds db the same way and sums row loss (in double) and row hits in one fixed tree.
// Every sum has one writer and one order: no atomics, equal inputs give equal bits.  A gathered index outside [0, n) or a label
// outside [0, c) is compared, never used to form an address: the row's x is taken as zeros and its g, loss and hit are zero.
//
// Sweep (cstp_probe_sweep_step / cstp_probe_sweep_score): `heads` classifiers on the same batch in the same launches.  Head h
// reads (w, b) + h * head_stride floats, writes (dw, db) at the same stride and owns workspace bytes [h * round16(single),
// (h + 1) * round16(single)), laid out as the single-head workspace is.  The head is blockIdx.y of launches 1 and 3 and a factor
// of blockIdx.z of launch 2 (z = head * slices + slice); everything else -- chains, reductions, slices, fold order -- is the
// single-head code, which the old entry points run with heads = 1, so head h has the bits of the single-head call on (W_h, b_h).
// LDS per block is unchanged (8 c floats dynamic): heads multiply blocks, not a block's footprint.  Score mode writes row loss
// and row hit only (no g, no launch 2) and its fold block sums them: two launches.
#pragma once
#include <math.h>

#include "common.h"

namespace cstp {
namespace {

constexpr int PR_TM = 8, PR_CT = 128, PR_BK = 32, PR_LDK = PR_BK + 4;   // 144-byte LDS rows: 16 lanes' b128 reads hit 16 slots
constexpr int PR_MAX_C = 1024, PR_MAX_TOP = 8;
constexpr int PR_GT = 64, PR_GR = 16;                                   // wgrad: tile edge, rows per LDS chunk
constexpr int PR_MAX_SLICE = 32, PR_FILL_BLOCKS = 512;

// p[base + k .. k + 3] with zeros from feature d on; vec: d % 4 == 0 and p 16-byte aligned (then k < d means k + 3 < d)
__device__ __forceinline__ float4 pr_load4(const float* __restrict__ p, size_t base, int k, int d, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    if (k < d) v = *reinterpret_cast<const float4*>(p + base + k);
  } else {
    if (k < d) v.x = p[base + k];
    if (k + 1 < d) v.y = p[base + k + 1];
    if (k + 2 < d) v.z = p[base + k + 2];
    if (k + 3 < d) v.w = p[base + k + 3];
  }
  return v;
}

// the standardisation constants of features k .. k + 3: (0, 1) where the vector is NULL, (0, 0) from feature d on
__device__ __forceinline__ void pr_consts(const float* __restrict__ mean, const float* __restrict__ inv_std, int k, int d, bool vec,
                                          float4& mu, float4& is) {
  mu = mean != nullptr ? pr_load4(mean, 0, k, d, vec) : make_float4(0.f, 0.f, 0.f, 0.f);
  is = inv_std != nullptr ? pr_load4(inv_std, 0, k, d, vec) : make_float4(1.f, 1.f, 1.f, 1.f);
}

__device__ __forceinline__ float4 pr_std(float4 v, float4 mu, float4 is) {
  return make_float4((v.x - mu.x) * is.x, (v.y - mu.y) * is.y, (v.z - mu.z) * is.z, (v.w - mu.w) * is.w);
}

// the source row of batch row r, or -1: rows[r] is compared against [0, n) before anything is read through it
__device__ __forceinline__ int pr_source(const int32_t* __restrict__ rows, int r, int m, int n) {
  if (r >= m) return -1;
  const int s = rows != nullptr ? rows[r] : r;
  return s >= 0 && s < n ? s : -1;
}

// vec bits: 1 = x rows, 2 = w rows, 4 = mean / inv_std may be read as float4
// MODE: PR_PREDICT ranks classes; PR_STEP writes g, row loss, row hit; PR_SCORE row loss and row hit only.  blockIdx.y = head:
// w, b advance by head_stride floats, g / row_loss / row_hit by ws_stride floats (both 0 with one head)
enum { PR_PREDICT = 0, PR_STEP = 1, PR_SCORE = 2 };

template <int MODE>
__global__ void __launch_bounds__(256)
probe_logits_kernel(const float* __restrict__ x, const int32_t* __restrict__ rows, const int64_t* __restrict__ labels,
                    const float* __restrict__ mean, const float* __restrict__ inv_std, const float* __restrict__ w,
                    const float* __restrict__ b, size_t head_stride, size_t ws_stride, int m, int n, int d, int c, int cpad, int vec,
                    float inv_m, float* __restrict__ g, float* __restrict__ row_loss, int* __restrict__ row_hit, int n_top,
                    int* __restrict__ pred, float* __restrict__ score) {
  constexpr bool STEP = MODE != PR_PREDICT;
  if (STEP && blockIdx.y != 0) {
    w += blockIdx.y * head_stride;
    b += blockIdx.y * head_stride;
    if (MODE == PR_STEP) g += blockIdx.y * ws_stride;
    row_loss += blockIdx.y * ws_stride;
    row_hit += blockIdx.y * ws_stride;
  }
  extern __shared__ float Ls[];                                           // [PR_TM][c] logits of the slab
  __shared__ __attribute__((aligned(16))) float Ws[PR_CT * PR_LDK];
  __shared__ __attribute__((aligned(16))) float Xs[PR_TM * PR_LDK];
  __shared__ int Rs[PR_TM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * PR_TM;
  if (tid < PR_TM) Rs[tid] = pr_source(rows, m0 + tid, m, n);
  __syncthreads();

  // staging: thread -> features k4 .. k4 + 3 of W rows (tid >> 3) + 32 p and (tid < 64) of x row tid >> 3
  const int srow = tid >> 3, k4 = (tid & 7) * 4;
  const int xsrc = tid < 64 ? Rs[srow] : -1;
  const bool vx = vec & 1, vw = vec & 2, vm = vec & 4;
  const int nchunk = (d + PR_BK - 1) / PR_BK;
  float4 wreg[4], xreg = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int ct0 = 0; ct0 < c; ct0 += PR_CT) {
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int cls = ct0 + srow + 32 * p;
        wreg[p] = cls < c ? pr_load4(w, (size_t)cls * d, k0 + k4, d, vw) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (xsrc >= 0) {
        float4 mu, is;
        pr_consts(mean, inv_std, k0 + k4, d, vm, mu, is);
        xreg = pr_std(pr_load4(x, (size_t)xsrc * d, k0 + k4, d, vx), mu, is);
      }
    };
    float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;                     // (row 2 wave + i, class ct0 + lane + 64 j)
    fetch(0);
    for (int ch = 0; ch < nchunk; ++ch) {
      __syncthreads();                                                    // the previous chunk has been multiplied
#pragma unroll
      for (int p = 0; p < 4; ++p) *reinterpret_cast<float4*>(&Ws[(srow + 32 * p) * PR_LDK + k4]) = wreg[p];
      if (tid < 64) *reinterpret_cast<float4*>(&Xs[srow * PR_LDK + k4]) = xreg;
      __syncthreads();
      if (ch + 1 < nchunk) fetch((ch + 1) * PR_BK);
#pragma unroll
      for (int kk = 0; kk < PR_BK; kk += 4) {
        const float4 w0 = *reinterpret_cast<const float4*>(&Ws[lane * PR_LDK + kk]);
        const float4 w1 = *reinterpret_cast<const float4*>(&Ws[(lane + 64) * PR_LDK + kk]);
        const float4 x0 = *reinterpret_cast<const float4*>(&Xs[(2 * wave) * PR_LDK + kk]);
        const float4 x1 = *reinterpret_cast<const float4*>(&Xs[(2 * wave + 1) * PR_LDK + kk]);
        a00 = fmaf(x0.x, w0.x, a00); a00 = fmaf(x0.y, w0.y, a00); a00 = fmaf(x0.z, w0.z, a00); a00 = fmaf(x0.w, w0.w, a00);
        a01 = fmaf(x0.x, w1.x, a01); a01 = fmaf(x0.y, w1.y, a01); a01 = fmaf(x0.z, w1.z, a01); a01 = fmaf(x0.w, w1.w, a01);
        a10 = fmaf(x1.x, w0.x, a10); a10 = fmaf(x1.y, w0.y, a10); a10 = fmaf(x1.z, w0.z, a10); a10 = fmaf(x1.w, w0.w, a10);
        a11 = fmaf(x1.x, w1.x, a11); a11 = fmaf(x1.y, w1.y, a11); a11 = fmaf(x1.z, w1.z, a11); a11 = fmaf(x1.w, w1.w, a11);
      }
    }
    const int c0 = ct0 + lane, c1 = c0 + 64;
    if (c0 < c) {
      const float bb = b[c0];
      Ls[(2 * wave) * c + c0] = a00 + bb;
      Ls[(2 * wave + 1) * c + c0] = a10 + bb;
    }
    if (c1 < c) {
      const float bb = b[c1];
      Ls[(2 * wave) * c + c1] = a01 + bb;
      Ls[(2 * wave + 1) * c + c1] = a11 + bb;
    }
  }
  __syncthreads();

  for (int i = 0; i < 2; ++i) {
    const int lrow = 2 * wave + i, r = m0 + lrow;
    if (r >= m) break;                                                    // wave-uniform
    const float* L = Ls + lrow * c;
    if (STEP) {
      float bv = -INFINITY;
      int bc = 0x7fffffff;
      for (int k = lane; k < c; k += 64) {
        const float v = L[k];
        if (v > bv) {                                                     // k ascending: the first of equal values stays
          bv = v;
          bc = k;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oc = __shfl_xor(bc, off, 64);
        if (ov > bv || (ov == bv && oc < bc)) {
          bv = ov;
          bc = oc;
        }
      }
      float sum = 0.f;
      for (int k = lane; k < c; k += 64) sum += expf(L[k] - bv);
      sum = wave_sum_all(sum);
      const int src = Rs[lrow];
      const int64_t y64 = src >= 0 ? labels[src] : -1;
      const bool valid = src >= 0 && y64 >= 0 && y64 < c;
      const int y = valid ? (int)y64 : -1;
      if (MODE == PR_STEP) {
        const float inv_sum = 1.f / sum;
        for (int k = lane; k < cpad; k += 64) {
          float gv = 0.f;
          if (valid && k < c) gv = (expf(L[k] - bv) * inv_sum - (k == y ? 1.f : 0.f)) * inv_m;
          g[(size_t)r * cpad + k] = gv;
        }
      }
      if (lane == 0) {
        row_loss[r] = valid ? (logf(sum) + bv) - L[y] : 0.f;
        row_hit[r] = valid && bc == y ? 1 : 0;
      }
    } else {
      float pv = INFINITY, out_s = 0.f;
      int pc = -1, out_c = -1;
      for (int t = 0; t < n_top; ++t) {
        float bv = -INFINITY;
        int bc = 0x7fffffff;
        for (int k = lane; k < c; k += 64) {
          const float v = L[k];
          const bool after = v < pv || (v == pv && k > pc);               // not yet picked
          if (after && (bc == 0x7fffffff || v > bv)) {
            bv = v;
            bc = k;
          }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const float ov = __shfl_xor(bv, off, 64);
          const int oc = __shfl_xor(bc, off, 64);
          if (oc != 0x7fffffff && (bc == 0x7fffffff || ov > bv || (ov == bv && oc < bc))) {
            bv = ov;
            bc = oc;
          }
        }
        if (bc == 0x7fffffff) break;                                      // wave-uniform: the classes ran out
        if (lane == t) {
          out_c = bc;
          out_s = bv;
        }
        pv = bv;
        pc = bc;
      }
      if (lane < n_top) {
        pred[(size_t)r * n_top + lane] = out_c;
        score[(size_t)r * n_top + lane] = out_s;
      }
    }
  }
}

// out: dw when nslice == 1, otherwise the partials [slice][c][d]; dbp [slice][c].  blockIdx.z = head * nslice + slice: g and dbp
// advance by ws_stride floats per head, out by out_stride (the workspace stride for partials, the head stride for dw itself)
__global__ void __launch_bounds__(256)
probe_wgrad_kernel(const float* __restrict__ x, const int32_t* __restrict__ rows, const float* __restrict__ mean,
                   const float* __restrict__ inv_std, const float* __restrict__ g, int m, int n, int d, int c, int cpad, int vec,
                   int rows_per_slice, int nslice, size_t ws_stride, size_t out_stride, float* __restrict__ out,
                   float* __restrict__ dbp) {
  __shared__ __attribute__((aligned(16))) float Gs[PR_GR * PR_GT];
  __shared__ __attribute__((aligned(16))) float Xs[PR_GR * PR_GT];
  const int tid = threadIdx.x, tc = tid & 15, td = tid >> 4;
  const int d0 = blockIdx.x * PR_GT, c0 = blockIdx.y * PR_GT, head = blockIdx.z / nslice, slice = blockIdx.z - head * nslice;
  if (head != 0) {
    g += head * ws_stride;
    dbp += head * ws_stride;
    out += head * out_stride;
  }
  const int r_begin = slice * rows_per_slice;
  const int r_end = r_begin + rows_per_slice < m ? r_begin + rows_per_slice : m;
  const bool vx = vec & 1, vm = vec & 4, vo = vec & 8;
  const int srow = tid >> 4, s4 = (tid & 15) * 4;                         // staging: chunk row, 4 classes / 4 features
  float4 mu, is;
  pr_consts(mean, inv_std, d0 + s4, d, vm, mu, is);                       // the thread stages the same features in every chunk
  float4 greg, xreg;
  auto fetch = [&](int r0) __attribute__((always_inline)) {
    const int r = r0 + srow;
    greg = make_float4(0.f, 0.f, 0.f, 0.f);
    xreg = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < r_end) {
      if (c0 + s4 < cpad) greg = *reinterpret_cast<const float4*>(g + (size_t)r * cpad + c0 + s4);
      const int src = pr_source(rows, r, m, n);
      if (src >= 0) xreg = pr_std(pr_load4(x, (size_t)src * d, d0 + s4, d, vx), mu, is);
    }
  };
  float acc[4][4];
  float gs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  fetch(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += PR_GR) {
    __syncthreads();
    *reinterpret_cast<float4*>(&Gs[srow * PR_GT + s4]) = greg;
    *reinterpret_cast<float4*>(&Xs[srow * PR_GT + s4]) = xreg;
    __syncthreads();
    if (r0 + PR_GR < r_end) fetch(r0 + PR_GR);
#pragma unroll
    for (int rr = 0; rr < PR_GR; ++rr) {                                  // rows past r_end are zeros
      const float4 ga = *reinterpret_cast<const float4*>(&Gs[rr * PR_GT + 4 * tc]);
      const float4 xa = *reinterpret_cast<const float4*>(&Xs[rr * PR_GT + 4 * td]);
      const float gv[4] = {ga.x, ga.y, ga.z, ga.w}, xv[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gs[i] += gv[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(gv[i], xv[j], acc[i][j]);
      }
    }
  }
  float* o = out + (size_t)slice * c * d;
  const int col = d0 + 4 * td;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cls = c0 + 4 * tc + i;
    if (cls >= c) continue;
    float* dst = o + (size_t)cls * d + col;
    if (vo) {
      if (col < d) *reinterpret_cast<float4*>(dst) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col + j < d) dst[j] = acc[i][j];
    }
    if (blockIdx.x == 0 && td == 0) dbp[(size_t)slice * c + cls] = gs[i];
  }
}

// blockIdx.y = head: the workspace operands advance by ws_stride floats, dw / db by head_stride, loss / hits by one.  db NULL
// (score): the last block sums row loss and row hits only
__global__ void __launch_bounds__(256)
probe_fold_kernel(const float* __restrict__ partial, int nslice, size_t cd, int fold_blocks, float* __restrict__ dw,
                  const float* __restrict__ dbp, int c, float* __restrict__ db, const float* __restrict__ row_loss,
                  const int* __restrict__ row_hit, int m, float* __restrict__ loss, int* __restrict__ hits, size_t head_stride,
                  size_t ws_stride) {
  __shared__ double sd[16];
  __shared__ int si[16];
  const int tid = threadIdx.x;
  if (blockIdx.y != 0) {
    const size_t h = blockIdx.y;
    partial += h * ws_stride;
    dbp += h * ws_stride;
    row_loss += h * ws_stride;
    row_hit += h * ws_stride;
    if (dw != nullptr) dw += h * head_stride;
    if (db != nullptr) db += h * head_stride;
    loss += h;
    hits += h;
  }
  if ((int)blockIdx.x < fold_blocks) {
    const size_t i = (size_t)blockIdx.x * 256 + tid;
    if (i < cd) {
      float s = 0.f;
      for (int sl = 0; sl < nslice; ++sl) s += partial[(size_t)sl * cd + i];
      dw[i] = s;
    }
    return;
  }
  if (db != nullptr) {
    for (int k = tid; k < c; k += 256) {
      float s = 0.f;
      for (int sl = 0; sl < nslice; ++sl) s += dbp[(size_t)sl * c + k];
      db[k] = s;
    }
  }
  double l = 0.0;
  int h = 0;
  for (int r = tid; r < m; r += 256) {
    l += (double)row_loss[r];
    h += row_hit[r];
  }
  l = block_sum(l, sd);
  h = block_sum(h, si);
  if (tid == 0) {
    loss[0] = (float)(l / (double)m);
    hits[0] = h;
  }
}

inline bool probe_shape_ok(int m, int n, int d, int c) {
  return m >= 1 && n >= 1 && d >= 1 && c >= 2 && c <= PR_MAX_C && (long)c * d < (1L << 31) && (long)m + PR_TM < (1L << 31) &&
         (long)n < (1L << 31) - 1;
}

inline int probe_cpad(int c) { return (c + 3) & ~3; }

// the row slices of launch 2, as the workspace is sized for them: enough blocks to fill the device, at least 64 rows each
inline int probe_slices(int m, int d, int c) {
  int s = PR_FILL_BLOCKS / (cdiv(d, PR_GT) * cdiv(c, PR_GT));
  if (s > PR_MAX_SLICE) s = PR_MAX_SLICE;
  if (s > cdiv(m, 64)) s = cdiv(m, 64);
  return s < 1 ? 1 : s;
}

struct ProbeWs { size_t g, row_loss, row_hit, dbp, partial, total; };

inline ProbeWs probe_layout(int m, int d, int c) {
  const int s = probe_slices(m, d, c);
  ProbeWs o;
  o.g = 0;
  o.row_loss = (size_t)m * probe_cpad(c) * sizeof(float);
  o.row_hit = o.row_loss + (size_t)m * sizeof(float);
  o.dbp = align_up(o.row_hit + (size_t)m * sizeof(int32_t), 16);
  o.partial = o.dbp + align_up((size_t)s * c * sizeof(float), 16);
  o.total = o.partial + (s > 1 ? (size_t)s * c * d * sizeof(float) : 0);
  return o;
}

inline bool pr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int probe_vec(int d, const float* x, const float* w, const float* mean, const float* inv_std) {
  if ((d & 3) != 0) return 0;
  return (pr_aligned16(x) ? 1 : 0) | (w != nullptr && pr_aligned16(w) ? 2 : 0) | (pr_aligned16(mean) && pr_aligned16(inv_std) ? 4 : 0);
}

inline bool pr_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

constexpr int PR_MAX_HEADS = 32;

inline size_t probe_head_ws(int m, int d, int c) { return align_up(probe_layout(m, d, c).total, 16); }

// The launches of a step (grads) or a score over `heads` classifiers; the arguments have been checked.  head_stride: floats
// between consecutive heads of w / b / dw / db; ws_stride: floats between consecutive heads' workspaces (both unused with 1 head)
inline int probe_run(hipStream_t st, bool grads, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                     const float* inv_std, const float* w, const float* b, size_t head_stride, int heads, int m, int n, int d, int c,
                     float* loss, int32_t* hits, float* dw, float* db, void* ws) {
  const ProbeWs lay = probe_layout(m, d, c);
  const size_t ws_stride = align_up(lay.total, 16) / sizeof(float);
  char* base = reinterpret_cast<char*>(ws);
  float* g = reinterpret_cast<float*>(base + lay.g);
  float* row_loss = reinterpret_cast<float*>(base + lay.row_loss);
  int* row_hit = reinterpret_cast<int*>(base + lay.row_hit);
  float* dbp = reinterpret_cast<float*>(base + lay.dbp);
  float* partial = reinterpret_cast<float*>(base + lay.partial);
  const int cpad = probe_cpad(c);
  int vec = probe_vec(d, x, w, mean, inv_std);
  const size_t lds = (size_t)PR_TM * c * sizeof(float);
  if (!grads) {
    hipLaunchKernelGGL(probe_logits_kernel<PR_SCORE>, dim3(cdiv(m, PR_TM), heads), dim3(256), lds, st, x, rows, labels, mean, inv_std,
                       w, b, head_stride, ws_stride, m, n, d, c, cpad, vec, 1.f / (float)m, g, row_loss, row_hit, 0, nullptr, nullptr);
    CSTP_LAUNCH_CHECK();
    hipLaunchKernelGGL(probe_fold_kernel, dim3(1, heads), dim3(256), 0, st, partial, 1, (size_t)0, 0, (float*)nullptr, dbp, c,
                       (float*)nullptr, row_loss, row_hit, m, loss, hits, head_stride, ws_stride);
    CSTP_LAUNCH_CHECK();
    return 0;
  }
  const int rps = (int)align_up((size_t)cdiv(m, probe_slices(m, d, c)), PR_GR);
  const int ns = cdiv(m, rps);                                            // <= probe_slices: no slice is left without rows
  float* out = ns > 1 ? partial : dw;
  if ((d & 3) == 0 && pr_aligned16(out)) vec |= 8;                        // every head's out: both strides are multiples of 4 floats
  hipLaunchKernelGGL(probe_logits_kernel<PR_STEP>, dim3(cdiv(m, PR_TM), heads), dim3(256), lds, st, x, rows, labels, mean, inv_std, w,
                     b, head_stride, ws_stride, m, n, d, c, cpad, vec, 1.f / (float)m, g, row_loss, row_hit, 0, nullptr, nullptr);
  CSTP_LAUNCH_CHECK();
  hipLaunchKernelGGL(probe_wgrad_kernel, dim3(cdiv(d, PR_GT), cdiv(c, PR_GT), ns * heads), dim3(256), 0, st, x, rows, mean, inv_std, g,
                     m, n, d, c, cpad, vec, rps, ns, ws_stride, ns > 1 ? ws_stride : head_stride, out, dbp);
  CSTP_LAUNCH_CHECK();
  const size_t cd = (size_t)c * d;
  const int fold_blocks = ns > 1 ? (int)((cd + 255) / 256) : 0;
  hipLaunchKernelGGL(probe_fold_kernel, dim3(fold_blocks + 1, heads), dim3(256), 0, st, partial, ns, cd, fold_blocks, dw, dbp, c, db,
                     row_loss, row_hit, m, loss, hits, head_stride, ws_stride);
  CSTP_LAUNCH_CHECK();
  return 0;
}

// the checks the two sweep entry points share (dw == nullptr: score); 0 or the error code
inline int probe_sweep_check(const float* w, const float* b, int64_t head_stride, int heads, int m, int n, int d, int c,
                             const int32_t* rows, const float* dw, const float* db, const void* ws, size_t ws_bytes) {
  CSTP_REQUIRE(heads >= 1 && heads <= PR_MAX_HEADS, "heads must be in 1..32");
  CSTP_REQUIRE(c >= 2 && c <= PR_MAX_C, "c must be in 2..1024");
  CSTP_REQUIRE(probe_shape_ok(m, n, d, c), "bad shape");
  CSTP_REQUIRE(rows != nullptr || m <= n, "m must not exceed n without a row list");
  const int64_t wn = ((int64_t)c * d + 3) & ~(int64_t)3;
  CSTP_REQUIRE(head_stride > 0 && (head_stride & 3) == 0 && head_stride >= wn + c,
               "head stride must be a multiple of 4 floats and at least pad4(c d) + c");
  if (dw != nullptr) {
    const size_t wb = (size_t)c * d * sizeof(float), bb = (size_t)c * sizeof(float);
    for (int i = 0; i < heads; ++i)
      for (int j = 0; j < heads; ++j) {
        const float *dwi = dw + (size_t)i * head_stride, *dbi = db + (size_t)i * head_stride;
        const float *wj = w + (size_t)j * head_stride, *bj = b + (size_t)j * head_stride;
        CSTP_REQUIRE(!pr_overlap(dwi, wb, wj, wb) && !pr_overlap(dwi, wb, bj, bb) && !pr_overlap(dbi, bb, wj, wb) &&
                         !pr_overlap(dbi, bb, bj, bb), "dw / db must not alias w / b of any head");
      }
  }
  CSTP_REQUIRE(pr_aligned16(ws), "workspace must be 16-byte aligned");
  CSTP_REQUIRE(ws_bytes >= (size_t)heads * probe_head_ws(m, d, c), "workspace too small");
  return 0;
}

}  // namespace
}  // namespace cstp

extern "C" size_t cstp_probe_workspace_bytes(int32_t m, int32_t d, int32_t c) {
  if (!cstp::probe_shape_ok(m, 1, d, c)) return 0;
  return cstp::probe_layout(m, d, c).total;
}

extern "C" size_t cstp_probe_sweep_workspace_bytes(int32_t heads, int32_t m, int32_t d, int32_t c) {
  if (heads < 1 || heads > cstp::PR_MAX_HEADS || !cstp::probe_shape_ok(m, 1, d, c)) return 0;
  return (size_t)heads * cstp::probe_head_ws(m, d, c);
}

extern "C" int cstp_probe_step(void* stream, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                               const float* inv_std, const float* w, const float* b, int32_t m, int32_t n, int32_t d, int32_t c,
                               float* loss, int32_t* hits, float* dw, float* db, void* ws, size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && labels != nullptr && w != nullptr && b != nullptr && loss != nullptr && hits != nullptr &&
                   dw != nullptr && db != nullptr && ws != nullptr, "null argument");
  CSTP_REQUIRE(c >= 2 && c <= PR_MAX_C, "c must be in 2..1024");
  CSTP_REQUIRE(probe_shape_ok(m, n, d, c), "bad shape");
  CSTP_REQUIRE(rows != nullptr || m <= n, "m must not exceed n without a row list");
  const size_t wb = (size_t)c * d * sizeof(float), bb = (size_t)c * sizeof(float);
  CSTP_REQUIRE(!pr_overlap(dw, wb, w, wb) && !pr_overlap(dw, wb, b, bb) && !pr_overlap(db, bb, w, wb) && !pr_overlap(db, bb, b, bb),
               "dw / db must not alias w / b");
  CSTP_REQUIRE(pr_aligned16(ws), "workspace must be 16-byte aligned");
  CSTP_REQUIRE(ws_bytes >= probe_layout(m, d, c).total, "workspace too small");
  return probe_run(as_stream(stream), true, x, rows, labels, mean, inv_std, w, b, 0, 1, m, n, d, c, loss, hits, dw, db, ws);
}

extern "C" int cstp_probe_sweep_step(void* stream, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                                     const float* inv_std, const float* w, const float* b, int64_t head_stride, int32_t heads,
                                     int32_t m, int32_t n, int32_t d, int32_t c, float* loss, int32_t* hits, float* dw, float* db,
                                     void* ws, size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && labels != nullptr && w != nullptr && b != nullptr && loss != nullptr && hits != nullptr &&
                   dw != nullptr && db != nullptr && ws != nullptr, "null argument");
  if (const int rc = probe_sweep_check(w, b, head_stride, heads, m, n, d, c, rows, dw, db, ws, ws_bytes)) return rc;
  return probe_run(as_stream(stream), true, x, rows, labels, mean, inv_std, w, b, (size_t)head_stride, heads, m, n, d, c, loss, hits,
                   dw, db, ws);
}

extern "C" int cstp_probe_sweep_score(void* stream, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                                      const float* inv_std, const float* w, const float* b, int64_t head_stride, int32_t heads,
                                      int32_t m, int32_t n, int32_t d, int32_t c, float* loss, int32_t* hits, void* ws,
                                      size_t ws_bytes) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && labels != nullptr && w != nullptr && b != nullptr && loss != nullptr && hits != nullptr &&
                   ws != nullptr, "null argument");
  if (const int rc = probe_sweep_check(w, b, head_stride, heads, m, n, d, c, rows, nullptr, nullptr, ws, ws_bytes)) return rc;
  return probe_run(as_stream(stream), false, x, rows, labels, mean, inv_std, w, b, (size_t)head_stride, heads, m, n, d, c, loss, hits,
                   nullptr, nullptr, ws);
}

extern "C" int cstp_probe_predict(void* stream, const float* x, const float* mean, const float* inv_std, const float* w,
                                  const float* b, int32_t n, int32_t d, int32_t c, int32_t n_top, int32_t* pred, float* score) {
  using namespace cstp;
  CSTP_REQUIRE(x != nullptr && w != nullptr && b != nullptr && pred != nullptr && score != nullptr, "null argument");
  CSTP_REQUIRE(c >= 2 && c <= PR_MAX_C, "c must be in 2..1024");
  CSTP_REQUIRE(n_top >= 1 && n_top <= PR_MAX_TOP, "n_top must be in 1..8");
  CSTP_REQUIRE(probe_shape_ok(n, n, d, c), "bad shape");
  const int vec = probe_vec(d, x, w, mean, inv_std);
  hipLaunchKernelGGL(probe_logits_kernel<PR_PREDICT>, dim3(cdiv(n, PR_TM)), dim3(256), (size_t)PR_TM * c * sizeof(float),
                     as_stream(stream), x, nullptr, nullptr, mean, inv_std, w, b, (size_t)0, (size_t)0, n, n, d, c, probe_cpad(c), vec,
                     0.f, nullptr, nullptr, nullptr, n_top, pred, score);
  CSTP_LAUNCH_CHECK();
  return 0;
}
