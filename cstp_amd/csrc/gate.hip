// S3D-G self-gating fused with the inception concat (models/coclr/s3dg.py:100-110, :150-163), forward and backward.
//
// One SepInception block has up to four branches; branch i's output x_i [n][c_i][s] is gated by
//   g_i[n][c] = sigmoid(b_i[c] + sum_k W_i[c][k] * mean_s x_i[n][k][s])
// and written, multiplied by its gate, straight into channels [o_i, o_i + c_i) of the concat tensor y [n][C][s]: the four
// SelfGating modules and torch.cat become two launches (means; gate + apply), their backward three (row dot products;
// parameter gradients and the gradient of the means; input gradients).  Rows are short (s = 18 .. 1568) and there are many
// of them, so one wave owns one (sample, channel) row; every reduction is a fixed-order wave shuffle or a fixed-order loop
// (no float atomics): two calls with the same inputs are bit-identical.  The only atomic is the integer max that folds
// each apply block's max |y| into the caller's cell (max is order-independent).
#include "common.h"

namespace cstp {
namespace {

struct GateSet {
  cstp_gate_branch br[CSTP_GATE_MAX_BRANCHES];
  int off[CSTP_GATE_MAX_BRANCHES + 1];   // channel offsets in the concat tensor; off[nb] = C
  int pe[CSTP_GATE_MAX_BRANCHES + 1];    // offsets of each branch's (dW | db) elements: c_i * (c_i + 1) per branch
  int nb;
};

__device__ __forceinline__ int gate_branch(const GateSet& gs, int ch) {
  int i = 0;
#pragma unroll
  for (int j = 1; j < CSTP_GATE_MAX_BRANCHES; ++j)
    if (j < gs.nb && ch >= gs.off[j]) i = j;
  return i;
}

__device__ __forceinline__ unsigned gate_umax(unsigned a, unsigned b) { return a > b ? a : b; }

constexpr int GATE_WAVES = 4;              // waves (rows in flight) per 256-thread block
constexpr int GATE_APPLY_MAX_BLOCKS = 1024;  // caps the apply grid, and with it the absmax atomics per call

// ---- forward 1: m[n][C] = row means; block 0 zeroes the absmax cell the apply launch folds into ---------------------------
template <bool VEC4>
__global__ void __launch_bounds__(256) gate_mean_kernel(GateSet gs, int rows, int ctot, int s, float* __restrict__ m,
                                                         unsigned* __restrict__ cell) {
  if (cell != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *cell = 0;
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * GATE_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int ns = r / ctot, ch = r - ns * ctot;
  const int i = gate_branch(gs, ch);
  const int c = gs.br[i].c, k = ch - gs.off[i];
  const float* x = gs.br[i].x + ((size_t)ns * c + k) * s;
  float acc = 0.f;
  if (VEC4) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (int j = lane; j < (s >> 2); j += 64) {
      const float4 v = x4[j];
      acc += (v.x + v.y) + (v.z + v.w);
    }
  } else if ((s & 3) == 0) {      // rows off a 16-byte boundary: the float4 body's order of additions, so the bits do not depend on alignment
    for (int j = lane; j < (s >> 2); j += 64) {
      const float* v = x + 4 * j;
      acc += (v[0] + v[1]) + (v[2] + v[3]);
    }
  } else {
    for (int j = lane; j < s; j += 64) acc += x[j];
  }
  acc = wave_sum_all(acc);
  if (lane == 0) m[r] = acc / (float)s;
}

// ---- forward 2: gate (one dot product of length c_i per row) and y = g * x into the concat tensor ------------------------
template <bool VEC4>
__global__ void __launch_bounds__(256) gate_apply_kernel(GateSet gs, int rows, int ctot, int s, const float* __restrict__ m,
                                                          float* __restrict__ g, float* __restrict__ y,
                                                          unsigned* __restrict__ cell) {
  __shared__ unsigned red[GATE_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned mx = 0;
  for (int r = blockIdx.x * GATE_WAVES + wave; r < rows; r += gridDim.x * GATE_WAVES) {
    const int ns = r / ctot, ch = r - ns * ctot;
    const int i = gate_branch(gs, ch);
    const int c = gs.br[i].c, k = ch - gs.off[i];
    const float* wrow = gs.br[i].w + (size_t)k * c;
    const float* mrow = m + (size_t)ns * ctot + gs.off[i];
    float z = 0.f;
    for (int j = lane; j < c; j += 64) z = __builtin_fmaf(wrow[j], mrow[j], z);
    z = wave_sum_all(z) + gs.br[i].b[k];
    const float gv = 1.f / (1.f + expf(-z));
    if (g != nullptr && lane == 0) g[r] = gv;
    const float* x = gs.br[i].x + ((size_t)ns * c + k) * s;
    float* yr = y + (size_t)r * s;
    if (VEC4) {
      const float4* x4 = reinterpret_cast<const float4*>(x);
      float4* y4 = reinterpret_cast<float4*>(yr);
      for (int j = lane; j < (s >> 2); j += 64) {
        const float4 v = x4[j];
        const float4 o = make_float4(gv * v.x, gv * v.y, gv * v.z, gv * v.w);
        y4[j] = o;
        mx = gate_umax(mx, gate_umax(gate_umax(abs_bits(o.x), abs_bits(o.y)),
                                     gate_umax(abs_bits(o.z), abs_bits(o.w))));
      }
    } else {
      for (int j = lane; j < s; j += 64) {
        const float o = gv * x[j];
        yr[j] = o;
        mx = gate_umax(mx, abs_bits(o));
      }
    }
  }
  if (cell == nullptr) return;        // grid-uniform
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = gate_umax(mx, (unsigned)__shfl_xor((int)mx, o, 64));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned a = gate_umax(gate_umax(red[0], red[1]), gate_umax(red[2], red[3]));
    if (a != 0) atomicMax(cell, a);
  }
}

// ---- backward 1: d[n][C] = (sum_s dy * x) * g * (1 - g) -------------------------------------------------------------------
template <bool VEC4>
__global__ void __launch_bounds__(256) gate_dot_kernel(GateSet gs, int rows, int ctot, int s, const float* __restrict__ dy,
                                                        const float* __restrict__ g, float* __restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * GATE_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int ns = r / ctot, ch = r - ns * ctot;
  const int i = gate_branch(gs, ch);
  const int c = gs.br[i].c, k = ch - gs.off[i];
  const float* x = gs.br[i].x + ((size_t)ns * c + k) * s;
  const float* dyr = dy + (size_t)r * s;
  float t = 0.f;
  if (VEC4) {
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* d4 = reinterpret_cast<const float4*>(dyr);
    for (int j = lane; j < (s >> 2); j += 64) {
      const float4 a = x4[j], b = d4[j];
      t = __builtin_fmaf(a.x, b.x, t);
      t = __builtin_fmaf(a.y, b.y, t);
      t = __builtin_fmaf(a.z, b.z, t);
      t = __builtin_fmaf(a.w, b.w, t);
    }
  } else if ((s & 3) == 0) {      // ... and here the float4 body's chain of four per lane
    for (int j = lane; j < (s >> 2); j += 64) {
      const float* a = x + 4 * j;
      const float* b = dyr + 4 * j;
      t = __builtin_fmaf(a[0], b[0], t);
      t = __builtin_fmaf(a[1], b[1], t);
      t = __builtin_fmaf(a[2], b[2], t);
      t = __builtin_fmaf(a[3], b[3], t);
    }
  } else {
    for (int j = lane; j < s; j += 64) t = __builtin_fmaf(x[j], dyr[j], t);
  }
  t = wave_sum_all(t);
  if (lane == 0) {
    const float gv = g[r];
    d[r] = t * gv * (1.f - gv);
  }
}

// ---- backward 2: blocks [0, nwb) one thread per (dW | db) element (sum over the batch), the rest one thread per dm element
//      (sum over the branch's gate channels, W read down a column: consecutive threads, consecutive k) -------------------------
__global__ void __launch_bounds__(256) gate_param_kernel(GateSet gs, int n, int ctot, const float* __restrict__ m,
                                                          const float* __restrict__ d, float* __restrict__ dm, int nwb,
                                                          int accumulate) {
  if ((int)blockIdx.x < nwb) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= gs.pe[gs.nb]) return;
    int i = 0;
#pragma unroll
    for (int j = 1; j < CSTP_GATE_MAX_BRANCHES; ++j)
      if (j < gs.nb && e >= gs.pe[j]) i = j;
    const int c = gs.br[i].c, o = gs.off[i];
    const int loc = e - gs.pe[i];
    const int cc = loc / (c + 1), kk = loc - cc * (c + 1);
    float acc = 0.f;
    if (kk < c) {
      for (int ns = 0; ns < n; ++ns) acc = __builtin_fmaf(d[(size_t)ns * ctot + o + cc], m[(size_t)ns * ctot + o + kk], acc);
      float* dst = gs.br[i].dw + (size_t)cc * c + kk;
      *dst = accumulate ? *dst + acc : acc;
    } else {
      for (int ns = 0; ns < n; ++ns) acc += d[(size_t)ns * ctot + o + cc];
      float* dst = gs.br[i].db + cc;
      *dst = accumulate ? *dst + acc : acc;
    }
    return;
  }
  const int e = (blockIdx.x - nwb) * 256 + threadIdx.x;
  if (e >= n * ctot) return;
  const int ns = e / ctot, ch = e - ns * ctot;
  const int i = gate_branch(gs, ch);
  const int c = gs.br[i].c, k = ch - gs.off[i];
  const float* w = gs.br[i].w + k;
  const float* dr = d + (size_t)ns * ctot + gs.off[i];
  float acc = 0.f;
  for (int cc = 0; cc < c; ++cc) acc = __builtin_fmaf(w[(size_t)cc * c], dr[cc], acc);
  dm[e] = acc;
}

// ---- backward 3: dx_i = g * dy + dm / s -----------------------------------------------------------------------------------
template <bool VEC4>
__global__ void __launch_bounds__(256) gate_dx_kernel(GateSet gs, int rows, int ctot, int s, const float* __restrict__ dy,
                                                       const float* __restrict__ g, const float* __restrict__ dm) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * GATE_WAVES + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int ns = r / ctot, ch = r - ns * ctot;
  const int i = gate_branch(gs, ch);
  const int c = gs.br[i].c, k = ch - gs.off[i];
  float* dx = gs.br[i].dx + ((size_t)ns * c + k) * s;
  const float* dyr = dy + (size_t)r * s;
  const float gv = g[r], add = dm[r] / (float)s;
  if (VEC4) {
    const float4* d4 = reinterpret_cast<const float4*>(dyr);
    float4* o4 = reinterpret_cast<float4*>(dx);
    for (int j = lane; j < (s >> 2); j += 64) {
      const float4 v = d4[j];
      o4[j] = make_float4(__builtin_fmaf(gv, v.x, add), __builtin_fmaf(gv, v.y, add), __builtin_fmaf(gv, v.z, add),
                          __builtin_fmaf(gv, v.w, add));
    }
  } else {
    for (int j = lane; j < s; j += 64) dx[j] = __builtin_fmaf(gv, dyr[j], add);
  }
}


// validates the branch table and fills the kernel-argument set; vec4: every row starts on a 16-byte boundary
int make_set(const cstp_gate_branch* br, int nb, int n, int s, bool bwd, GateSet* gs, bool* vec4) {
  CSTP_REQUIRE(br != nullptr && nb >= 1 && nb <= CSTP_GATE_MAX_BRANCHES, "bad branch table");
  CSTP_REQUIRE(n > 0 && s > 0, "bad shape");
  memset(gs, 0, sizeof(*gs));
  gs->nb = nb;
  bool v = (s & 3) == 0;
  long ctot = 0, pe = 0;
  for (int i = 0; i < nb; ++i) {
    const cstp_gate_branch& b = br[i];
    CSTP_REQUIRE(b.x != nullptr && b.w != nullptr && b.b != nullptr && b.c > 0, "null argument");
    if (bwd) CSTP_REQUIRE(b.dx != nullptr && b.dw != nullptr && b.db != nullptr, "null argument");
    v = v && al16(b.x) && (!bwd || al16(b.dx));
    gs->br[i] = b;
    gs->off[i] = (int)ctot;
    gs->pe[i] = (int)pe;
    ctot += b.c;
    pe += (long)b.c * (b.c + 1);
  }
  CSTP_REQUIRE(ctot * n < (1L << 31) && pe < (1L << 31) && ctot * n * (long)s < (1L << 40), "tensor too large");
  for (int i = nb; i <= CSTP_GATE_MAX_BRANCHES; ++i) {
    gs->off[i] = (int)ctot;
    gs->pe[i] = (int)pe;
  }
  *vec4 = v;
  return 0;
}

}  // namespace
}  // namespace cstp

using namespace cstp;

extern "C" size_t cstp_gate_workspace_bytes(int32_t n, int32_t ctot) {
  if (n <= 0 || ctot <= 0) return 0;
  return align_up((size_t)n * ctot * sizeof(float), 256) * 2;    // d [n][C] | dm [n][C]
}

extern "C" int cstp_gate_concat_forward(void* stream, const cstp_gate_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                                        float* y, float* m, float* g, uint32_t* y_absmax) {
  GateSet gs;
  bool v4 = false;
  if (make_set(branches, nbranch, n, s, false, &gs, &v4)) return 1;
  CSTP_REQUIRE(y != nullptr && m != nullptr, "null argument");
  v4 = v4 && al16(y);
  const int ctot = gs.off[gs.nb], rows = n * ctot;
  hipStream_t st = as_stream(stream);
  const dim3 grid1(cdiv(rows, GATE_WAVES));
  if (v4) hipLaunchKernelGGL(gate_mean_kernel<true>, grid1, dim3(256), 0, st, gs, rows, ctot, s, m, y_absmax);
  else hipLaunchKernelGGL(gate_mean_kernel<false>, grid1, dim3(256), 0, st, gs, rows, ctot, s, m, y_absmax);
  CSTP_LAUNCH_CHECK();
  const dim3 grid2(cdiv(rows, GATE_WAVES) < GATE_APPLY_MAX_BLOCKS ? cdiv(rows, GATE_WAVES) : GATE_APPLY_MAX_BLOCKS);
  if (v4) hipLaunchKernelGGL(gate_apply_kernel<true>, grid2, dim3(256), 0, st, gs, rows, ctot, s, m, g, y, y_absmax);
  else hipLaunchKernelGGL(gate_apply_kernel<false>, grid2, dim3(256), 0, st, gs, rows, ctot, s, m, g, y, y_absmax);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_gate_concat_backward(void* stream, const cstp_gate_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                                         const float* dy, const float* m, const float* g, void* ws, size_t ws_bytes,
                                         int32_t accumulate) {
  GateSet gs;
  bool v4 = false;
  if (make_set(branches, nbranch, n, s, true, &gs, &v4)) return 1;
  CSTP_REQUIRE(dy != nullptr && m != nullptr && g != nullptr && ws != nullptr, "null argument");
  v4 = v4 && al16(dy);
  const int ctot = gs.off[gs.nb], rows = n * ctot;
  CSTP_REQUIRE(ws_bytes >= cstp_gate_workspace_bytes(n, ctot), "workspace too small");
  float* d = reinterpret_cast<float*>(ws);
  float* dm = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + align_up((size_t)rows * sizeof(float), 256));
  hipStream_t st = as_stream(stream);
  const dim3 grid(cdiv(rows, GATE_WAVES));
  if (v4) hipLaunchKernelGGL(gate_dot_kernel<true>, grid, dim3(256), 0, st, gs, rows, ctot, s, dy, g, d);
  else hipLaunchKernelGGL(gate_dot_kernel<false>, grid, dim3(256), 0, st, gs, rows, ctot, s, dy, g, d);
  CSTP_LAUNCH_CHECK();
  const int nwb = cdiv(gs.pe[gs.nb], 256);
  hipLaunchKernelGGL(gate_param_kernel, dim3(nwb + cdiv(rows, 256)), dim3(256), 0, st, gs, n, ctot, m, d, dm, nwb,
                     accumulate ? 1 : 0);
  CSTP_LAUNCH_CHECK();
  if (v4) hipLaunchKernelGGL(gate_dx_kernel<true>, grid, dim3(256), 0, st, gs, rows, ctot, s, dy, g, dm);
  else hipLaunchKernelGGL(gate_dx_kernel<false>, grid, dim3(256), 0, st, gs, rows, ctot, s, dy, g, dm);
  CSTP_LAUNCH_CHECK();
  return 0;
}
