// RandAugment and random erasing on a BATCH of 8-bit clips (cstp_randaug_layer, cstp_randaug_finish; spec in include/cstp_hip.h,
// DESIGN.md section 23).  Included from clip.hip behind the kernels whose arithmetic it reuses (luma8, blend8, clip_grid).
//
// One LAYER = one operation per clip, read from a device table with one entry per clip: blockIdx.y picks the clip and its entry,
// so the operation is uniform over a block and the switch on it is a scalar branch.  A layer is at most two launches whatever the
// batch size:
//   statistics  only when some clip's operation is AutoContrast, Equalize or Contrast (the host copy of the table decides): one
//               block per (frame, clip); blocks of other clips return at once.  Contrast takes the frame's luma sum as
//               clip_luma_mean_kernel does (integer, order-free).  AutoContrast / Equalize build three 256-bin histograms in LDS
//               with integer atomics (order-free as well) and then the three look-up tables of ImageOps.autocontrast /
//               ImageOps.equalize: thread j owns table entry j and walks the 256 bins itself -- every lane of a wave reads the
//               same LDS word, a broadcast -- which yields the first / last non-empty bin, the non-empty count and the exclusive
//               prefix without a reduction or a scan to get wrong; 768 LDS reads per thread are noise next to the histogram.
//   apply       every clip, src -> dst.  Pointwise operations (copy, table look-up, Posterize, Solarize, the blends against black /
//               the frame's mean luma / the pixel's luma) move 16 pixels = 48 bytes = three 16-byte loads and stores per thread when
//               the clip's pixel count is a multiple of 16 and both buffers are 16-byte aligned, one pixel per thread otherwise.
//               Sharpness (blend against the 3x3 smooth of the SOURCE buffer), the fixed-point affine with fill and the integer shift
//               with fill gather one pixel per thread.
// The FINISH is cstp_clip_finish for the whole batch in one launch -- flip, ToTensor, 'tf' normalisation into out[out_slot] -- with
// the erased box filled on the way out from Philox4x32-10 (philox.h), counter layout of cstp_dropout: element e of the clip's fp32
// tensor takes word e & 3 of Philox((e >> 2), 0; key).
// Every entry is checked on the host copy before a launch and again where it is used: an unknown operation is served as a copy, a
// bad output slot writes nothing, a box that leaves the frame erases nothing; gathers test their source coordinates.
#pragma once
#include "common.h"
#include "philox.h"

namespace cstp {

enum : int {
  RA_COPY = 0, RA_AUTOCONTRAST = 1, RA_EQUALIZE = 2, RA_POSTERIZE = 3, RA_SOLARIZE = 4, RA_BRIGHTNESS = 5, RA_CONTRAST = 6,
  RA_COLOR = 7,                                   // ... up to here: pointwise
  RA_SHARPNESS = 8, RA_AFFINE = 9, RA_SHIFT = 10, RA_OPS = 11
};
constexpr int RA_FILL = 128;                      // the fill colour (128, 128, 128): ~0 after the 'tf' normalisation

__device__ __forceinline__ bool ra_needs_lut(int op) { return op == RA_AUTOCONTRAST || op == RA_EQUALIZE; }
__device__ __forceinline__ double rounded64(double x) { asm volatile("" : "+v"(x)); return x; }

// ImageOps.autocontrast's table entry: int(ix * scale + offset) clipped, in double, the product rounded before the sum
__device__ __forceinline__ int ra_autocontrast_entry(int ix, int lo, int hi) {
#pragma clang fp contract(off)
  const double scale = __ddiv_rn(255.0, (double)(hi - lo));
  const double offset = rounded64(__dmul_rn((double)(-lo), scale));
  const int v = (int)__dadd_rn(rounded64(__dmul_rn((double)ix, scale)), offset);
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ void __launch_bounds__(256) randaug_stats_kernel(const uint8_t* __restrict__ src,
                                                            const cstp_randaug_entry* __restrict__ table,
                                                            uint8_t* __restrict__ lut, int32_t* __restrict__ mean, int T, int HW) {
  __shared__ unsigned hist[3][256];
  __shared__ unsigned long long red[4];
  const int clip = blockIdx.y, frame = blockIdx.x;
  const int op = table[clip].op;
  if (!ra_needs_lut(op) && op != RA_CONTRAST) return;                 // uniform over the block
  const size_t fr = (size_t)clip * T + frame;
  const uint8_t* p = src + fr * HW * 3;
  if (op == RA_CONTRAST) {                                             // clip_luma_mean_kernel's arithmetic
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < HW; i += 256) acc += (unsigned long long)luma8(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) mean[fr] = (int32_t)((double)(red[0] + red[1] + red[2] + red[3]) / (double)HW + 0.5);
    return;
  }
  const int j = threadIdx.x;
  hist[0][j] = 0; hist[1][j] = 0; hist[2][j] = 0;
  __syncthreads();
  for (int i = j; i < HW; i += 256) {
    atomicAdd(&hist[0][p[3 * i]], 1u);
    atomicAdd(&hist[1][p[3 * i + 1]], 1u);
    atomicAdd(&hist[2][p[3 * i + 2]], 1u);
  }
  __syncthreads();
  uint8_t* out = lut + fr * 768;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    unsigned prefix = 0, total = 0, last_count = 0;
    int lo = 256, hi = -1, filled = 0;
    for (int i = 0; i < 256; ++i) {
      const unsigned v = hist[c][i];                                   // the same word in every lane: an LDS broadcast
      if (i < j) prefix += v;
      total += v;
      if (v != 0) { lo = lo == 256 ? i : lo; hi = i; last_count = v; ++filled; }
    }
    int e = j;                                                         // the identity table
    if (op == RA_AUTOCONTRAST) {
      if (hi > lo) e = ra_autocontrast_entry(j, lo, hi);
    } else {
      const unsigned step = (total - last_count) / 255u;
      if (filled > 1 && step != 0) {
        const unsigned v = (step / 2u + prefix) / step;
        e = v > 255u ? 255 : (int)v;                                   // Image.point clips its table to 8 bits
      }
    }
    out[c * 256 + j] = (uint8_t)e;
  }
}

// what one pixel becomes under a pointwise operation; lutf / mean belong to the pixel's frame
__device__ __forceinline__ void ra_point(int op, const cstp_randaug_entry& e, bool inside, const uint8_t* __restrict__ lutf, int mean,
                                         int r, int g, int b, int& o0, int& o1, int& o2) {
  switch (op) {
    case RA_AUTOCONTRAST:
    case RA_EQUALIZE: o0 = lutf[r]; o1 = lutf[256 + g]; o2 = lutf[512 + b]; break;
    case RA_POSTERIZE: o0 = r & e.a[0]; o1 = g & e.a[0]; o2 = b & e.a[0]; break;
    case RA_SOLARIZE: o0 = r < e.a[0] ? r : 255 - r; o1 = g < e.a[0] ? g : 255 - g; o2 = b < e.a[0] ? b : 255 - b; break;
    case RA_BRIGHTNESS: o0 = blend8(0, r, e.factor, inside); o1 = blend8(0, g, e.factor, inside); o2 = blend8(0, b, e.factor, inside); break;
    case RA_CONTRAST: o0 = blend8(mean, r, e.factor, inside); o1 = blend8(mean, g, e.factor, inside); o2 = blend8(mean, b, e.factor, inside); break;
    case RA_COLOR: {
      const int l = luma8(r, g, b);
      o0 = blend8(l, r, e.factor, inside); o1 = blend8(l, g, e.factor, inside); o2 = blend8(l, b, e.factor, inside);
      break;
    }
    default: o0 = r; o1 = g; o2 = b; break;
  }
}

// ImageFilter.SMOOTH at an inner pixel: (2 * sum + 13) / 26 with the weights (1 1 1 / 1 5 1 / 1 1 1); c = channel
__device__ __forceinline__ int ra_smooth(const uint8_t* __restrict__ p, int row, int c) {
  const uint8_t* u = p - row;
  const uint8_t* d = p + row;
  const int s = u[c - 3] + u[c] + u[c + 3] + p[c - 3] + 5 * p[c] + p[c + 3] + d[c - 3] + d[c] + d[c + 3];
  return (2 * s + 13) / 26;
}

__global__ void __launch_bounds__(256) randaug_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                            const cstp_randaug_entry* __restrict__ table,
                                                            const uint8_t* __restrict__ lut, const int32_t* __restrict__ mean, int T,
                                                            int S, int vec) {
  const int clip = blockIdx.y;
  const cstp_randaug_entry e = table[clip];
  const int op = e.op >= 0 && e.op < RA_OPS ? e.op : RA_COPY;
  const int HW = S * S, npix = T * HW;
  const uint8_t* __restrict__ sp = src + (size_t)clip * npix * 3;
  uint8_t* __restrict__ dp = dst + (size_t)clip * npix * 3;
  const uint8_t* __restrict__ lutc = ra_needs_lut(op) ? lut + (size_t)clip * T * 768 : nullptr;
  const int32_t* __restrict__ meanc = op == RA_CONTRAST ? mean + (size_t)clip * T : nullptr;
  const bool inside = e.factor >= 0.0f && e.factor <= 1.0f;
  const int start = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;

  if (op <= RA_COLOR && vec) {                                         // 16 pixels = 48 bytes per thread
    const int groups = npix >> 4;
    for (int gi = start; gi < groups; gi += stride) {
      const uint4* s4 = reinterpret_cast<const uint4*>(sp) + (size_t)gi * 3;
      const uint4 v0 = s4[0], v1 = s4[1], v2 = s4[2];
      const uint32_t w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
      uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      int f = (gi << 4) / HW, rem = (gi << 4) - f * HW;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int j = 3 * k;
        const int r = (w[j >> 2] >> (8 * (j & 3))) & 255, g = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255,
                  b = (w[(j + 2) >> 2] >> (8 * ((j + 2) & 3))) & 255;
        int o0, o1, o2;
        ra_point(op, e, inside, lutc ? lutc + (size_t)f * 768 : nullptr, meanc ? meanc[f] : 0, r, g, b, o0, o1, o2);
        o[j >> 2] |= (uint32_t)(o0 & 255) << (8 * (j & 3));
        o[(j + 1) >> 2] |= (uint32_t)(o1 & 255) << (8 * ((j + 1) & 3));
        o[(j + 2) >> 2] |= (uint32_t)(o2 & 255) << (8 * ((j + 2) & 3));
        if (++rem == HW) { rem = 0; ++f; }
      }
      uint4* d4 = reinterpret_cast<uint4*>(dp) + (size_t)gi * 3;
      d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
      d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
      d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
    return;
  }
  for (int i = start; i < npix; i += stride) {
    const uint8_t* p = sp + (size_t)i * 3;
    uint8_t* o = dp + (size_t)i * 3;
    int o0, o1, o2;
    if (op <= RA_COLOR) {
      const int f = i / HW;
      ra_point(op, e, inside, lutc ? lutc + (size_t)f * 768 : nullptr, meanc ? meanc[f] : 0, p[0], p[1], p[2], o0, o1, o2);
    } else {
      const int x = i % S, rr = i / S;
      const int y = rr % S, t = rr / S;
      if (op == RA_SHARPNESS) {
        const int r = p[0], g = p[1], b = p[2];
        int d0 = r, d1 = g, d2 = b;                                    // border rows and columns of the filter are copied
        if (x > 0 && y > 0 && x < S - 1 && y < S - 1) { d0 = ra_smooth(p, S * 3, 0); d1 = ra_smooth(p, S * 3, 1); d2 = ra_smooth(p, S * 3, 2); }
        o0 = blend8(d0, r, e.factor, inside); o1 = blend8(d1, g, e.factor, inside); o2 = blend8(d2, b, e.factor, inside);
      } else {
        int xin, yin;
        if (op == RA_AFFINE) {                                         // Geometry.c affine_fixed, 16.16 fixed point
          xin = (e.a[2] + e.a[1] * y + e.a[0] * x) >> 16;
          yin = (e.a[5] + e.a[4] * y + e.a[3] * x) >> 16;
        } else {                                                       // RA_SHIFT
          xin = x + e.a[0];
          yin = y + e.a[1];
        }
        o0 = o1 = o2 = RA_FILL;
        if (xin >= 0 && xin < S && yin >= 0 && yin < S) {
          const uint8_t* q = sp + (((size_t)t * S + yin) * S + xin) * 3;
          o0 = q[0]; o1 = q[1]; o2 = q[2];
        }
      }
    }
    o[0] = (uint8_t)o0; o[1] = (uint8_t)o1; o[2] = (uint8_t)o2;
  }
}

__global__ void __launch_bounds__(256) randaug_finish_kernel(const uint8_t* __restrict__ src, float* __restrict__ out,
                                                             const cstp_randaug_finish_entry* __restrict__ table, int T, int S,
                                                             int out_slots) {
  const int clip = blockIdx.y;
  const cstp_randaug_finish_entry e = table[clip];
  if (e.out_slot < 0 || e.out_slot >= out_slots) return;
  const bool erase = e.w > 0 && e.h > 0 && e.x0 >= 0 && e.y0 >= 0 && e.x0 <= S - e.w && e.y0 <= S - e.h;
  const int npix = T * S * S;
  const size_t plane = (size_t)npix;
  const uint8_t* __restrict__ sp = src + (size_t)clip * npix * 3;
  float* __restrict__ op = out + (size_t)e.out_slot * 3 * plane;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += gridDim.x * 256) {
    const int x = i % S, y = (i / S) % S;
    const int xo = e.flip ? S - 1 - x : x;
    const size_t o = (size_t)(i - x + xo);
    const uint8_t* p = sp + (size_t)i * 3;
    const bool boxed = erase && xo >= e.x0 && xo < e.x0 + e.w && y >= e.y0 && y < e.y0 + e.h;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t el = c * plane + o;
      float v;
      if (boxed) {
        const uint64_t q = (uint64_t)el >> 2;
        const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u, e.key_lo, e.key_hi);
        const int k = (int)(el & 3);
        const uint32_t wd = k == 0 ? r.v[0] : (k == 1 ? r.v[1] : (k == 2 ? r.v[2] : r.v[3]));
        v = (float)(wd >> 8) * 1.1920928955078125e-7f - 1.0f;          // 2^-23: exact, in [-1, 1)
      } else {
        v = (float)p[c] / 255.0f;                                      // transforms.ToTensor()
        v = v * 2.0f - 1.0f;                                           // ClipNormalize('tf')
        v = fminf(fmaxf(v, -1.0f), 1.0f);
      }
      op[el] = v;
    }
  }
}

inline bool ra_shape_ok(int32_t b, int32_t t, int32_t s) {
  return b > 0 && b <= 65535 && t > 0 && s > 0 && s <= 4096 && (int64_t)t * s * s * 3 <= INT32_MAX;
}

}  // namespace cstp

extern "C" size_t cstp_randaug_entry_bytes(void) { return sizeof(cstp_randaug_entry); }

extern "C" int cstp_randaug_layer(void* stream, const uint8_t* src, uint8_t* dst, const cstp_randaug_entry* table_dev,
                                  const cstp_randaug_entry* table_host, int32_t b, int32_t t, int32_t s, uint8_t* lut,
                                  int32_t* mean) {
  using namespace cstp;
  static_assert(sizeof(cstp_randaug_entry) == 32, "cstp_randaug_entry is packed by the host as 32 bytes");
  CSTP_REQUIRE(src && dst && table_dev && table_host && src != dst, "null or aliased argument");
  CSTP_REQUIRE(ra_shape_ok(b, t, s), "bad shape");
  bool stats = false;
  for (int i = 0; i < b; ++i) {          // the device copy may still be in flight: the host copy is what is checked
    const cstp_randaug_entry& e = table_host[i];
    CSTP_REQUIRE(e.op >= 0 && e.op < RA_OPS, "unknown operation in a table entry");
    CSTP_REQUIRE(e.factor == e.factor && e.factor >= -16.0f && e.factor <= 16.0f, "blend factor of a table entry out of range");
    if (e.op == RA_POSTERIZE) CSTP_REQUIRE(e.a[0] >= 0 && e.a[0] <= 255, "posterize mask of a table entry");
    if (e.op == RA_SOLARIZE) CSTP_REQUIRE(e.a[0] >= 0 && e.a[0] <= 256, "solarize threshold of a table entry");
    if (e.op == RA_SHIFT) CSTP_REQUIRE(e.a[0] >= -65536 && e.a[0] <= 65536 && e.a[1] >= -65536 && e.a[1] <= 65536, "shift of a table entry");
    if (e.op == RA_AFFINE) {             // s <= 4096: three terms below 2^29 each, the sum stays in 32 bits
      const int lim = 2 << 16, off = 1 << 29;
      CSTP_REQUIRE(e.a[0] >= -lim && e.a[0] <= lim && e.a[1] >= -lim && e.a[1] <= lim && e.a[3] >= -lim && e.a[3] <= lim &&
                   e.a[4] >= -lim && e.a[4] <= lim && e.a[2] > -off && e.a[2] < off && e.a[5] > -off && e.a[5] < off,
                   "affine coefficients of a table entry out of range");
    }
    stats = stats || e.op == RA_AUTOCONTRAST || e.op == RA_EQUALIZE || e.op == RA_CONTRAST;
  }
  CSTP_REQUIRE(!stats || (lut && mean), "AutoContrast / Equalize / Contrast need the lut [b][t][3][256] and mean [b][t] buffers");
  hipStream_t st = as_stream(stream);
  if (stats) {
    hipLaunchKernelGGL(randaug_stats_kernel, dim3(t, b), dim3(256), 0, st, src, table_dev, lut, mean, t, s * s);
    CSTP_LAUNCH_CHECK();
  }
  const int npix = t * s * s;
  const int vec = (npix % 16) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16) == 0;
  const int blocks = (npix + 255) / 256;        // (a pointwise clip uses a sixteenth of them; the rest find nothing to do)
  hipLaunchKernelGGL(randaug_apply_kernel, dim3(blocks > 1024 ? 1024 : blocks, b), dim3(256), 0, st, src, dst, table_dev, lut, mean,
                     t, s, vec);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_randaug_finish(void* stream, const uint8_t* src, float* out, const cstp_randaug_finish_entry* table_dev,
                                   const cstp_randaug_finish_entry* table_host, int32_t b, int32_t t, int32_t s, int32_t out_slots) {
  using namespace cstp;
  static_assert(sizeof(cstp_randaug_finish_entry) == 32, "cstp_randaug_finish_entry is packed by the host as 32 bytes");
  CSTP_REQUIRE(src && out && table_dev && table_host, "null argument");
  CSTP_REQUIRE(ra_shape_ok(b, t, s) && out_slots > 0, "bad shape");
  for (int i = 0; i < b; ++i) {
    const cstp_randaug_finish_entry& e = table_host[i];
    CSTP_REQUIRE(e.out_slot >= 0 && e.out_slot < out_slots, "output slot of a table entry leaves the buffer");
    CSTP_REQUIRE(e.w >= 0 && e.h >= 0, "negative box in a table entry");
    if (e.w > 0 || e.h > 0)
      CSTP_REQUIRE(e.w > 0 && e.h > 0 && e.x0 >= 0 && e.y0 >= 0 && e.x0 <= s - e.w && e.y0 <= s - e.h, "erased box of a table entry leaves the clip");
  }
  const int npix = t * s * s, blocks = (npix + 255) / 256;
  hipLaunchKernelGGL(randaug_finish_kernel, dim3(blocks > 1024 ? 1024 : blocks, b), dim3(256), 0, as_stream(stream), src, out,
                     table_dev, t, s, out_slots);
  CSTP_LAUNCH_CHECK();
  return 0;
}
