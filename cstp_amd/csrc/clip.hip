// GPU clip assembly for the CSTP data path: decoded uint8 video frames resident in HBM -> normalised fp32 clip tensors.
// Per frame of a clip (reference: data_process/datasets.py:876-948 + preprocess_data.py:479-581,1103-1110, the `null_transform`
// path):  Image.transpose(ROTATE_*) -> Image.crop(box) -> Image.resize((S, S), Image.BICUBIC) -> [FLIP_LEFT_RIGHT] ->
// ToTensor -> x * 2 - 1 clamped to [-1, 1] -> stacked as [3][T][S][S].
// The resize is Pillow's algorithm (libImaging/Resample.c) bit for bit: separable, horizontal pass first with a uint8
// intermediate, 22-bit fixed-point coefficients (computed on the host exactly as precompute_coeffs / normalize_coeffs_8bpc do
// and passed in), accumulator seeded with 1 << 21, arithmetic shift, clamp to 0..255.  Rotation and crop are folded into the
// source indexing of the horizontal pass (a box may reach past the rotated frame -- the second crop of a pair whose clips are
// rotated differently does, preprocess_data.py:535-541 checks only two of its four sides -- and reads zeros there, as
// Image.crop does), the flip and the normalisation into the store of the vertical pass, so a frame is read
// once and the clip is written once; both kernels are HBM/latency-trivial next to a training step (a 16-frame 112x112 clip from
// 240x320 frames: 3.7 MB in, 2.4 MB out).
// The fine-tune / validation / video-test clips (datasets.py:952-1097 UcfFineTune, preprocess_data.py:1131-1149) come a BATCH at a
// time through cstp_clip_batch_forward at the end of this file: one descriptor table, two launches for any number of clips.
// A batch of pre-training pairs takes the same road, with a rotation code per clip (clip_ops.assemble_pairs).
// Then cstp_clip_mix, mixup / CutMix of an assembled fp32 batch for fine-tuning (one launch, one table entry per sample), and last
// randaug.h: RandAugment and random erasing on a batch of 8-bit clips, one operation table per layer.
#include "common.h"

namespace cstp {

constexpr int CLIP_PRECISION_BITS = 22;

__device__ __forceinline__ int clip8_fixed(int acc) {
  const int v = acc >> CLIP_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// tmp[t][y][xx][c] = clip8(1 << 21 + sum_i src(t, y + row_first, x0(xx) + i, c) * kh[xx][i])   over the cropped image
__global__ void clip_resize_h_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ frame_idx,
                                     uint8_t* __restrict__ tmp, int F, int H, int W, int T, int rot, int bx0, int by0,
                                     int size, const int32_t* __restrict__ kh, const int32_t* __restrict__ bh, int ksh,
                                     int row_first, int rows) {
  const size_t total = (size_t)T * rows * size;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % size);
    const size_t r = i / size;
    const int y = (int)(r % rows), t = (int)(r / rows);
    int f = frame_idx[t];
    f = f < 0 ? 0 : (f >= F ? F - 1 : f);
    const uint8_t* fp = frames + (size_t)f * H * W * 3;
    const int x0 = bh[2 * xx], n = bh[2 * xx + 1];
    const int ry = by0 + y + row_first;                  // row in the ROTATED frame
    int a0 = 1 << (CLIP_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
      const int rx = bx0 + x0 + j;                        // column in the rotated frame
      int ox, oy;                                         // the same pixel in the stored frame (inverse of Image.transpose)
      if (rot == 90) { ox = W - 1 - ry; oy = rx; }
      else if (rot == 180) { ox = W - 1 - rx; oy = H - 1 - ry; }
      else if (rot == 270) { ox = ry; oy = H - 1 - rx; }
      else { ox = rx; oy = ry; }
      if (ox < 0 || ox >= W || oy < 0 || oy >= H) continue;   // Image.crop beyond the frame reads black (0, 0, 0)
      const uint8_t* p = fp + ((size_t)oy * W + ox) * 3;
      const int k = kh[xx * ksh + j];
      a0 += (int)p[0] * k; a1 += (int)p[1] * k; a2 += (int)p[2] * k;
    }
    uint8_t* o = tmp + i * 3;
    o[0] = (uint8_t)clip8_fixed(a0); o[1] = (uint8_t)clip8_fixed(a1); o[2] = (uint8_t)clip8_fixed(a2);
  }
}

// out[c][t][yy][flip ? S-1-xx : xx] = clamp(clip8(1 << 21 + sum_i tmp[t][y0(yy) - row_first + i][xx][c] * kv[yy][i]) / 255 * 2 - 1)
// U8: the resized frames stay 8-bit RGB [t][yy][xx][3] (no flip, no normalisation) for the base_transform operations below
template <bool U8>
__global__ void clip_resize_v_kernel(const uint8_t* __restrict__ tmp, float* __restrict__ out, uint8_t* __restrict__ out8, int T,
                                     int size, int flip, const int32_t* __restrict__ kv, const int32_t* __restrict__ bv, int ksv,
                                     int row_first, int rows) {
  const size_t total = (size_t)T * size * size;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % size);
    const size_t r = i / size;
    const int yy = (int)(r % size), t = (int)(r / size);
    const int y0 = bv[2 * yy] - row_first, n = bv[2 * yy + 1];
    int a0 = 1 << (CLIP_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
      const uint8_t* p = tmp + (((size_t)t * rows + (y0 + j)) * size + xx) * 3;
      const int k = kv[yy * ksv + j];
      a0 += (int)p[0] * k; a1 += (int)p[1] * k; a2 += (int)p[2] * k;
    }
    if constexpr (U8) {
      uint8_t* o8 = out8 + i * 3;
      o8[0] = (uint8_t)clip8_fixed(a0); o8[1] = (uint8_t)clip8_fixed(a1); o8[2] = (uint8_t)clip8_fixed(a2);
      continue;
    }
    const int xo = flip ? size - 1 - xx : xx;
    const size_t plane = (size_t)T * size * size;
    const size_t o = ((size_t)t * size + yy) * size + xo;
    const int c8[3] = {clip8_fixed(a0), clip8_fixed(a1), clip8_fixed(a2)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = (float)c8[c] / 255.0f;                   // transforms.ToTensor()
      v = v * 2.0f - 1.0f;                               // ClipNormalize('tf')
      out[c * plane + o] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
  }
}

// ---- the base_transform branch (preprocess_data.py:1110-1121) on 8-bit RGB clips [t][h][w][3]; every kernel reproduces the
//      Pillow call the reference makes bit for bit (oracle/pil_ops.py restates them in numpy and is pinned against Pillow) ----

// Image.rotate(angle), NEAREST, same size, black fill: Geometry.c affine_fixed, 16.16 fixed point (coefficients from the host)
__global__ void clip_rotate_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int T, int H, int W, int a0, int a1,
                                   int a2, int a3, int a4, int a5) {
  const size_t total = (size_t)T * H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const size_t r = i / W;
    const int y = (int)(r % H), t = (int)(r / H);
    const int xin = (a2 + a1 * y + a0 * x) >> 16, yin = (a5 + a4 * y + a3 * x) >> 16;
    uint8_t v0 = 0, v1 = 0, v2 = 0;
    if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
      const uint8_t* p = src + (((size_t)t * H + yin) * W + xin) * 3;
      v0 = p[0]; v1 = p[1]; v2 = p[2];
    }
    uint8_t* o = dst + i * 3;
    o[0] = v0; o[1] = v1; o[2] = v2;
  }
}

// Image.convert('L') of RGB (Convert.c rgb2l): ITU-R 601-2 luma in 16-bit fixed point
__device__ __forceinline__ int luma8(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// per-frame mean of the luma for ImageEnhance.Contrast: int(sum / count + 0.5) (ImageStat.Stat(...).mean[0] is a double)
__global__ void __launch_bounds__(256) clip_luma_mean_kernel(const uint8_t* __restrict__ src, int32_t* __restrict__ mean, int HW) {
  __shared__ unsigned long long red[4];
  const uint8_t* p = src + (size_t)blockIdx.x * HW * 3;
  unsigned long long acc = 0;
  for (int i = threadIdx.x; i < HW; i += 256) acc += (unsigned long long)luma8(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) mean[blockIdx.x] = (int32_t)((double)(red[0] + red[1] + red[2] + red[3]) / (double)HW + 0.5);
}

// Image.blend(degenerate, image, alpha) (Blend.c; single precision, NO fused multiply-add): interpolation truncates,
// extrapolation clips.  mode 0: degenerate = black (Brightness); 1: the frame's mean luma (Contrast); 2: the pixel's luma (Color)
// (hipcc contracts a * b + c into a fused multiply-add by default and its __fmul_rn / __fadd_rn are plain operators: the
//  functions that must round like the C code they reproduce switch the contraction off AND pass every product that feeds an
//  addition through an opaque register move, which no later pass can fuse across)
__device__ __forceinline__ float rounded(float x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ uint8_t blend8(int deg, int v, float alpha, bool inside) {
#pragma clang fp contract(off)
  const float t = __fadd_rn((float)deg, rounded(__fmul_rn(alpha, (float)(v - deg))));
  if (inside) return (uint8_t)(int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (uint8_t)(int)t);
}
__global__ void clip_blend_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int T, int HW, int mode, float alpha,
                                  const int32_t* __restrict__ mean) {
  const bool inside = alpha >= 0.0f && alpha <= 1.0f;
  const size_t total = (size_t)T * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t* p = src + i * 3;
    const int r = p[0], g = p[1], b = p[2];
    const int deg = mode == 0 ? 0 : (mode == 1 ? mean[i / HW] : luma8(r, g, b));
    uint8_t* o = dst + i * 3;
    o[0] = blend8(deg, r, alpha, inside); o[1] = blend8(deg, g, alpha, inside); o[2] = blend8(deg, b, alpha, inside);
  }
}

// torchvision adjust_hue on PIL images: RGB -> HSV (Convert.c rgb2hsv_row), h += shift modulo 256, HSV -> RGB (hsv2rgb).  The
// float / double mix of the C statements is reproduced operation by operation (oracle/pil_ops.py: exact on all 2^24 colours).
__device__ __forceinline__ void rgb2hsv8(int r, int g, int b, int& uh, int& us, int& uv) {
#pragma clang fp contract(off)
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  uv = maxc;
  if (minc == maxc) { uh = 0; us = 0; return; }
  const float cr = (float)(maxc - minc);
  const float s = __fdiv_rn(cr, (float)maxc);
  const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
  float h;
  if (r == maxc) h = __fsub_rn(bc, gc);
  else if (g == maxc) h = (float)__dsub_rn(__dadd_rn(2.0, (double)rc), (double)bc);
  else h = (float)__dsub_rn(__dadd_rn(4.0, (double)gc), (double)rc);
  h = (float)fmod(__dadd_rn(__ddiv_rn((double)h, 6.0), 1.0), 1.0);
  const int ih = (int)__dmul_rn((double)h, 255.0), is = (int)__dmul_rn((double)s, 255.0);
  uh = ih < 0 ? 0 : (ih > 255 ? 255 : ih);
  us = is < 0 ? 0 : (is > 255 ? 255 : is);
}
__device__ __forceinline__ int round_half_away(float x) {      // C round() of a non-negative value, clipped to 0..255
  const int v = (int)floor((double)x + 0.5);
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}
__device__ __forceinline__ void hsv2rgb8(int h, int s, int v, int& r, int& g, int& b) {
#pragma clang fp contract(off)
  if (s == 0) { r = g = b = v; return; }
  const float hf = __fdiv_rn(__fmul_rn((float)h, 6.0f), 255.0f);
  const int i = (int)floorf(hf);
  const float f = __fsub_rn(hf, (float)i);
  const float fs = __fdiv_rn((float)s, 255.0f), vf = (float)v;
  const int p = round_half_away(__fmul_rn(vf, __fsub_rn(1.0f, fs)));
  const int q = round_half_away(__fmul_rn(vf, __fsub_rn(1.0f, rounded(__fmul_rn(fs, f)))));
  const int t = round_half_away(__fmul_rn(vf, __fsub_rn(1.0f, rounded(__fmul_rn(fs, __fsub_rn(1.0f, f))))));
  switch (i % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
}
// mode 0: hue shift (RGB -> RGB); 1: RGB -> HSV; 2: HSV -> RGB (the two conversions alone, for the exhaustive tests)
__global__ void clip_hue_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t npix, int shift, int mode) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (size_t)gridDim.x * blockDim.x) {
    const uint8_t* p = src + i * 3;
    int a = p[0], b = p[1], c = p[2], h, s, v, r, g, bb;
    if (mode == 2) { h = a; s = b; v = c; }
    else rgb2hsv8(a, b, c, h, s, v);
    if (mode == 1) { r = h; g = s; bb = v; }
    else { h = (h + shift) & 255; hsv2rgb8(h, s, v, r, g, bb); }
    uint8_t* o = dst + i * 3;
    o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)bb;
  }
}

// ClipRandomGray.grayscale: frame t keeps channel ch[t] in all three channels (ch[t] < 0: the frame is copied)
__global__ void clip_gray_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int T, int HW,
                                 const int32_t* __restrict__ ch) {
  const size_t total = (size_t)T * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int c = ch[i / HW];
    const uint8_t* p = src + i * 3;
    uint8_t* o = dst + i * 3;
    if (c < 0) { o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; }
    else { const uint8_t v = p[c]; o[0] = v; o[1] = v; o[2] = v; }
  }
}

// one pass of BoxBlur.c ImagingLineBoxBlur8 along x (vertical == 0) or y: box of 2 r + 1 pixels of weight ww plus the two next
// pixels of weight fw, 24-bit fixed point, edge pixels repeated beyond the line's ends
__global__ void clip_box_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int T, int H, int W, int vertical,
                                     int radius, unsigned ww, unsigned fw) {
  const size_t total = (size_t)T * H * W;
  const int n = vertical ? H : W;
  const size_t step = vertical ? (size_t)W * 3 : 3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const size_t rr = i / W;
    const int y = (int)(rr % H);
    const int pos = vertical ? y : x;
    const uint8_t* line = src + i * 3 - (size_t)pos * step;        // element 0 of my line
    unsigned s0 = 0, s1 = 0, s2 = 0;
    for (int k = pos - radius; k <= pos + radius; ++k) {
      const uint8_t* p = line + (size_t)(k < 0 ? 0 : (k > n - 1 ? n - 1 : k)) * step;
      s0 += p[0]; s1 += p[1]; s2 += p[2];
    }
    const int kl = pos - radius - 1, kr = pos + radius + 1;
    const uint8_t* pl = line + (size_t)(kl < 0 ? 0 : kl) * step;
    const uint8_t* pr = line + (size_t)(kr > n - 1 ? n - 1 : kr) * step;
    uint8_t* o = dst + i * 3;
    o[0] = (uint8_t)((s0 * ww + ((unsigned)pl[0] + pr[0]) * fw + (1u << 23)) >> 24);
    o[1] = (uint8_t)((s1 * ww + ((unsigned)pl[1] + pr[1]) * fw + (1u << 23)) >> 24);
    o[2] = (uint8_t)((s2 * ww + ((unsigned)pl[2] + pr[2]) * fw + (1u << 23)) >> 24);
  }
}

// [FLIP_LEFT_RIGHT] -> ToTensor -> x * 2 - 1 clamped: uint8 [t][s][s][3] -> fp32 [3][t][s][s]
__global__ void clip_finish_kernel(const uint8_t* __restrict__ src, float* __restrict__ out, int T, int H, int W, int flip) {
  const size_t total = (size_t)T * H * W, plane = total;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const size_t o = i - x + (flip ? W - 1 - x : x);
    const uint8_t* p = src + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = (float)p[c] / 255.0f;
      v = v * 2.0f - 1.0f;
      out[c * plane + o] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
  }
}

static inline int clip_grid(size_t n) {
  size_t b = (n + 255) / 256;
  return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

}  // namespace cstp

using namespace cstp;

extern "C" int cstp_clip_assemble(void* stream, const uint8_t* frames, int32_t f, int32_t h, int32_t w,
                                  const int32_t* frame_idx, int32_t t, int32_t rot, int32_t box_x0, int32_t box_y0,
                                  int32_t size, int32_t flip, const int32_t* kh, const int32_t* bh, int32_t ksh,
                                  const int32_t* kv, const int32_t* bv, int32_t ksv, int32_t row_first, int32_t rows,
                                  uint8_t* tmp, float* out) {
  CSTP_REQUIRE(frames && frame_idx && kh && bh && kv && bv && tmp && out, "null argument");
  CSTP_REQUIRE(f > 0 && h > 0 && w > 0 && t > 0 && size > 0 && ksh > 0 && ksv > 0 && rows > 0 && row_first >= 0, "bad shape");
  CSTP_REQUIRE(rot == 0 || rot == 90 || rot == 180 || rot == 270, "rotation must be 0 / 90 / 180 / 270");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(clip_resize_h_kernel, dim3(clip_grid((size_t)t * rows * size)), dim3(256), 0, s, frames, frame_idx, tmp, f, h, w,
                     t, rot, box_x0, box_y0, size, kh, bh, ksh, row_first, rows);
  CSTP_LAUNCH_CHECK();
  hipLaunchKernelGGL((clip_resize_v_kernel<false>), dim3(clip_grid((size_t)t * size * size)), dim3(256), 0, s, tmp, out, nullptr, t,
                     size, flip ? 1 : 0, kv, bv, ksv, row_first, rows);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_assemble_u8(void* stream, const uint8_t* frames, int32_t f, int32_t h, int32_t w,
                                     const int32_t* frame_idx, int32_t t, int32_t rot, int32_t box_x0, int32_t box_y0,
                                     int32_t size, const int32_t* kh, const int32_t* bh, int32_t ksh, const int32_t* kv,
                                     const int32_t* bv, int32_t ksv, int32_t row_first, int32_t rows, uint8_t* tmp,
                                     uint8_t* out) {
  CSTP_REQUIRE(frames && frame_idx && kh && bh && kv && bv && tmp && out, "null argument");
  CSTP_REQUIRE(f > 0 && h > 0 && w > 0 && t > 0 && size > 0 && ksh > 0 && ksv > 0 && rows > 0 && row_first >= 0, "bad shape");
  CSTP_REQUIRE(rot == 0 || rot == 90 || rot == 180 || rot == 270, "rotation must be 0 / 90 / 180 / 270");
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(clip_resize_h_kernel, dim3(clip_grid((size_t)t * rows * size)), dim3(256), 0, s, frames, frame_idx, tmp, f, h, w,
                     t, rot, box_x0, box_y0, size, kh, bh, ksh, row_first, rows);
  CSTP_LAUNCH_CHECK();
  hipLaunchKernelGGL((clip_resize_v_kernel<true>), dim3(clip_grid((size_t)t * size * size)), dim3(256), 0, s, tmp, nullptr, out, t,
                     size, 0, kv, bv, ksv, row_first, rows);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_rotate(void* stream, const uint8_t* src, uint8_t* dst, int32_t t, int32_t h, int32_t w,
                                const int32_t* coef6) {
  CSTP_REQUIRE(src && dst && coef6 && src != dst, "null or aliased argument");
  CSTP_REQUIRE(t > 0 && h > 0 && w > 0 && h < 16384 && w < 16384, "bad shape");
  hipLaunchKernelGGL(clip_rotate_kernel, dim3(clip_grid((size_t)t * h * w)), dim3(256), 0, as_stream(stream), src, dst, t, h, w,
                     coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_blend(void* stream, const uint8_t* src, uint8_t* dst, int32_t t, int32_t h, int32_t w, int32_t mode,
                               float alpha, int32_t* ws_means) {
  CSTP_REQUIRE(src && dst, "null argument");
  CSTP_REQUIRE(t > 0 && h > 0 && w > 0 && mode >= 0 && mode <= 2, "bad shape or mode");
  CSTP_REQUIRE(mode != 1 || ws_means != nullptr, "contrast needs t int32 of workspace");
  hipStream_t s = as_stream(stream);
  if (mode == 1) {
    hipLaunchKernelGGL(clip_luma_mean_kernel, dim3(t), dim3(256), 0, s, src, ws_means, h * w);
    CSTP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(clip_blend_kernel, dim3(clip_grid((size_t)t * h * w)), dim3(256), 0, s, src, dst, t, h * w, mode, alpha, ws_means);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_hue(void* stream, const uint8_t* src, uint8_t* dst, size_t npix, int32_t shift, int32_t mode) {
  CSTP_REQUIRE(src && dst, "null argument");
  CSTP_REQUIRE(npix > 0 && shift >= 0 && shift <= 255 && mode >= 0 && mode <= 2, "bad size, shift or mode");
  hipLaunchKernelGGL(clip_hue_kernel, dim3(clip_grid(npix)), dim3(256), 0, as_stream(stream), src, dst, npix, shift, mode);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_gray(void* stream, const uint8_t* src, uint8_t* dst, int32_t t, int32_t h, int32_t w,
                              const int32_t* channel) {
  CSTP_REQUIRE(src && dst && channel, "null argument");
  CSTP_REQUIRE(t > 0 && h > 0 && w > 0, "bad shape");
  hipLaunchKernelGGL(clip_gray_kernel, dim3(clip_grid((size_t)t * h * w)), dim3(256), 0, as_stream(stream), src, dst, t, h * w, channel);
  CSTP_LAUNCH_CHECK();
  return 0;
}

extern "C" int cstp_clip_box_blur(void* stream, uint8_t* img, uint8_t* tmp, int32_t t, int32_t h, int32_t w, int32_t radius,
                                  uint32_t ww, uint32_t fw, int32_t passes) {
  CSTP_REQUIRE(img && tmp && img != tmp, "null or aliased argument");
  CSTP_REQUIRE(t > 0 && h > 0 && w > 0 && radius >= 0 && radius < 4096 && passes >= 1 && passes <= 8, "bad shape, radius or passes");
  // (the weights of a pass sum to at most 1 << 24, so the 32-bit accumulators cannot overflow)
  CSTP_REQUIRE((unsigned long long)ww * (2 * radius + 1) + 2ull * fw <= (1ull << 24), "weights exceed 1 << 24");
  hipStream_t s = as_stream(stream);
  uint8_t* a = img;
  uint8_t* b = tmp;
  for (int v = 0; v < 2; ++v)
    for (int p = 0; p < passes; ++p) {
      hipLaunchKernelGGL(clip_box_blur_kernel, dim3(clip_grid((size_t)t * h * w)), dim3(256), 0, s, a, b, t, h, w, v, radius, ww, fw);
      CSTP_LAUNCH_CHECK();
      uint8_t* sw = a; a = b; b = sw;
    }
  if (a != img) {        // an odd number of launches ends in tmp
    if (hipMemcpyAsync(img, a, (size_t)t * h * w * 3, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail("hipMemcpyAsync failed%s", "");
  }
  return 0;
}

extern "C" int cstp_clip_finish(void* stream, const uint8_t* src, float* out, int32_t t, int32_t h, int32_t w, int32_t flip) {
  CSTP_REQUIRE(src && out, "null argument");
  CSTP_REQUIRE(t > 0 && h > 0 && w > 0, "bad shape");
  hipLaunchKernelGGL(clip_finish_kernel, dim3(clip_grid((size_t)t * h * w)), dim3(256), 0, as_stream(stream), src, out, t, h, w,
                     flip ? 1 : 0);
  CSTP_LAUNCH_CHECK();
  return 0;
}

// ---- batched, descriptor-driven assembly (cstp_clip_batch_forward): the fine-tune / validation / video-test data path -------
// A whole batch -- clips of different videos, frame sizes, boxes and scales -- in two launches: blockIdx.y picks the clip's
// descriptor, blockIdx.x strides over that clip's pixels.  The arithmetic is that of clip_resize_h_kernel / clip_resize_v_kernel
// (rotation included: desc.rot, see below); new is the output WINDOW: of the resized rw x rh image only the size x size window at
// (win_x, win_y) is produced, so ClipScale -> ClipCenterCrop (240x320 -> 128x170 -> 112x112) computes 112 of 170 columns and
// only the tmp rows the window's vertical taps read, and the result still equals resize-then-crop bit for bit because an output
// pixel depends on its own taps alone.
// What bounds them: gather latency, not bandwidth.  A batch of 32 clips of 16 frames from 240x320 frames reads at most 118 MB of
// frames and writes 77 MB of fp32 (~30 us at the HBM rate); every output pixel instead walks 5..13 taps of 3 bytes behind two
// dependent table loads (bounds, then coefficients), so the passes run at the rate the L1 / L2 return those short reads -- the
// lanes of a wave read neighbouring output columns, whose tap spans overlap, and the vertical pass reads tmp rows that 64 lanes
// share coalesced.  Tables (at most a few KiB per axis) and descriptors stay in the scalar / L2 caches.  Next to a training step
// the two launches are noise; what the batching removes is the 2+ launches, the blocking index upload and the allocation PER CLIP.
// Rotation (desc.rot, the pre-training pairs): each tap is mapped to the stored frame as clip_resize_h_kernel maps it; rot == 0
// takes the branch it always took.  Under 180 a wave still reads one stored row, backwards.  Under 90 / 270 the roles of the
// axes swap: the taps of ONE output pixel walk a column of the stored frame (stride w * 3 bytes, a new 128-byte line per tap),
// and the 64 lanes of a wave -- neighbouring output columns of one row -- read 64 different stored rows at one stored column,
// so a wave's tap load touches up to 64 lines instead of the 2..6 of the row walk.  The lines are not wasted: the output rows
// y + 1 .. y + 42 (128 / 3 pixels) of the same frame read the same lines at the neighbouring stored columns, and those rows
// belong to the next waves of the same or the next block, so the reuse is served by the L2 (a 240x320 frame is 230 KB).
// No measured change followed from this yet: the by-rotation line of tools/bench_frames.py has not been run on a GPU, and no
// tiling (a transposing LDS stage for 90 / 270) is attempted before it shows that the column walk costs time worth having.
namespace cstp {

__global__ void __launch_bounds__(256) clip_batch_h_kernel(const cstp_clip_batch_desc* __restrict__ descs,
                                                           const int32_t* __restrict__ frame_idx, uint8_t* __restrict__ tmp,
                                                           int T, int size) {
  const cstp_clip_batch_desc d = descs[blockIdx.y];
  const size_t total = (size_t)T * d.rows * size;
  uint8_t* const tp = tmp + (size_t)d.tmp_off * 3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % size);
    const size_t r = i / size;
    const int y = (int)(r % d.rows), t = (int)(r / d.rows);
    int f = frame_idx[d.idx_off + t];
    f = f < 0 ? 0 : (f >= d.f ? d.f - 1 : f);
    const int cx = d.win_x + xx;                           // column of the resized image
    const int x0 = d.bh[2 * cx];
    int n = d.bh[2 * cx + 1];
    n = n > d.ksh ? d.ksh : n;
    const int oy = d.box_y0 + d.row_first + y;             // row in the (rotated) frame
    int a0 = 1 << (CLIP_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    if (d.rot != 0) {                                      // uniform over the block: one descriptor per blockIdx.y
      const uint8_t* fp = d.frames + (size_t)f * d.h * d.w * 3;
      const int32_t* k = d.kh + (size_t)cx * d.ksh;
      for (int j = 0; j < n; ++j) {
        const int rx = d.box_x0 + x0 + j;                  // column in the rotated frame
        int sx, sy;                                        // the same pixel in the stored frame (inverse of Image.transpose)
        if (d.rot == 90) { sx = d.w - 1 - oy; sy = rx; }
        else if (d.rot == 180) { sx = d.w - 1 - rx; sy = d.h - 1 - oy; }
        else { sx = oy; sy = d.h - 1 - rx; }               // 270
        if (sx < 0 || sx >= d.w || sy < 0 || sy >= d.h) continue;   // Image.crop beyond the rotated frame reads black
        const uint8_t* p = fp + ((size_t)sy * d.w + sx) * 3;
        const int kj = k[j];
        a0 += (int)p[0] * kj; a1 += (int)p[1] * kj; a2 += (int)p[2] * kj;
      }
    } else if (oy >= 0 && oy < d.h) {                      // Image.crop beyond the frame reads black (0, 0, 0)
      const uint8_t* row = d.frames + ((size_t)f * d.h + oy) * d.w * 3;
      const int32_t* k = d.kh + (size_t)cx * d.ksh;
      for (int j = 0; j < n; ++j) {
        const int ox = d.box_x0 + x0 + j;
        if (ox < 0 || ox >= d.w) continue;
        const uint8_t* p = row + (size_t)ox * 3;
        const int kj = k[j];
        a0 += (int)p[0] * kj; a1 += (int)p[1] * kj; a2 += (int)p[2] * kj;
      }
    }
    uint8_t* o = tp + i * 3;
    o[0] = (uint8_t)clip8_fixed(a0); o[1] = (uint8_t)clip8_fixed(a1); o[2] = (uint8_t)clip8_fixed(a2);
  }
}

__global__ void __launch_bounds__(256) clip_batch_v_kernel(const cstp_clip_batch_desc* __restrict__ descs,
                                                           const uint8_t* __restrict__ tmp, float* __restrict__ out,
                                                           uint8_t* __restrict__ out8, int T, int size) {
  const cstp_clip_batch_desc d = descs[blockIdx.y];
  const size_t total = (size_t)T * size * size;
  const uint8_t* const tp = tmp + (size_t)d.tmp_off * 3;
  const size_t plane = total;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % size);
    const size_t r = i / size;
    const int yy = (int)(r % size), t = (int)(r / size);
    const int cy = d.win_y + yy;                           // row of the resized image
    const int y0 = d.bv[2 * cy] - d.row_first;
    int n = d.bv[2 * cy + 1];
    n = n > d.ksv ? d.ksv : n;
    const int32_t* k = d.kv + (size_t)cy * d.ksv;
    int a0 = 1 << (CLIP_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
      const int ry = y0 + j;
      if (ry < 0 || ry >= d.rows) continue;                // never taken with consistent tables; keeps a bad table inside tmp
      const uint8_t* p = tp + (((size_t)t * d.rows + ry) * size + xx) * 3;
      const int kj = k[j];
      a0 += (int)p[0] * kj; a1 += (int)p[1] * kj; a2 += (int)p[2] * kj;
    }
    const int c8[3] = {clip8_fixed(a0), clip8_fixed(a1), clip8_fixed(a2)};
    if (d.out8_slot >= 0) {                                // 8-bit RGB for the colour-jitter kernels: no flip, no normalisation
      uint8_t* o8 = out8 + ((size_t)d.out8_slot * plane + i) * 3;
      o8[0] = (uint8_t)c8[0]; o8[1] = (uint8_t)c8[1]; o8[2] = (uint8_t)c8[2];
      continue;
    }
    const int xo = d.flip ? size - 1 - xx : xx;
    float* o = out + (size_t)d.out_slot * 3 * plane + ((size_t)t * size + yy) * size + xo;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = (float)c8[c] / 255.0f;                     // transforms.ToTensor()
      v = v * 2.0f - 1.0f;                                 // ClipNormalize('tf')
      o[c * plane] = fminf(fmaxf(v, -1.0f), 1.0f);
    }
  }
}

}  // namespace cstp

extern "C" size_t cstp_clip_batch_desc_bytes(void) { return sizeof(cstp_clip_batch_desc); }

extern "C" int cstp_clip_batch_forward(void* stream, const cstp_clip_batch_desc* desc_dev, const cstp_clip_batch_desc* desc_host,
                                       int32_t n, int32_t t, int32_t size, const int32_t* frame_idx, int32_t n_idx, uint8_t* tmp,
                                       int64_t tmp_pixels, float* out, int32_t out_slots, uint8_t* out8, int32_t out8_slots) {
  static_assert(sizeof(cstp_clip_batch_desc) == 120, "cstp_clip_batch_desc is packed by the host as 120 bytes");
  CSTP_REQUIRE(desc_dev && desc_host && frame_idx && tmp, "null argument");
  CSTP_REQUIRE(n > 0 && n <= 65535 && t > 0 && size > 0 && size <= 4096 && n_idx > 0 && tmp_pixels > 0, "bad shape");
  CSTP_REQUIRE(out_slots >= 0 && out8_slots >= 0 && (out || out_slots == 0) && (out8 || out8_slots == 0), "bad output");
  size_t most_h = 0;
  for (int i = 0; i < n; ++i) {      // every offset the kernels form from a descriptor is checked here, against the sizes given
    const cstp_clip_batch_desc& d = desc_host[i];
    CSTP_REQUIRE(d.frames && d.kh && d.bh && d.kv && d.bv, "null pointer in a descriptor");
    CSTP_REQUIRE(d.f > 0 && d.h > 0 && d.w > 0 && d.h < 32768 && d.w < 32768, "bad frame shape in a descriptor");
    CSTP_REQUIRE(d.rot == 0 || d.rot == 90 || d.rot == 180 || d.rot == 270, "rotation of a descriptor must be 0 / 90 / 180 / 270");
    CSTP_REQUIRE(d.idx_off >= 0 && (int64_t)d.idx_off + t <= n_idx, "frame indices of a descriptor leave the index array");
    CSTP_REQUIRE(d.ksh > 0 && d.ksv > 0 && d.rw > 0 && d.rh > 0, "bad table shape in a descriptor");
    CSTP_REQUIRE(d.win_x >= 0 && d.win_y >= 0 && (int64_t)d.win_x + size <= d.rw && (int64_t)d.win_y + size <= d.rh,
                 "output window of a descriptor leaves the resized image");
    CSTP_REQUIRE(d.row_first >= 0 && d.rows > 0 && d.rows < 32768, "bad tmp rows in a descriptor");
    CSTP_REQUIRE(d.tmp_off >= 0 && d.tmp_off + (int64_t)t * d.rows * size <= tmp_pixels, "tmp of a descriptor leaves the buffer");
    CSTP_REQUIRE((d.out_slot >= 0) != (d.out8_slot >= 0), "a descriptor needs exactly one of out_slot / out8_slot");
    CSTP_REQUIRE(d.out_slot < out_slots && d.out8_slot < out8_slots, "output slot of a descriptor leaves its buffer");
    const size_t items = (size_t)t * d.rows * size;
    most_h = items > most_h ? items : most_h;
  }
  hipStream_t s = as_stream(stream);
  const size_t bh_ = (most_h + 255) / 256, bv_ = ((size_t)t * size * size + 255) / 256;
  hipLaunchKernelGGL(clip_batch_h_kernel, dim3((unsigned)(bh_ > 2048 ? 2048 : bh_), n), dim3(256), 0, s, desc_dev, frame_idx, tmp, t,
                     size);
  CSTP_LAUNCH_CHECK();
  hipLaunchKernelGGL(clip_batch_v_kernel, dim3((unsigned)(bv_ > 2048 ? 2048 : bv_), n), dim3(256), 0, s, desc_dev, tmp, out, out8, t,
                     size);
  CSTP_LAUNCH_CHECK();
  return 0;
}

// ---- mixup / CutMix over a batch of fp32 clips (fine-tuning: cstp_amd/mix.py) -------------------------------------------------
// x, y: [b][planes][h][w]; one launch, blockIdx.y = sample, its table entry read by every block that serves it.  The entry is
// checked where it is used -- partner in [0, b), known mode, box inside the frame -- and a malformed one is served as a copy,
// never followed (the rule of the LARS tables, lars.h).  A sample that is its own partner is a copy too: exact, whatever lam.
// VEC: w % 4 == 0 and both bases 16-byte aligned, so every sample and every row starts on a 16-byte boundary and a float4
// group never straddles a row; a box edge inside a group is resolved per element.  CutMix copies bits (no arithmetic).
namespace cstp {

template <bool VEC>
__global__ void __launch_bounds__(256) clip_mix_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       const cstp_clip_mix_entry* __restrict__ table, int b, int planes, int h,
                                                       int w) {
  const int i = blockIdx.y;
  const cstp_clip_mix_entry e = table[i];
  int mode = e.mode;
  const bool ok = e.partner >= 0 && e.partner < b && (mode == 1 || mode == 2) && e.y0 >= 0 && e.y0 <= e.y1 && e.y1 <= h &&
                  e.x0 >= 0 && e.x0 <= e.x1 && e.x1 <= w;
  if (!ok || e.partner == i) mode = 0;
  const int partner = mode ? e.partner : i;
  const size_t n = (size_t)planes * h * w;
  const float* __restrict__ xs = x + (size_t)i * n;
  const float* __restrict__ xp = x + (size_t)partner * n;
  float* __restrict__ ys = y + (size_t)i * n;
  const float lam = e.lam, rem = 1.f - e.lam;
  if (VEC) {
    const size_t groups = n >> 2;
    const int wg = w >> 2;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
      float4 v = reinterpret_cast<const float4*>(xs)[g];
      if (mode == 1) {
        const float4 p = reinterpret_cast<const float4*>(xp)[g];
        v.x = lam * v.x + rem * p.x; v.y = lam * v.y + rem * p.y; v.z = lam * v.z + rem * p.z; v.w = lam * v.w + rem * p.w;
      } else if (mode == 2) {
        const int col = (int)(g % wg) << 2, row = (int)((g / wg) % h);
        if (row >= e.y0 && row < e.y1 && col + 4 > e.x0 && col < e.x1) {
          const float4 p = reinterpret_cast<const float4*>(xp)[g];
          if (col >= e.x0 && col < e.x1) v.x = p.x;
          if (col + 1 >= e.x0 && col + 1 < e.x1) v.y = p.y;
          if (col + 2 >= e.x0 && col + 2 < e.x1) v.z = p.z;
          if (col + 3 >= e.x0 && col + 3 < e.x1) v.w = p.w;
        }
      }
      reinterpret_cast<float4*>(ys)[g] = v;
    }
  } else {
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256) {
      float v = xs[j];
      if (mode == 1) {
        v = lam * v + rem * xp[j];
      } else if (mode == 2) {
        const int col = (int)(j % w), row = (int)((j / w) % h);
        if (row >= e.y0 && row < e.y1 && col >= e.x0 && col < e.x1) v = xp[j];
      }
      ys[j] = v;
    }
  }
}

}  // namespace cstp

extern "C" int cstp_clip_mix(void* stream, const float* x, float* y, const cstp_clip_mix_entry* table, int32_t b, int32_t planes,
                             int32_t h, int32_t w) {
  static_assert(sizeof(cstp_clip_mix_entry) == 32, "cstp_clip_mix_entry is packed by the host as 32 bytes");
  CSTP_REQUIRE(x && y && table, "null argument");
  CSTP_REQUIRE(b > 0 && b <= 65535 && planes > 0 && h > 0 && w > 0, "bad shape");
  CSTP_REQUIRE((int64_t)b * planes * h * w <= INT32_MAX && (int64_t)planes * h <= INT32_MAX, "bad shape (more than 2^31 - 1 values)");
  CSTP_REQUIRE(y != x, "y must not alias x");
  const size_t n = (size_t)planes * h * w;
  const bool vec = (w % 4) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16) == 0;
  const size_t units = vec ? n / 4 : n, blocks = (units + 255) / 256;
  const dim3 grid((unsigned)(blocks > 1024 ? 1024 : blocks), b);
  if (vec) hipLaunchKernelGGL(clip_mix_kernel<true>, grid, dim3(256), 0, as_stream(stream), x, y, table, b, planes, h, w);
  else hipLaunchKernelGGL(clip_mix_kernel<false>, grid, dim3(256), 0, as_stream(stream), x, y, table, b, planes, h, w);
  CSTP_LAUNCH_CHECK();
  return 0;
}

#include "randaug.h"   // RandAugment layers and the erasing finish of a batch of 8-bit clips: cstp_randaug_layer, cstp_randaug_finish
