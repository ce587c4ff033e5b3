/*
 * cstp_hip.h -- C ABI of libcstp_hip.so: the MI355X (gfx950) kernels behind the CSTP
 * BYOL pre-training step (R(2+1)D, 3D-ResNet, S3D-G and I3D backbones), its fine-tune / test callers, the GPU clip
 * pipeline in front of it and the nearest-neighbour retrieval evaluation behind it.
 *
 * The reference (KT27-A/CSTP) owns no native code and no FFI: every op below is an ATen
 * call-site of its Python hot path, cited per entry point (paths relative to the
 * reference root).  A maintainer binds this library with ctypes;
 * cstp_amd/_lib.py is that binding.
 *
 * Conventions
 *   - all tensors are fp32, contiguous, NCDHW ([N][C][D][H][W]); 2-D [B][F] tensors are the
 *     D=H=W=1 case.  Labels are int64.
 *   - every pointer is a DEVICE pointer on the current HIP device; `stream` is a hipStream_t
 *     passed as void* (NULL = default stream).  Nothing here allocates, frees, copies to the
 *     host or synchronises: calls only enqueue work (graph-capture safe).  Scratch comes from
 *     the caller through (ws, ws_bytes); query the size with the *_workspace_bytes functions.
 *   - return value: 0 on success, non-zero on error; cstp_last_error() returns a message for
 *     the calling thread.
 *   - PROCESS-GLOBAL mutable state behind this interface (all of it; none is per stream or per call):
 *       * the thread-local error string;
 *       * the mutex-guarded table of tuned tile shapes (cstp_conv3d_autotune / cstp_conv3d_set_tile write it, every
 *         convolution call reads it);
 *       * the GEMM arithmetic selector cstp_gemm_set_split_terms (atomic; 0 = the CSTP_GEMM environment default) -- it picks
 *         the kernel family of EVERY later convolution / linear call of the process, on any stream, and is part of the tile
 *         table's key;
 *       * the deterministic-mode switch cstp_set_deterministic (atomic; ordered slabs instead of float atomics in the weight
 *         gradients), likewise process-wide;
 *       * the per-thread pack mode and record list (cstp_pack_mode), the process-wide set of registered workspaces
 *         (cstp_pack_register) and the records last drained for each (cstp_pack_recorded; both mutex-guarded);
 *       * environment knobs read once: CSTP_GEMM, CSTP_DETERMINISTIC, CSTP_PERSIST_CUS, CSTP_TILE / CSTP_WTILE (developer
 *         overrides).
 *     A caller that wants two arithmetics side by side in one process must serialise the switch with its launches
 *     (bench.py does, between timed loops); results never depend on the state of another STREAM.
 */
#ifndef CSTP_HIP_H
#define CSTP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSTP_ABI_VERSION 18

/* Geometry of one nn.Conv3d(bias=False) call-site.
 * models/pace/r21d_byol.py:81-82 (spatial 1xkxk), :91-92 (temporal tx1x1), :125 (1x1x1 shortcut);
 * nn.Linear (r21d_byol.py:235-241, 249-255, 276-291) is the D=H=W=1, k=1 case. */
typedef struct cstp_conv_desc {
  int32_t n, c, d, h, w; /* input  [n][c][d][h][w]            */
  int32_t k;             /* output channels                    */
  int32_t kt, kh, kw;    /* kernel                             */
  int32_t st, sh, sw;    /* stride                             */
  int32_t pt, ph, pw;    /* zero padding                       */
} cstp_conv_desc;

/* Optional input transform fused into a convolution's gather: z = act(x * scale + shift) with one
 * (scale, shift) pair per (BN group, input channel) -- the train-mode BatchNorm (+ReLU) that precedes the
 * convolution in the reference (r21d_byol.py:94-97 `temporal_conv(relu(bn(spatial_conv(x))))`, :142-143
 * `conv2(relu1(bn1(.)))`) applied on the fly, so the normalised tensor is never written to HBM.
 * scale_shift: float[groups][c][2] as produced by cstp_bn_stats_train; zero padding applies to z. */
typedef struct cstp_in_affine {
  const float* scale_shift;
  int32_t groups; /* 1..4, must divide desc->n */
  int32_t relu;   /* non-zero: z = max(z, 0) */
} cstp_in_affine;

/* 1 when BOTH the forward and the weight gradient of this geometry apply a cstp_in_affine over `groups` BatchNorm groups inside
 * their f16-pair gather kernels (igemm_k1s / igemm_k2s <.., AFF>) given the transformed tensor's absmax cell; 0 = such a call
 * would fall back to the native fp32 kernels (correct, much slower): callers then materialise the BatchNorm output instead. */
int32_t cstp_conv3d_in_affine_fused(const cstp_conv_desc* desc, int32_t groups);

int cstp_abi_version(void);
const char* cstp_last_error(void);

/* ---- convolution (F.conv3d / F.linear and their autograd) ------------------------------- */
/* (F.linear is the D = H = W = 1, 1x1x1 case.  On n <= 32 rows -- the heads, r21d_byol.py:159-176, 318-334 -- forward, data gradient
 *  (reduction length a multiple of 64) and weight gradient run as weight-streaming kernels in EXACT fp32 FMAs, slices summed in a
 *  fixed order (csrc/linear.h); the native-f32 arithmetic and a pinned tile keep them on the convolution kernels.) */
size_t cstp_conv3d_workspace_bytes(const cstp_conv_desc* desc);
/* y[n][k][do][ho][wo] = conv3d(T(x), w) (+ bias[k] when bias != NULL).  w is [k][c][kt][kh][kw].
 * T = identity when in_affine == NULL, else the fused BN(+ReLU) input transform above.  (The _am variants: with an in_affine the
 * absmax cell is that of T(x), cstp_bn_finalize_pre.) */
int cstp_conv3d_forward(void* stream, const cstp_conv_desc* desc, const float* x, const float* w,
                        const float* bias, const cstp_in_affine* in_affine, float* y, void* ws, size_t ws_bytes);
/* dx = conv3d input gradient (aten::convolution_backward, input mask). */
int cstp_conv3d_backward_data(void* stream, const cstp_conv_desc* desc, const float* dy, const float* w,
                              float* dx, void* ws, size_t ws_bytes);
/* dw = conv3d weight gradient w.r.t. T(x), [k][c][kt][kh][kw] (aten::convolution_backward, weight mask);
 * in_affine as in the forward call (NULL = identity). */
int cstp_conv3d_backward_weight(void* stream, const cstp_conv_desc* desc, const float* x,
                                const cstp_in_affine* in_affine, const float* dy, float* dw, void* ws,
                                size_t ws_bytes);

/* The same three calls with the LARGEST MAGNITUDE of the gathered activation operand(s) supplied by the caller: each
 * *_absmax points to one device uint32 holding the fp32 bit pattern (sign cleared) of max |element| of that tensor -- exactly
 * what cstp_bn_forward_train_am / cstp_bn_backward_am leave behind for the tensor they write.  The 2xf16-split kernels
 * (csrc/igemm_split.h: operands scaled by a power of two into f16 range and split into an f16 pair, three f16 MFMA
 * products per fp32 product) need it for their operand scale; with NULL they measure it themselves with one extra read of
 * the tensor.  Every other kernel variant ignores it.  The value must not be smaller than the true maximum (f16 overflow);
 * a larger value costs one bit of the 22-bit operand precision per factor of two. */
int cstp_conv3d_forward_am(void* stream, const cstp_conv_desc* desc, const float* x, const float* w, const float* bias,
                           const cstp_in_affine* in_affine, float* y, void* ws, size_t ws_bytes, const uint32_t* x_absmax);
/* Forward of a bias-free convolution whose output feeds a train-mode BatchNorm3d over `groups` (1 or 2) equal slices of the batch
 * (r21d_byol.py:82-83: spatial_conv -> bn): where the layer runs the LDS-resident-patch kernel, the launch also leaves the
 * per-channel, per-group sums of y and y^2 as fp64 partials part[k][groups][nsplit][2] (cstp_bn_forward_train_pre folds
 * them: the BatchNorm then needs no statistics pass over y).  *nsplit = partials per (channel, group), or 0 when this layer's
 * kernel cannot deliver them -- the call is then exactly cstp_conv3d_forward_am and BatchNorm takes its usual path.
 * cstp_conv3d_bnstats_nsplit: the same answer in advance (part needs k * groups * nsplit * 3 + k doubles).
 * pivot (float[k] on the device, or NULL = zeros): the sums are taken AROUND it -- sum(y - pivot[ch]), sum((y - pivot[ch])^2) --
 * and the launch stores the values it used in the k doubles behind the sums; any finite values are correct, values near the
 * channel means (the BatchNorm's running_mean) keep the variance free of cancellation when |mean| >> std.
 * Behind the pivots the launch leaves every channel's smallest and largest output per group and partial
 * (uint32 keys [k][groups][nsplit][2]): cstp_bn_finalize_pre turns them into the exact largest magnitude of the normalised
 * tensor, so that the convolution consuming it can apply the BatchNorm in its own gather (cstp_in_affine) with the tensor
 * never written.  z_cell (device uint32, or NULL): zeroed by this launch for that purpose (cstp_bn_finalize_pre takes the
 * maximum into it with atomics).  in_affine (or NULL): the input transform of cstp_conv3d_forward_am, for a temporal
 * convolution that consumes one BatchNorm inside its gather and feeds the next (x_absmax is then that of T(x)). */
int32_t cstp_conv3d_bnstats_nsplit(const cstp_conv_desc* desc, int32_t groups);
/* ... the answer for a call that carries an in_affine (such a forward may run another kernel variant than the plain one:
 * the weight-resident temporal kernel igemm_k1w where it applies, csrc/igemm_twres.h). */
int32_t cstp_conv3d_bnstats_nsplit_aff(const cstp_conv_desc* desc, int32_t groups);
int cstp_conv3d_forward_bnstats(void* stream, const cstp_conv_desc* desc, const float* x, const float* w, float* y, void* ws,
                                size_t ws_bytes, const uint32_t* x_absmax, int32_t groups, const float* pivot, double* part,
                                size_t part_bytes, int32_t* nsplit, uint32_t* z_cell, const cstp_in_affine* in_affine);
int cstp_conv3d_backward_data_am(void* stream, const cstp_conv_desc* desc, const float* dy, const float* w, float* dx,
                                 void* ws, size_t ws_bytes, const uint32_t* dy_absmax);
/* ... and with accumulate != 0: dx += the data gradient instead of dx = -- autograd's sum of the gradients of a tensor that
 * feeds two consumers (the residual connection, r21d_byol.py:141-148: x goes into conv1 AND into the addition behind bn2),
 * folded into the convolution's epilogue: one extra read of dx instead of a separate three-tensor add pass. */
int cstp_conv3d_backward_data_acc(void* stream, const cstp_conv_desc* desc, const float* dy, const float* w, float* dx,
                                  void* ws, size_t ws_bytes, const uint32_t* dy_absmax, int32_t accumulate);
int cstp_conv3d_backward_weight_am(void* stream, const cstp_conv_desc* desc, const float* x, const cstp_in_affine* in_affine,
                                   const float* dy, float* dw, void* ws, size_t ws_bytes, const uint32_t* x_absmax,
                                   const uint32_t* dy_absmax);
/* ... and with accumulate != 0: dw += the weight gradient instead of dw = -- autograd's AccumulateGrad (`.grad += `,
 * main_byol.py:87 loss.backward()) folded into the unpacking pass, for a `.grad` that lives in the flat gradient arena. */
int cstp_conv3d_backward_weight_acc(void* stream, const cstp_conv_desc* desc, const float* x, const cstp_in_affine* in_affine,
                                    const float* dy, float* dw, void* ws, size_t ws_bytes, const uint32_t* x_absmax,
                                    const uint32_t* dy_absmax, int32_t accumulate);

/* Deterministic mode, process-wide (also CSTP_DETERMINISTIC=1 in the environment): the weight-gradient kernels reduce their
 * split-K partial sums through per-split slabs added in a fixed order instead of f32 atomics, so two runs on the same
 * inputs give bit-identical gradients (slower; for debugging -- the default's summation order varies from run to run, rel 1e-6).
 * Switch it BEFORE sizing workspaces: cstp_conv3d_workspace_bytes grows by the slab count. */
int cstp_set_deterministic(int32_t on);
int32_t cstp_get_deterministic(void);

/* Arithmetic of the split kernels (csrc/igemm_split.h), process-wide: 2 = every fp32 operand scaled by a power of two and
 * split into an f16 PAIR, three f16 MFMA products per fp32 product (default; 22 operand bits, measured at least as close to
 * fp64 as the native f32 MFMA chain); 3 = split EXACTLY into a bf16 TRIPLE, six bf16 MFMA products (no operand scaling, no
 * dynamic-range caveat; also selected by CSTP_GEMM=bf16x3 in the environment); 1 = no split kernels at all: every GEMM-shaped
 * op on the native f32 MFMA (bit-for-bit an fmaf chain; also CSTP_GEMM=f32), with its own class of tuned tiles;
 * 0 = back to the environment's choice.  All accumulate in f32.  cstp_gemm_get_split_terms returns 1, 2 or 3. */
int cstp_gemm_set_split_terms(int32_t terms);
int32_t cstp_gemm_get_split_terms(void);

/* The weight packs of a whole network pass from ONE launch.  Every convolution / linear call re-lays its weights out for the
 * kernel variant it runs (a launch of ~10 us per call: ~137 per R(2+1)D-18 training step, main_byol.py:60-91 being ONE Python
 * step).  A caller that keeps a PERSISTENT workspace per (weight tensor, direction) can hoist them:
 *   cstp_pack_mode(1); <the call>; cstp_pack_mode(0);  n = cstp_pack_recorded(recs, cap);     -- once: what the call packs
 *   cstp_pack_replay(stream, recs_dev, first_block_dev, n, total_blocks);                     -- per pass: all recorded packs
 *   cstp_pack_mode(2); <the same call, same pointers>; cstp_pack_mode(0);                     -- the call skips its pack
 * A record is the pack launch itself (kind 1: f16-pair split rows, 2: LDS-patch K-tiles, 3: native fp32 re-layout, 4: the
 * bf16-storage path's operand rows; pointers,
 * integer arguments, blocks of 256 threads), so the replay does exactly what the call would have done -- provided descriptor,
 * tile table, weight pointer and workspace pointer are those of the recorded call.  first_block_dev[i] = sum of nblocks of the
 * records before i; total_blocks = the sum over all.  The mode is per calling THREAD (0 = default).  Mode 2 is an unchecked
 * promise (for tests).  bf16-triple packs are not recorded (they keep packing inside the call in every mode). */
typedef struct cstp_pack_rec {
  int32_t kind, nblocks;
  const float* w;
  void* dst;
  float* inv_a;
  uint32_t* cells;
  int32_t a[10];
} cstp_pack_rec;
int cstp_pack_mode(int32_t mode);
int32_t cstp_pack_recorded(cstp_pack_rec* out, int32_t cap);
int cstp_pack_replay(void* stream, const cstp_pack_rec* recs_dev, const int32_t* first_block_dev, int32_t n, int32_t total_blocks);
/* ... or, instead of mode 2 around every call: REGISTER the workspaces (the records' dst pointers) whose packs the caller replays --
 * a call that receives a registered workspace skips its pack ONLY IF the pack it would launch equals a record that
 * cstp_pack_recorded handed out for that workspace (kind, nblocks, w, inv_a, cells, a[]; each drain replaces the records an
 * earlier one left for the same workspaces).  Any other pack -- another kernel variant (operand alignment, an absmax cell or
 * not, a tile or arithmetic changed since the recording), another weight tensor, a workspace without a record -- runs inside
 * the call, and that workspace stops counting as registered until it is registered again; so does a workspace that a call
 * uses for something other than a recorded pack (a bf16-triple pack, a linear layer's partial sums).  on = 0: unregister;
 * n = 0 with on = 0: forget all registrations and records.  Process-wide. */
int cstp_pack_register(const void* const* workspaces, int32_t n, int32_t on);

/* Which kernel variant the next forward (mode 0) / backward_data (mode 1) / backward_weight (mode 2) call with this
 * descriptor will run: out[0] = rows per block tile, out[1] = positions (mode 2: (tap, channel) columns) per block tile,
 * out[2] = 0 for the native f32 MFMA kernel, else the number of terms each operand is split into by the split kernel (2 or
 * 3, see cstp_gemm_set_split_terms), out[3] = K-tiles per barrier (mode 2: split-K block target / 256).  mode 3 = a forward
 * call that carries an in_affine (it may run another variant than the plain forward: cstp_conv3d_bnstats_nsplit_aff).
 * Reporting only (bench.py names the kernels and picks their roofline peaks with it). */
int cstp_conv3d_query_tile(const cstp_conv_desc* desc, int32_t mode, int32_t* out4);

/* The TUNED entry of one geometry and direction in cstp_conv3d_set_tile's encoding (tile4[0] = -1 when the geometry has
 * not been tuned or pinned in the current arithmetic class): lets the host persist a tuning table and replay it with
 * cstp_conv3d_set_tile, so that every rank and every run executes the same kernels (cstp_amd/tuned/). */
int cstp_conv3d_get_tile(const cstp_conv_desc* desc, int32_t mode, int32_t* tile4);

/* Pin the kernel variant of one geometry and direction (what cstp_conv3d_autotune would otherwise decide by timing):
 * mode 0 forward / 1 backward_data: tile[0] = 1 for the split kernel (arithmetic: cstp_gemm_set_split_terms; tile[1] = row tiles of 16: 2,3,4,5,6,8,9;
 * tile[2] = 2 selects the 256-column tile, available with 8 / 9 row tiles) or 0
 * for the native f32 kernel (tile[1] = row tiles of 32: 1..5, or 9 = the 144-row tile of nine 16-row MFMA tiles, tile[2] = waves
 * along rows 1|2|4, tile[3] = K-tiles per barrier 1|2); mode 2 backward_weight: tile[0] = 1 split (tile[1] = 4|8|9 row tiles of 16) or 0 native (tile[1] = 1..5 row tiles of
 * 32, or 9 = the 144-row tile), tile[2] = split-K block target / 256 (4, 8, 16).  Inadmissible requests (3-channel stem, > 27
 * taps, >= 2 GiB tensors for the split kernels) fall back to a native tile at call time.  Used by the parity tests to put every
 * kernel variant against the fp64 reference regardless of which one is fastest on the machine at hand. */
int cstp_conv3d_set_tile(const cstp_conv_desc* desc, int32_t mode, const int32_t* tile4);

/* Optional one-off tuning, OUTSIDE graph capture: times the tile shapes of the forward (mode 0: src = x, w = weights,
 * out = y), data-gradient (mode 1: src = dy, w = weights, out = dx) or weight-gradient (mode 2: src = x, w = dy,
 * out = dw; row-tile height x split-K block count) kernel for this geometry on `stream` (this call DOES synchronise)
 * and remembers the fastest in a process-wide table that later calls with the same descriptor consult.  The native
 * f32 tiles give bit-identical results among themselves; the split tiles (candidates unless the environment says
 * CSTP_GEMM=f32) differ from them in the last bits (both sit ~4e-7 rms from the fp64 result per convolution,
 * tools/split_accuracy.py).  Without tuning an analytic native-f32 choice is used.  `out` is overwritten. */
int cstp_conv3d_autotune(void* stream, const cstp_conv_desc* desc, int32_t mode, const float* src, const float* w,
                         float* out, void* ws, size_t ws_bytes, int32_t iters);

/* ---- BatchNorm3d / BatchNorm1d in TRAIN mode, fused with the residual add and ReLU that follow
 *      it (r21d_byol.py:83-84,133-134,138-139,148,199-200,216; Projector/Predictor/heads BN1d).
 *      x,y,residual: [n][c][s] (s = D*H*W).  y = act(bn(x) + residual), act = relu if relu != 0.
 *      `groups`: the batch holds that many independent BN calls back to back (n = groups * n_per_group,
 *      e.g. the two views of a clip pair, r21d_byol.py:359-360): statistics are per (group, channel),
 *      running stats are updated group after group as successive F.batch_norm(training=True) calls would.
 *      save_mean/save_invstd: [groups][c] outputs for backward.  running_mean/var updated in place with
 *      `momentum` (unbiased variance).  scale_shift (optional, s > 1): float[groups][c][2] affine form of the
 *      normalisation; handing it to cstp_bn_backward lets the ReLU mask be recomputed from x instead of
 *      re-reading y (two fewer HBM passes in the backward). */
size_t cstp_bn_workspace_bytes(int32_t n, int32_t c, int32_t s, int32_t groups);
int cstp_bn_forward_train(void* stream, const float* x, const float* residual, float* y, const float* gamma,
                          const float* beta, float* running_mean, float* running_var, float* save_mean,
                          float* save_invstd, float* scale_shift, int32_t n, int32_t c, int32_t s, int32_t groups,
                          float eps, float momentum, int32_t relu, void* ws, size_t ws_bytes);
/* ... and, as a by-product of the pass that writes y (s > 1 only), the largest magnitude of y into *y_absmax (fp32 bits,
 * sign cleared; NULL = not wanted) for the consumer convolution (cstp_conv3d_forward_am / _backward_weight_am). */
int cstp_bn_forward_train_am(void* stream, const float* x, const float* residual, float* y, const float* gamma,
                             const float* beta, float* running_mean, float* running_var, float* save_mean,
                             float* save_invstd, float* scale_shift, int32_t n, int32_t c, int32_t s, int32_t groups,
                             float eps, float momentum, int32_t relu, void* ws, size_t ws_bytes, uint32_t* y_absmax);
/* ... with the statistics pass replaced by the partial sums a producing convolution left (cstp_conv3d_forward_bnstats;
 * part[c][groups][nsplit][2] fp64 sums of (x - pivot) and (x - pivot)^2, then pivot[c]; s > 1).  Everything else as
 * cstp_bn_forward_train_am. */
int cstp_bn_forward_train_pre(void* stream, const float* x, const float* residual, float* y, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float* save_mean,
                              float* save_invstd, float* scale_shift, int32_t n, int32_t c, int32_t s, int32_t groups,
                              float eps, float momentum, int32_t relu, void* ws, size_t ws_bytes, uint32_t* y_absmax,
                              const double* part, int32_t nsplit);
/* The finalize step of cstp_bn_forward_train_pre ALONE (no pass over x, no output tensor): save_mean / save_invstd, the running
 * statistics, the affine table scale_shift[groups][c][2] and -- from the minima / maxima cstp_conv3d_forward_bnstats left behind
 * its sums -- the largest magnitude of act(x * scale + shift) over the whole tensor, bit-identical to what the apply pass of
 * cstp_bn_forward_train_pre would have measured, taken into *z_cell with atomicMax (the cell must hold 0 or a lower bound: the
 * producing launch zeroes the one it was given).  count = n * s / groups values per channel and group. */
int cstp_bn_finalize_pre(void* stream, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         float* save_mean, float* save_invstd, float* scale_shift, int32_t n, int32_t c, int32_t s,
                         int32_t groups, float eps, float momentum, int32_t relu, const double* part, int32_t nsplit,
                         uint32_t* z_cell);
/* Statistics only: save_mean/save_invstd [groups][c], running stats update, and the affine table
 * scale_shift float[groups][c][2] = (invstd*gamma, beta - mean*invstd*gamma) that a consumer convolution
 * applies in its gather (cstp_in_affine) -- the BN output itself is never materialised. */
int cstp_bn_stats_train(void* stream, const float* x, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, float* save_mean, float* save_invstd, float* scale_shift, int32_t n,
                        int32_t c, int32_t s, int32_t groups, float eps, float momentum, void* ws, size_t ws_bytes);
/* Backward of the fused op.  y is the forward OUTPUT (its sign is the ReLU mask); when the output was
 * never materialised (cstp_bn_stats_train + cstp_in_affine) pass y = NULL and the scale_shift table and the
 * mask is recomputed from x.  dresidual may be NULL.  dgamma/dbeta: [c], summed over the groups.
 * s > 1 only: a BatchNorm1d backward (s = 1) is REFUSED with an error that names cstp_bn1d_backward, here and in
 * cstp_bn_backward_am.  The fp32 forms these entries once ran for s = 1 missed the project's tolerance on few rows per group
 * (see cstp_bn1d_backward); an entry that says where to go is better than one that silently answers outside it. */
int cstp_bn_backward(void* stream, const float* x, const float* y, const float* dy, const float* gamma,
                     const float* save_mean, const float* save_invstd, const float* scale_shift, float* dx,
                     float* dresidual, float* dgamma, float* dbeta, int32_t n, int32_t c, int32_t s, int32_t groups,
                     int32_t relu, void* ws, size_t ws_bytes);

/* ... with the largest magnitude of dx as a by-product (the dY operand of the producing convolution's data / weight
 * gradient, cstp_conv3d_backward_data_am / _backward_weight_am); s > 1 only, NULL = not wanted.  accumulate != 0: dgamma and
 * dbeta are ADDED to the buffers (the parameters' gradient slices of a flat arena: no separate accumulation kernel). */
int cstp_bn_backward_am(void* stream, const float* x, const float* y, const float* dy, const float* gamma,
                        const float* save_mean, const float* save_invstd, const float* scale_shift, float* dx,
                        float* dresidual, float* dgamma, float* dbeta, int32_t n, int32_t c, int32_t s, int32_t groups,
                        int32_t relu, void* ws, size_t ws_bytes, uint32_t* dx_absmax, int32_t accumulate);

/* BatchNorm1d (x [n][c], s = 1) backward with the batch statistics REBUILT from x and eps in fp64 and dx formed in fp64: with
 * few rows per group dx is eps / (var + eps) of the size of the terms it is the difference of (two rows: exactly that, in
 * every feature), which an fp32 invstd cannot carry.  No saved statistics, no workspace; y (the forward output) is needed only
 * with relu; dresidual may be NULL; accumulate as in cstp_bn_backward_am.  The only backward for s = 1: cstp_bn_backward[_am]
 * refuse it. */
int cstp_bn1d_backward(void* stream, const float* x, const float* y, const float* dy, const float* gamma, float* dx,
                       float* dresidual, float* dgamma, float* dbeta, int32_t n, int32_t c, int32_t groups, float eps,
                       int32_t relu, int32_t accumulate);

/* EVAL mode (model.eval(): main_ft_mp.py:254-262 validation, test.py:74-76): the running statistics are the
 * statistics -- y = act((x - running_mean) / sqrt(running_var + eps) * gamma + beta + residual); nothing is updated.
 * Forward only (the reference evaluates under torch.no_grad()).  ws: cstp_bn_eval_workspace_bytes(c) when s > 1. */
size_t cstp_bn_eval_workspace_bytes(int32_t c);
int cstp_bn_forward_eval(void* stream, const float* x, const float* residual, float* y, const float* gamma,
                         const float* beta, const float* running_mean, const float* running_var, int32_t n, int32_t c,
                         int32_t s, float eps, int32_t relu, void* ws, size_t ws_bytes);
/* ... with max |y| as a by-product (s > 1; see cstp_bn_forward_train_am); ws then is cstp_bn_workspace_bytes(n, c, s, 1). */
int cstp_bn_forward_eval_am(void* stream, const float* x, const float* residual, float* y, const float* gamma,
                            const float* beta, const float* running_mean, const float* running_var, int32_t n, int32_t c,
                            int32_t s, float eps, int32_t relu, void* ws, size_t ws_bytes, uint32_t* y_absmax);

/* ---- AdaptiveAvgPool3d(1) (r21d_byol.py:210,222-223) and its backward ------------------- */
int cstp_avgpool_forward(void* stream, const float* x, float* y, int32_t rows, int32_t s);
int cstp_avgpool_backward(void* stream, const float* dy, float* dx, int32_t rows, int32_t s);
/* nn.MaxPool3d (models/BE/r3d_byol.py:158,197: kernel 3, stride 2, padding 1 after the stem of the 3D-ResNet backbone; any
 * kernel / stride / padding with 2*pad <= kernel here).  x: [rows = n*c][d][h][w] -> y: [rows][do][ho][wo]; argmax (int32,
 * same shape as y) records the flat in-plane index of the first maximum in (d, h, w) scan order, as aten's kernel keeps it.
 * backward gathers: dx[p] = sum of dy over the windows whose argmax is p (deterministic, no atomics). */
int cstp_maxpool3d_forward(void* stream, const float* x, float* y, int32_t* argmax, int32_t rows, int32_t d, int32_t h,
                           int32_t w, const int32_t* kernel3, const int32_t* stride3, const int32_t* pad3);
int cstp_maxpool3d_backward(void* stream, const float* dy, const int32_t* argmax, float* dx, int32_t rows, int32_t d,
                            int32_t h, int32_t w, const int32_t* kernel3, const int32_t* stride3, const int32_t* pad3);
/* out[c] = sum over n,s of x[n][c][s]  (bias gradient of nn.Linear). */
int cstp_channel_sum(void* stream, const float* x, float* out, int32_t n, int32_t c, int32_t s, void* ws,
                     size_t ws_bytes);

/* ---- loss heads ------------------------------------------------------------------------- */
/* BYOL regression loss r21d_byol.py:346-349: loss[b] = 2 - 2*<x/|x|, y/|y|>, eps 1e-12; x,y [b][f].
 * backward writes dx only (the target branch is detached, r21d_byol.py:368-369). */
int cstp_byol_loss_forward(void* stream, const float* x, const float* y, float* loss, int32_t b, int32_t f);
int cstp_byol_loss_backward(void* stream, const float* x, const float* y, const float* dloss, float* dx,
                            int32_t b, int32_t f);
/* F.normalize(x, p=2, dim=1) of the fine-tune/test head (r21d_byol.py:396): y = x / max(|x|_2, eps), x,y [rows][f];
 * norm[rows] = max(|x|, eps) is kept for the backward: dx = (dy - y <y, dy>) / norm. */
int cstp_l2_normalize_forward(void* stream, const float* x, float* y, float* norm, int32_t rows, int32_t f, float eps);
int cstp_l2_normalize_backward(void* stream, const float* y, const float* norm, const float* dy, float* dx, int32_t rows,
                               int32_t f, float eps);
/* nn.CrossEntropyLoss() (mean) main_byol.py:63-68: logits [b][k], labels int64 [b] -> loss[1].
 * backward: dlogits = dloss[0] * (softmax - onehot) / b. */
int cstp_cross_entropy_forward(void* stream, const float* logits, const int64_t* labels, float* loss, int32_t b,
                               int32_t k);
int cstp_cross_entropy_backward(void* stream, const float* logits, const int64_t* labels, const float* dloss,
                                float* dlogits, int32_t b, int32_t k);
/* Soft-target cross-entropy (mean) for fine-tuning with label smoothing and mixup / CutMix: per row two targets ta[b], tb[b]
 * (int64, device), a weight lam[b] (fp32, device) and one host scalar eps in [0, 1):
 *   q[r][c] = (1-eps)*(lam[r]*[c==ta[r]] + (1-lam[r])*[c==tb[r]]) + eps/k
 *   loss[0] = mean_r -sum_c q[r][c]*log_softmax(logits[r])[c]           (= F.cross_entropy(logits, q); with lam = 1 it is
 *                                                                          F.cross_entropy(logits, ta, label_smoothing=eps))
 *   backward: dlogits = dloss[0] * (softmax - q) / b.
 * tb == NULL means tb = ta and lam == NULL means lam = 1 (smoothing only).  A target outside [0, k) contributes no one-hot mass
 * and is never used as an index (the backward stays the gradient of that loss: softmax is weighted by the row's sum of q).  One wave per row with the lanes along k, the batch mean accumulated in double, fixed-order
 * reductions and no atomics: equal inputs give equal bits.  b*k < 2^31; dlogits must not alias logits. */
int cstp_soft_cross_entropy_forward(void* stream, const float* logits, const int64_t* ta, const int64_t* tb, const float* lam,
                                    float eps, float* loss, int32_t b, int32_t k);
int cstp_soft_cross_entropy_backward(void* stream, const float* logits, const int64_t* ta, const int64_t* tb, const float* lam,
                                     float eps, const float* dloss, float* dlogits, int32_t b, int32_t k);
/* NT-Xent loss/NTXent.py:46-62 on reps = cat(zjs, zis) [2n][f] (cosine similarity, eps 1e-8).
 * forward needs ws of cstp_ntxent_workspace_bytes (the 2n x 2n similarity matrix + norms);
 * backward reuses that ws and writes dreps [2n][f]. */
size_t cstp_ntxent_workspace_bytes(int32_t two_n, int32_t f);
int cstp_ntxent_forward(void* stream, const float* reps, float* loss, int32_t two_n, int32_t f, float temperature,
                        void* ws, size_t ws_bytes);
int cstp_ntxent_backward(void* stream, const float* reps, const float* dloss, float* dreps, int32_t two_n,
                         int32_t f, float temperature, void* ws, size_t ws_bytes);

/* ---- GPU clip assembly (data path next to the step: data_process/datasets.py:876-948, preprocess_data.py:479-581,1103-1110) ----
 * frames: decoded video, uint8 [f][h][w][3] in HBM.  For each of the t frames frame_idx[i] (device int32): Image.transpose(rot in
 * {0, 90, 180, 270}, counter-clockwise) -> Image.crop at (box_x0, box_y0) of the ROTATED frame -> Image.resize((size, size),
 * Image.BICUBIC) -> FLIP_LEFT_RIGHT if flip -> ToTensor -> x*2-1 clamped  =>  out fp32 [3][t][size][size].
 * The resize is Pillow's fixed-point algorithm bit for bit; its integer coefficient tables come from the caller (kh/kv int32
 * [size][ks*], bh/bv int32 [size][2] = (first tap, tap count), computed as Resample.c's precompute_coeffs +
 * normalize_coeffs_8bpc do for the crop's width / height -- cstp_amd/clip_ops.py); the horizontal pass covers the crop rows
 * [row_first, row_first + rows) that the vertical pass reads and writes them to tmp (uint8 [t][rows][size][3]). */
int cstp_clip_assemble(void* stream, const uint8_t* frames, int32_t f, int32_t h, int32_t w, const int32_t* frame_idx, int32_t t,
                       int32_t rot, int32_t box_x0, int32_t box_y0, int32_t size, int32_t flip, const int32_t* kh,
                       const int32_t* bh, int32_t ksh, const int32_t* kv, const int32_t* bv, int32_t ksv, int32_t row_first,
                       int32_t rows, uint8_t* tmp, float* out);

/* ... the same up to the resize, result kept as 8-bit RGB [t][size][size][3] (no flip, no normalisation): the input of the
 * base_transform operations below. */
int cstp_clip_assemble_u8(void* stream, const uint8_t* frames, int32_t f, int32_t h, int32_t w, const int32_t* frame_idx,
                          int32_t t, int32_t rot, int32_t box_x0, int32_t box_y0, int32_t size, const int32_t* kh,
                          const int32_t* bh, int32_t ksh, const int32_t* kv, const int32_t* bv, int32_t ksv, int32_t row_first,
                          int32_t rows, uint8_t* tmp, uint8_t* out);
/* ---- the `base_transform` branch of the clip pipeline (data_process/preprocess_data.py:1110-1121; taken with p = 0.3 per clip,
 * TwoClipTransform :713-741) on 8-bit RGB clips [t][h][w][3] in HBM.  Each entry reproduces, bit for bit, the Pillow call the
 * reference makes (directly, or through torchvision's PIL backend):
 *   cstp_clip_rotate    RandomRotation(10) :1060-1100 -> Image.rotate(angle): NEAREST, same size, black fill.  coef6 (HOST
 *                       pointer) = Geometry.c affine_fixed's six 16.16 fixed-point coefficients of Image.rotate's reverse matrix.
 *   cstp_clip_blend     ClipColorJitter :584-672 -> adjust_brightness (mode 0), adjust_contrast (1; ws_means: t int32 on the
 *                       device), adjust_saturation (2) = ImageEnhance.{Brightness, Contrast, Color}.enhance(alpha) = Image.blend.
 *   cstp_clip_hue       adjust_hue: RGB -> HSV, h += shift (= uint8(hue_factor * 255)) modulo 256, HSV -> RGB; mode 1 / 2: the
 *                       RGB -> HSV / HSV -> RGB conversion alone.  In place allowed.
 *   cstp_clip_gray      ClipRandomGray.grayscale :704-709: frame i keeps channel[i] (device int32, < 0 = unchanged) in all three.
 *   cstp_clip_box_blur  ClipGaussianBlur :675-687 -> ImageFilter.GaussianBlur(radius) = `passes` (3) extended box blurs per axis
 *                       (BoxBlur.c); radius / ww / fw = integer box radius and its two 24-bit fixed-point weights, computed by
 *                       the caller as BoxBlur.c does from the float box radius.  In place (tmp: same size scratch).
 *   cstp_clip_finish    [FLIP_LEFT_RIGHT] -> ToTensor -> x * 2 - 1 clamped: uint8 [t][h][w][3] -> fp32 [3][t][h][w]. */
int cstp_clip_rotate(void* stream, const uint8_t* src, uint8_t* dst, int32_t t, int32_t h, int32_t w, const int32_t* coef6);
int cstp_clip_blend(void* stream, const uint8_t* src, uint8_t* dst, int32_t t, int32_t h, int32_t w, int32_t mode, float alpha,
                    int32_t* ws_means);
int cstp_clip_hue(void* stream, const uint8_t* src, uint8_t* dst, size_t npix, int32_t shift, int32_t mode);
int cstp_clip_gray(void* stream, const uint8_t* src, uint8_t* dst, int32_t t, int32_t h, int32_t w, const int32_t* channel);
int cstp_clip_box_blur(void* stream, uint8_t* img, uint8_t* tmp, int32_t t, int32_t h, int32_t w, int32_t radius, uint32_t ww,
                       uint32_t fw, int32_t passes);
int cstp_clip_finish(void* stream, const uint8_t* src, float* out, int32_t t, int32_t h, int32_t w, int32_t flip);

/* ---- batched, descriptor-driven clip assembly: the fine-tune / validation / video-test data path (reference
 * data_process/datasets.py:952-1097 UcfFineTune + preprocess_data.py:1131-1149 'img' / 'img_val' / 'img_test') and any other
 * batch of crop -> BICUBIC resize -> window clips.  One call serves n clips that may come from different videos of different
 * frame sizes, in TWO launches (horizontal pass, vertical pass) whatever n is.  Per clip: the crop box at (box_x0, box_y0) of
 * its frames is resized to rw x rh with the caller's coefficient tables (kh / bh of rw entries, kv / bv of rh entries, as
 * cstp_clip_assemble takes them); only the size x size window at (win_x, win_y) of the resized image is computed, and of the
 * horizontal pass only the box rows [row_first, row_first + rows) which that window's vertical taps read -- each output pixel
 * depends on its own taps alone, so the result equals resize-then-crop bit for bit.  Arithmetic as cstp_clip_assemble
 * (Pillow's 22-bit fixed point, uint8 intermediate, zeros beyond the frame).  A clip may carry a rotation by a multiple of 90
 * degrees (the pre-training pairs, datasets.py:876-948), folded into the source indexing of the horizontal pass exactly as
 * cstp_clip_assemble folds it. */
typedef struct cstp_clip_batch_desc {
  const uint8_t* frames;   /* this clip's video: uint8 [f][h][w][3] */
  const int32_t* kh;       /* horizontal coefficients [rw][ksh] */
  const int32_t* bh;       /* horizontal bounds [rw][2] = (first tap, tap count), relative to the box */
  const int32_t* kv;       /* vertical coefficients [rh][ksv] */
  const int32_t* bv;       /* vertical bounds [rh][2] */
  int64_t tmp_off;         /* this clip's offset (in PIXELS) into the ragged tmp buffer: uint8 [t][rows][size][3] */
  int32_t f, h, w;         /* its video's frame count and frame size */
  int32_t idx_off;         /* its t frame indices start here in the shared frame-index array */
  int32_t box_x0, box_y0;  /* source box origin in the frame (the box may reach past the frame: zeros) */
  int32_t ksh, ksv;
  int32_t rw, rh;          /* size of the resized image */
  int32_t win_x, win_y;    /* output window origin inside the resized image */
  int32_t row_first, rows; /* box rows the horizontal pass covers */
  int32_t flip;            /* FLIP_LEFT_RIGHT folded into the fp32 store (ignored for an 8-bit output) */
  int32_t out_slot;        /* clip index in out (fp32 [slots][3][t][size][size]), or -1 */
  int32_t out8_slot;       /* clip index in out8 (uint8 [slots8][t][size][size][3], no flip, no normalisation), or -1 */
  int32_t rot;             /* 0 / 90 / 180 / 270: Image.transpose(ROTATE_*) of the whole frame before the crop; box_x0 / box_y0 and
                              the zeros beyond the frame then refer to the ROTATED frame (h x w pixels for 90 / 270) */
} cstp_clip_batch_desc;
/* sizeof(cstp_clip_batch_desc), for callers that pack the table without this header. */
size_t cstp_clip_batch_desc_bytes(void);
/* desc_dev: the n descriptors on the device; desc_host: the same table in host memory, read only during the call to check
 * every offset and slot against the buffer sizes given here before anything is launched (the device copy may still be in
 * flight on `stream`).  frame_idx: device int32 [n_idx]; tmp: device uint8, tmp_pixels * 3 bytes; out / out8 may be NULL when
 * no clip targets them.  Exactly one of out_slot / out8_slot is >= 0 per clip. */
int cstp_clip_batch_forward(void* stream, const cstp_clip_batch_desc* desc_dev, const cstp_clip_batch_desc* desc_host, int32_t n,
                            int32_t t, int32_t size, const int32_t* frame_idx, int32_t n_idx, uint8_t* tmp, int64_t tmp_pixels,
                            float* out, int32_t out_slots, uint8_t* out8, int32_t out8_slots);

/* ---- mixup / CutMix of a batch of fp32 clips (fine-tuning; no reference counterpart) ----
 * x: [b][planes][h][w] (planes = 3*T) -> y of the same shape, y must not alias x.  One launch, driven by a DEVICE table with one
 * entry per sample i:
 *   mode 0: y[i] = x[i]
 *   mode 1: y[i] = lam*x[i] + (1-lam)*x[partner]                                   (mixup)
 *   mode 2: y[i] = x[partner] inside the half-open box [y0,y1) x [x0,x1) of every plane, x[i] outside: bits are copied (CutMix)
 * 16-byte accesses when w % 4 == 0 and both bases are 16-byte aligned, scalar ones otherwise.  Every block checks the entry it
 * uses (partner in [0, b), mode 1 / 2, 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w); a malformed entry, and a sample that is its own
 * partner, is served as mode 0 instead of being followed.  b <= 65535, b*planes*h*w < 2^31.  No backward: clips carry no
 * gradient. */
typedef struct cstp_clip_mix_entry {
  int32_t partner;         /* row of the batch this sample is blended with */
  int32_t mode;            /* 0 copy, 1 mixup, 2 CutMix */
  float lam;               /* blend weight of the sample itself (mixup) */
  int32_t y0, y1, x0, x1;  /* CutMix box, the same in every plane */
  int32_t reserved;        /* pads the entry to 32 bytes */
} cstp_clip_mix_entry;
int cstp_clip_mix(void* stream, const float* x, float* y, const cstp_clip_mix_entry* table, int32_t b, int32_t planes, int32_t h,
                  int32_t w);

/* ---- RandAugment and random erasing on a batch of 8-bit clips (fine-tuning; csrc/randaug.h; no reference
 * counterpart).  Clips are square: uint8 [b][t][s][s][3].  Every operation equals the Pillow call it stands for bit for bit, on
 * every frame, with the fill colour (128, 128, 128).
 * cstp_randaug_layer applies ONE operation per clip, src -> dst (dst must not alias src), read from a table with one entry per
 * clip; at most two launches whatever b is:
 *   op 0  copy
 *   op 1  ImageOps.autocontrast        op 2  ImageOps.equalize     (per frame and channel: histograms -> look-up tables)
 *   op 3  ImageOps.posterize: v & a[0]                              (a[0] = ~(2^(8 - bits) - 1) & 255)
 *   op 4  ImageOps.solarize: v < a[0] ? v : 255 - v
 *   op 5  ImageEnhance.Brightness      op 6  ImageEnhance.Contrast  op 7  ImageEnhance.Color   op 8  ImageEnhance.Sharpness
 *         = Image.blend(degenerate, image, factor) against black / the frame's mean luma / the pixel's luma / the 3x3
 *         ImageFilter.SMOOTH of the frame; single precision without fused multiply-add, as cstp_clip_blend
 *   op 9  Image.transform(AFFINE, NEAREST, fillcolor) / Image.rotate(fillcolor): Geometry.c affine_fixed with the six 16.16
 *         fixed-point coefficients a[0..5] (as cstp_clip_rotate's coef6), the fill colour outside the frame
 *   op 10 integer translation: out(x, y) = in(x + a[0], y + a[1]), the fill colour outside the frame
 * lut: device uint8 [b][t][3][256], mean: device int32 [b][t] -- scratch of the statistics launch, which runs only when some
 * entry holds op 1, 2 or 6 (both may be NULL otherwise); nothing is read back.  table_host is the same table in host memory,
 * read only during the call to check every entry before anything is launched.  b <= 65535, s <= 4096, t*s*s*3 < 2^31.
 * cstp_randaug_finish is cstp_clip_finish for the whole batch in one launch: clip i of src -> out[out_slot] (fp32
 * [out_slots][3][t][s][s]) with [FLIP_LEFT_RIGHT] -> ToTensor -> x * 2 - 1 clamped.  A box with w, h > 0 -- in OUTPUT coordinates,
 * after the flip, through all frames and channels -- is erased on the way out: element e of the clip's fp32 tensor inside it
 * becomes (word >> 8) * 2^-23 - 1 (uniform on [-1, 1)), word = Philox4x32-10(counter (e >> 2, 0), key)[e & 3], the counter layout
 * of cstp_dropout with offset 0. */
typedef struct cstp_randaug_entry {
  int32_t op;              /* 0..10, see above */
  int32_t a[6];            /* fixed-point coefficients / shift / mask / threshold */
  float factor;            /* blend factor of ops 5..8 */
} cstp_randaug_entry;
typedef struct cstp_randaug_finish_entry {
  int32_t out_slot;        /* clip index in out */
  int32_t flip;            /* FLIP_LEFT_RIGHT folded into the store */
  int32_t x0, y0, w, h;    /* erased box in the output frame; w = h = 0: none */
  uint32_t key_lo, key_hi; /* the 64-bit Philox key of the fill */
} cstp_randaug_finish_entry;
/* sizeof(cstp_randaug_entry) == sizeof(cstp_randaug_finish_entry), for callers that pack the tables without this header. */
size_t cstp_randaug_entry_bytes(void);
int cstp_randaug_layer(void* stream, const uint8_t* src, uint8_t* dst, const cstp_randaug_entry* table_dev,
                       const cstp_randaug_entry* table_host, int32_t b, int32_t t, int32_t s, uint8_t* lut, int32_t* mean);
int cstp_randaug_finish(void* stream, const uint8_t* src, float* out, const cstp_randaug_finish_entry* table_dev,
                        const cstp_randaug_finish_entry* table_host, int32_t b, int32_t t, int32_t s, int32_t out_slots);

/* ---- per-step utilities over FLAT parameter arenas -------------------------------------- */
/* EMA r21d_byol.py:331-337: target = target*m + online*(1-m) over n floats. */
int cstp_ema_update(void* stream, float* target, const float* online, size_t n, double m);
/* out[0] = sum(g^2) over n floats (for clip_grad_norm_, main_byol.py:88-90); ws >= 8 KiB. */
int cstp_sumsq(void* stream, const float* g, size_t n, float* out, void* ws, size_t ws_bytes);
/* coef[0] = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)); norm_out[0] = sqrt(sumsq[0]). */
int cstp_clip_coef(void* stream, const float* sumsq, float max_norm, float* coef, float* norm_out);
/* torch.optim.SGD step (main_byol.py:91,228-232; momentum, weight decay, no nesterov, dampening 0):
 *   g' = g*coef[0] (coef may be NULL); if write_back_grad: g = g';  g' += wd*p;
 *   buf = first_step ? g' : momentum*buf + g';  p -= lr[0]*buf.   lr is a DEVICE scalar. */
int cstp_sgd_step(void* stream, float* p, float* g, float* buf, size_t n, const float* lr, float momentum,
                  float weight_decay, const float* coef, int32_t first_step, int32_t write_back_grad);
/* torch.optim.Adam (decoupled = 0: g += wd*p) / AdamW (decoupled = 1: p *= 1 - lr*wd), no amsgrad
 * (main_ft_mp.py:139-147): m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;
 * p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).  `step` counts from 1; lr is a DEVICE scalar. */
int cstp_adam_step(void* stream, float* p, const float* g, float* exp_avg, float* exp_avg_sq, size_t n, const float* lr,
                   float beta1, float beta2, float eps, float weight_decay, int32_t decoupled, int32_t step);

/* LARS (SGD with momentum whose step is scaled per tensor by a trust ratio), the variant of the published BYOL-family PyTorch
 * code: no eps in the ratio, tensors with dim() <= 1 (biases, BatchNorm gamma / beta) get neither weight decay nor adaptation.
 * Per tensor, c = coef[0] (1 when coef is NULL):
 *   g <- c*g                                  (written back when write_back_grad)
 *   adapted:     d = g + wd*p;  wn = ||p||_2, dn = ||d||_2 over the whole tensor (accumulated in double);
 *                q = eta*wn/dn if wn > 0 and dn > 0 else 1;  d = q*d
 *   not adapted: d = g;  q = 1
 *   buf <- momentum*buf + d;   p <- p - lr[0]*buf          (buf starts at zero; lr is a DEVICE scalar)
 * The tensors of one call are described by two DEVICE int32 tables over arenas p / g / buf of n floats (n < 2^31):
 *   chunks [n_chunks][3] = {segment, offset, length}: a run of floats of ONE tensor, offset and length multiples of 4 (tensors
 *                          start on 16-byte boundaries and are zero-padded to four floats; the padding belongs to the chunk and
 *                          stays zero), length <= CSTP_LARS_CHUNK; the chunks of a segment are consecutive
 *   segs   [n_segs][3]   = {first chunk, chunk count, adapted}: one tensor
 * One block per chunk.  cstp_lars_ratio: two launches (chunk partials into ws, then a fixed-order sum per segment) ->
 * ratio[n_segs] = q.  cstp_lars_step: one launch, the update with those q.  No atomics, no host read: equal inputs give equal
 * bits.  A table entry that points outside the arena or the tables is skipped, not followed. */
#define CSTP_LARS_CHUNK 4096
int cstp_lars_chunk(void);                          /* CSTP_LARS_CHUNK of the built library */
size_t cstp_lars_workspace_bytes(int32_t n_chunks); /* two doubles per chunk; 0 for n_chunks <= 0 */
int cstp_lars_ratio(void* stream, const float* p, const float* g, size_t n, const int32_t* chunks, int32_t n_chunks,
                    const int32_t* segs, int32_t n_segs, float weight_decay, float eta, const float* coef, float* ratio, void* ws,
                    size_t ws_bytes);
int cstp_lars_step(void* stream, float* p, float* g, float* buf, size_t n, const int32_t* chunks, int32_t n_chunks,
                   const int32_t* segs, int32_t n_segs, const float* ratio, const float* lr, float momentum, float weight_decay,
                   const float* coef, int32_t write_back_grad);

/* cstp_sgd_step / cstp_adam_step with PER-TENSOR hyper-parameters (layer-wise learning-rate decay, no weight decay on biases and
 * BatchNorm vectors) and an optional weight EMA in the same pass: ONE launch whatever the grouping.  The trainable tensors are
 * described by the chunk table of LARS above (chunks [n_chunks][3] = {segment, offset, length}; frozen tensors are not listed and
 * are never touched) and a DEVICE float table
 *   hyper [n_segs][2] = {lr scale, weight decay}: one tensor
 * over arenas of n floats (n < 2^31).  With s the chunk's segment, scale = hyper[s][0], wd = hyper[s][1], and lr[0] * scale ONE
 * fp32 product (lr is the DEVICE scalar of the plain entry points):
 *   cstp_tab_sgd_step:   g' = g*coef[0] (coef may be NULL); if write_back_grad: g = g';  g' += wd*p;
 *                        buf = first_step ? g' : momentum*buf + g';  p -= (lr[0]*scale)*buf
 *   cstp_tab_adam_step:  with l = lr[0]*scale: decoupled = 0: g += wd*p / decoupled = 1: p *= 1 - l*wd;
 *                        m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g;  p -= l/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * the fp32 expressions of cstp_sgd_step / cstp_adam_step: with every scale 1 and one wd the results are theirs bit for bit.
 * ema (may be NULL; an arena of the layout of p): after the update, ema = ema_momentum*ema + (1 - ema_momentum)*p, the expression
 * of cstp_ema_update, saving that pass's read of p and its launch.  One block per chunk, no atomics, no host read: equal inputs
 * give equal bits; zero padding stays zero in every arena; a table entry that points outside the arena or the tables is skipped. */
int cstp_tab_sgd_step(void* stream, float* p, float* g, float* buf, float* ema, size_t n, const int32_t* chunks, int32_t n_chunks,
                      const float* hyper, int32_t n_segs, const float* lr, float momentum, const float* coef, int32_t first_step,
                      int32_t write_back_grad, float ema_momentum);
int cstp_tab_adam_step(void* stream, float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                       const int32_t* chunks, int32_t n_chunks, const float* hyper, int32_t n_segs, const float* lr, float beta1,
                       float beta2, float eps, int32_t decoupled, int32_t step, float ema_momentum);

/* ---- the bf16-STORAGE path (BASELINE configs[4]: 3D-ResNet-50 backbone swap, bf16) --------------------------------
 * The ATen call-sites of models/BE/r3d_byol.py under bf16 activations (what torch.autocast(bfloat16) makes of them): every
 * 5-D activation tensor and every gradient of one is bf16 in HBM (uint16_t* below = raw bf16 bits, NCDHW, contiguous), all
 * arithmetic between a load and a store is fp32 (fp64 in the BatchNorm reductions), each stored value is rounded to
 * nearest-even once; weights, weight gradients, BatchNorm parameters / statistics stay fp32; convolution operands are the
 * bf16 activations and the fp32 weights rounded to bf16 at use (v_mfma_f32_16x16x32_bf16, fp32 accumulation).
 * Geometry limits: any channel counts with at most 27 taps -- forward, data gradient and weight gradient (counts that are not
 * multiples of 16, such as R(2+1)D's mid channels 83 / 230 / 460 / 921, are gathered in 16-channel groups whose last one is
 * partial: the missing channels read as zero and meet zero-padded packed weights; no padded copy of the activation) -- or, above
 * 27 taps, any channel count with taps * channels <= 1056 (the 3-channel 7x7x7 / 1x7x7 stems through a zero-padded copy and an
 * offset table, forward and weight gradient only); every gathered tensor < 2 GiB; the bf16 OUTPUT of the forward and of the data
 * gradient 8-byte aligned (four values per store; refused before anything is launched; the gathered operands may start at
 * any element).  Anything else is refused with an error, not emulated. */
/* x.to(torch.bfloat16) of the clip (r3d_byol.py:193-194 under autocast): n floats -> n bf16, round to nearest even. */
int cstp_b16_cast(void* stream, const float* x, uint16_t* y, size_t n);
size_t cstp_b16_conv3d_workspace_bytes(const cstp_conv_desc* desc);
/* F.conv3d(x, w) of r3d_byol.py:45-53 (conv3x3x3), :104-111 (Bottleneck 1x1x1 / 3x3x3 / 1x1x1), :150-152 (7x7x7 stem),
 * :177-180 (1x1x1 shortcut): y[n][k][do][ho][wo] bf16. */
int cstp_b16_conv3d_forward(void* stream, const cstp_conv_desc* desc, const uint16_t* x, const float* w, uint16_t* y, void* ws,
                            size_t ws_bytes);
/* its autograd backward w.r.t. the input: dx[n][c][d][h][w] bf16 (every element written). */
int cstp_b16_conv3d_backward_data(void* stream, const cstp_conv_desc* desc, const uint16_t* dy, const float* w, uint16_t* dx,
                                  void* ws, size_t ws_bytes);
/* ... accumulate != 0: dx = bf16(bf16(gradient) + dx) -- the second gradient of a tensor that feeds two ops (a residual
 * connection) added in the epilogue instead of by a separate add pass; the rounding points are those of the add it replaces. */
int cstp_b16_conv3d_backward_data_acc(void* stream, const cstp_conv_desc* desc, const uint16_t* dy, const float* w, uint16_t* dx,
                                  void* ws, size_t ws_bytes, int32_t accumulate);
/* ... and w.r.t. the weight: dw[k][c][kt][kh][kw] fp32, accumulate != 0: dw += (position splits through fp32 slabs summed in
 * a fixed order: bit-reproducible). */
int cstp_b16_conv3d_backward_weight(void* stream, const cstp_conv_desc* desc, const uint16_t* x, const uint16_t* dy, float* dw,
                                    void* ws, size_t ws_bytes, int32_t accumulate);
size_t cstp_b16_bn_workspace_bytes(int32_t n, int32_t c, int32_t s, int32_t groups);
/* relu(bn(x) + residual) in train mode (r3d_byol.py:84-95, :117-135, :153-154, :181): as cstp_bn_forward_train on bf16 x /
 * residual / y; scale_shift (float[groups][c][2], required) receives the affine form the apply pass uses. */
int cstp_b16_bn_forward_train(void* stream, const uint16_t* x, const uint16_t* residual, uint16_t* y, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                              float* scale_shift, int32_t n, int32_t c, int32_t s, int32_t groups, float eps, float momentum,
                              int32_t relu, void* ws, size_t ws_bytes);
/* its backward: as cstp_bn_backward_am (y == NULL with relu: the mask is recomputed from x and scale_shift). */
int cstp_b16_bn_backward(void* stream, const uint16_t* x, const uint16_t* y, const uint16_t* dy, const float* gamma,
                         const float* save_mean, const float* save_invstd, const float* scale_shift, uint16_t* dx,
                         uint16_t* dresidual, float* dgamma, float* dbeta, int32_t n, int32_t c, int32_t s, int32_t groups,
                         int32_t relu, void* ws, size_t ws_bytes, int32_t accumulate);
/* every BatchNorm3d under model.eval() (main_ft_mp.py:261-262, test.py:75-81) on bf16: as cstp_bn_forward_eval. */
int cstp_b16_bn_forward_eval(void* stream, const uint16_t* x, const uint16_t* residual, uint16_t* y, const float* gamma,
                             const float* beta, const float* running_mean, const float* running_var, int32_t n, int32_t c,
                             int32_t s, float eps, int32_t relu);
/* nn.MaxPool3d r3d_byol.py:158 on bf16 (same tie rule and argmax as cstp_maxpool3d_forward). */
int cstp_b16_maxpool3d_forward(void* stream, const uint16_t* x, uint16_t* y, int32_t* argmax, int32_t rows, int32_t d, int32_t h,
                               int32_t w, const int32_t* kernel3, const int32_t* stride3, const int32_t* pad3);
int cstp_b16_maxpool3d_backward(void* stream, const uint16_t* dy, const int32_t* argmax, uint16_t* dx, int32_t rows, int32_t d,
                                int32_t h, int32_t w, const int32_t* kernel3, const int32_t* stride3, const int32_t* pad3);
/* nn.AdaptiveAvgPool3d(1) r3d_byol.py:203: bf16 rows -> fp32 means; backward: fp32 dy -> bf16 dx. */
int cstp_b16_avgpool_forward(void* stream, const uint16_t* x, float* y, int32_t rows, int32_t s);
int cstp_b16_avgpool_backward(void* stream, const float* dy, uint16_t* dx, int32_t rows, int32_t s);

/* ---- S3D-G self-gating fused with the inception concat (csrc/gate.hip) -------------------------------------------------
 * Replaces, per SepInception block (models/coclr/s3dg.py:100-110, :150-163), the four SelfGating calls
 *   torch.mean(x_i, dim=[2,3,4]) -> fc_i (Linear c_i x c_i) -> torch.sigmoid -> weights[:, :, None, None, None] * x_i
 * and the torch.cat((x0, x1, x2, x3), 1) that follows them.  Branch i: x_i [n][c_i][s] (the output of its last BN+ReLU),
 * w_i [c_i][c_i], b_i [c_i]; it occupies channels [o_i, o_i + c_i) of y [n][C][s], C = sum c_i, o_i = c_0 + .. + c_{i-1}.
 * m [n][C] receives the means, g [n][C] the gates.  Reductions run in a fixed order and no float atomics are used: two calls
 * with the same inputs give bit-identical outputs, whether or not the pointers are 16-byte aligned (the scalar bodies that
 * serve unaligned rows with s % 4 == 0 add in the order of the 16-byte ones). */
typedef struct cstp_gate_branch {
  const float* x;      /* [n][c][s] branch output */
  const float* w;      /* [c][c] gating Linear weight (fc.weight) */
  const float* b;      /* [c] gating Linear bias (fc.bias) */
  float* dx;           /* backward: [n][c][s] */
  float* dw;           /* backward: [c][c] */
  float* db;           /* backward: [c] */
  int32_t c;           /* channels of this branch */
  int32_t reserved;    /* 0 */
} cstp_gate_branch;
#define CSTP_GATE_MAX_BRANCHES 4
/* Forward, two launches: means, then gate + apply straight into the concat tensor y.  m is required (the apply launch
 * reads it); g may be NULL (no gradient needed).  y_absmax (optional): max |y| as fp32 bits (see cstp_bn_forward_train_am). */
int cstp_gate_concat_forward(void* stream, const cstp_gate_branch* branches, int32_t nbranch, int32_t n, int32_t s, float* y,
                             float* m, float* g, uint32_t* y_absmax);
size_t cstp_gate_workspace_bytes(int32_t n, int32_t ctot);
/* Backward, three launches, given dy [n][C][s] of the whole concat tensor (read through each branch's channel offset):
 *   t = sum_s dy * x,  d = t g (1 - g),  dw_i = sum_n d_i (x) m_i,  db_i = sum_n d_i,  dm_i[n][k] = sum_c w_i[c][k] d_i[n][c],
 *   dx_i = g dy + dm_i / s.
 * accumulate != 0: dw / db are ADDED to (a flat gradient arena), else written. */
int cstp_gate_concat_backward(void* stream, const cstp_gate_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                              const float* dy, const float* m, const float* g, void* ws, size_t ws_bytes, int32_t accumulate);

/* ---- I3D: TensorFlow-SAME max-pool, the inception tail, the fine-tune head's average pool (csrc/mixed.hip) ----------------
 * SAME max-pool (models/BE/i3d_byol.py:170-183): MaxPool3d(k, s, ceil_mode=True) over ConstantPad3d(get_padding_shape(k, s), 0)
 * without the padded copy.  Per dimension pad = max(k - s, 0), front = pad / 2, the rest behind; output length
 * cstp_maxpool3d_same_out(n, k, s) = ceil((n + pad - k) / s) + 1, one less if the last window would start at or beyond n + pad.
 * A window position in the padding is a candidate of value 0, one beyond the padded extent is none; scan order, the strict `>`
 * tie rule and the NaN rule are those of cstp_maxpool3d_forward.  argmax (int32, may be NULL in forward) holds the flat index
 * in the UNPADDED (d, h, w) volume, or -1 where a padding zero won (its gradient is dropped).  backward gathers (no atomics). */
int cstp_maxpool3d_same_out(int32_t n, int32_t k, int32_t s);
int cstp_maxpool3d_same_forward(void* stream, const float* x, float* y, int32_t* argmax, int32_t rows, int32_t d, int32_t h,
                                int32_t w, const int32_t* kernel3, const int32_t* stride3);
int cstp_maxpool3d_same_backward(void* stream, const float* dy, const int32_t* argmax, float* dx, int32_t rows, int32_t d,
                                 int32_t h, int32_t w, const int32_t* kernel3, const int32_t* stride3);
/* nn.AvgPool3d(kernel, stride 1) over valid windows (i3d_byol.py:297): x [rows][d][h][w] -> y [rows][d-kd+1][h-kh+1][w-kw+1]. */
int cstp_avgpool3d_window_forward(void* stream, const float* x, float* y, int32_t rows, int32_t d, int32_t h, int32_t w,
                                  const int32_t* kernel3);
int cstp_avgpool3d_window_backward(void* stream, const float* dy, float* dx, int32_t rows, int32_t d, int32_t h, int32_t w,
                                   const int32_t* kernel3);
/* Mixed tail (i3d_byol.py:214-220 with :159-167 of each branch's last Unit3Dpy): train-mode BatchNorm3d + ReLU of up to four
 * branches written straight into channels [o_i, o_i + c_i) of the concat tensor y [n][C][s].  Branch i: x_i [n][c_i][s], the raw
 * output of its last convolution.  part != NULL: the table cstp_conv3d_forward_bnstats left beside x_i ([c][groups][nsplit][2]
 * sums around the pivots behind them); the statistics then take the arithmetic of cstp_bn_forward_train_pre and y equals
 * cstp_bn_forward_train_pre + concatenation bit for bit.  part == NULL: one statistics launch covers every such branch.
 * save_mean / save_invstd [groups][C] and scale_shift [groups][C][2] are indexed by CONCAT channel.  Launches: finalize + apply
 * (+ statistics).  No float atomics: a second call gives the same bits. */
typedef struct cstp_bnc_branch {
  const float* x;          /* [n][c][s] */
  const float* gamma;      /* [c] */
  const float* beta;       /* [c]; not read by backward (may be NULL there) */
  float* running_mean;     /* [c], updated by the train forward; with running_var, or both NULL */
  float* running_var;
  const double* part;      /* train forward: the producing convolution's partial sums, or NULL */
  float* dx;               /* backward: [n][c][s] */
  float* dgamma;           /* backward: [c] */
  float* dbeta;            /* backward: [c] */
  uint32_t* dx_absmax;     /* backward, optional: max |dx_i| as fp32 bits */
  int32_t c;
  int32_t nsplit;          /* of part */
} cstp_bnc_branch;
#define CSTP_BNC_MAX_BRANCHES 4
size_t cstp_bnrelu_concat_workspace_bytes(int32_t ctot, int32_t groups);
int cstp_bnrelu_concat_forward(void* stream, const cstp_bnc_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                               int32_t groups, float eps, float momentum, float* y, float* save_mean, float* save_invstd,
                               float* scale_shift, void* ws, size_t ws_bytes, uint32_t* y_absmax);
/* model.eval(): the running statistics are the statistics (cstp_bn_forward_eval per branch + concatenation); two launches. */
int cstp_bnrelu_concat_eval(void* stream, const cstp_bnc_branch* branches, int32_t nbranch, int32_t n, int32_t s, float eps,
                            float* y, float* scale_shift, uint32_t* y_absmax);
/* Backward, two launches: dy [n][C][s] of the whole concat tensor is read through each branch's channel offset; the ReLU mask is
 * recomputed from x_i and scale_shift.  accumulate != 0: dgamma / dbeta are ADDED to (a flat gradient arena), else written. */
int cstp_bnrelu_concat_backward(void* stream, const cstp_bnc_branch* branches, int32_t nbranch, int32_t n, int32_t s,
                                int32_t groups, const float* dy, const float* save_mean, const float* save_invstd,
                                const float* scale_shift, void* ws, size_t ws_bytes, int32_t accumulate);

/* ---- nearest-neighbour video retrieval: streaming similarity top-k (csrc/retrieve.hip) -------------------------------------
 * The evaluation protocol after the feature (no call-site in the reference): q [nq][d] queries, g [ng][d] gallery rows, fp32,
 * row-major, FINITE (NaN handling is not specified), L2-normalised by the caller with cstp_l2_normalize_forward.
 *   sim(i, j) = sum_c q[i][c] * g[j][c]     fp32 products, fp32 accumulation, c ascending (one fmaf chain per pair)
 * val / idx [nq][k]: row i holds the k largest sim(i, .) and their gallery rows, by similarity descending; where two
 * similarities are bit-equal the LOWER gallery index comes first.  Where fewer than k candidates exist (ng < k, or ng - 1 < k
 * with exclude_self) the tail is idx = -1, val = -inf.  exclude_self != 0 (q and g are the same set): candidate j == i is skipped.
 * Limits: 1 <= k <= 64, d >= 1, 1 <= nq, ng < 2^31 - 128; anything else is refused before any HIP call.
 * The [nq][ng] matrix never exists: a block owns 64 queries and streams its share of the gallery in tiles of 128 rows, keeping k
 * candidates per query.  With few queries the gallery is split over nsplit <= 32 blocks per query tile, whose lists go through
 * the workspace and a second launch that merges them; the answer does not depend on nsplit.  Workspace:
 * nsplit * nq * k * 8 bytes rounded up to 512, plus 256 -- at most 32 * nq * k * 8 + 768, growing with nq * k and never with
 * nq * ng.  No atomics: two calls give the same bits.  One launch, two when the gallery is split.  The environment variable
 * CSTP_SIMTOPK_NSPLIT (1..32, read by every call and by the workspace query) overrides nsplit: a developer knob, the tests pin
 * the unsplit path with it. */
size_t cstp_simtopk_workspace_bytes(int32_t nq, int32_t ng, int32_t d, int32_t k);
int cstp_simtopk(void* stream, const float* q, const float* g, int32_t nq, int32_t ng, int32_t d, int32_t k,
                 int32_t exclude_self, float* val, int32_t* idx, void* ws, size_t ws_bytes);

/* ---- weighted k-nearest-neighbour classification: the vote on a similarity top-k list (csrc/retrieve.hip) ------------------
 * val / idx [nq][k] are exactly what cstp_simtopk writes: similarity descending, (-inf, -1) where candidates ran out.
 * g_labels [ng] int32, values >= 0.  pred / score [nq][n_top].  Per row:
 *   slot j is LIVE iff 0 <= idx[j] < ng; a dead slot weighs 0 and its idx is never used to form an address;
 *   w_j = expf((val_j - val_0) * inv_t) in fp32, val_0 the row's first (largest) value: w_0 = 1 and nothing overflows at any
 *         temperature, whether or not the features were normalised;
 *   score(c) = sum of w_j over the live slots with g_labels[idx_j] == c, added in slot order j ascending (one fixed order: no
 *         atomics, no class table, so the number of classes is unbounded, and two slots of one class see the same bits);
 *   output: the n_top best distinct classes by (score descending, class id ascending); (-1, 0.0f) where they run out.
 * Equal inputs give equal bits on every call.  One launch, one wave per query, no workspace.
 * Limits: 1 <= k <= 64, 1 <= n_top <= 8, nq >= 1, ng >= 1, inv_t finite and > 0, no null pointer; anything else is refused
 * before any HIP call. */
int cstp_knn_vote(void* stream, const float* val, const int32_t* idx, const int32_t* g_labels, int32_t nq, int32_t ng,
                  int32_t k, float inv_t, int32_t n_top, int32_t* pred, float* score);

/* ---- linear probe on cached features: a softmax classifier on frozen features (csrc/probe.h) --------------------------------
 * x [n][d] fp32 is the feature matrix; d need not be a multiple of anything and the rows need not be 16-byte aligned.
 * mean [d], inv_std [d] fp32 standardise on load, xs = (x - mean) * inv_std (either may be NULL: 0 and 1); no standardised copy
 * is written.  w [c][d], b [c] fp32.  logit(r, k) = b[k] + sum_f xs[r][f] * w[k][f]: fp32 fmaf chain in feature order, bias last.
 *
 * cstp_probe_step: the batch is rows [m] int32 into x (NULL: rows 0..m-1, then m <= n); labels [n] int64 are indexed by the
 * gathered row, y_r = labels[rows[r]].
 *   loss[0] = mean_r -log_softmax(logit(r, .))[y_r]   soft-max about the row maximum, the mean over m accumulated in double
 *   hits[0] = number of rows whose arg-max class is y_r (int32), ties going to the lowest class id
 *   dw [c][d] = (1/m) sum_r (p_r - onehot(y_r)) xs_r^T,  db [c] = (1/m) sum_r (p_r - onehot(y_r))
 * A label outside [0, c) follows the convention of cstp_soft_cross_entropy_* above: no one-hot mass, never used to form an
 * address, and here the row contributes 0 to loss, gradients and hits; an index in rows outside [0, n) is treated the same way and
 * is never dereferenced.  Such rows still count in m.
 * Three launches whatever the sizes (logits + soft-max of 8-row slabs; dw over 64 x 64 tiles and S row slices; the fold of the
 * slices, db, loss and hits), no atomics, no host read; every cross-row and cross-block sum has one fixed order, so equal inputs
 * give equal bits.  Nothing is written outside loss, hits, dw, db and the first cstp_probe_workspace_bytes(m, d, c) bytes of ws:
 *   cpad = 4 * ceil(c / 4);  S = max(1, min(32, ceil(m / 64), floor(512 / (ceil(d / 64) * ceil(c / 64)))))
 *   bytes = 4 * m * cpad                     g = (p - onehot) / m, [m][cpad]
 *         + round16(8 * m)                   row losses (fp32) and row hits (int32)
 *         + round16(4 * S * c)               db per slice
 *         + (S > 1 ? 4 * S * c * d : 0)      dw per slice
 * (round16: up to a multiple of 16).  cstp_probe_workspace_bytes is a pure host function, non-decreasing in m, 0 on bad arguments.
 *
 * cstp_probe_predict: for every row 0..n-1 the n_top best classes by (logit descending, class id ascending) and their logits,
 * pred / score [n][n_top] -- the layout cstp_knn_vote writes; (-1, 0.0f) where n_top > c.  One launch, no workspace, no logits
 * table in memory, equal bits on equal inputs.
 *
 * Limits, refused with a message before any HIP call: m, n, d >= 1; 2 <= c <= 1024; c * d < 2^31; 1 <= n_top <= 8; no NULL
 * among the required pointers (all but rows, mean, inv_std); dw / db overlapping w / b; ws not 16-byte aligned or smaller than
 * cstp_probe_workspace_bytes(m, d, c). */
size_t cstp_probe_workspace_bytes(int32_t m, int32_t d, int32_t c);
int cstp_probe_step(void* stream, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                    const float* inv_std, const float* w, const float* b, int32_t m, int32_t n, int32_t d, int32_t c, float* loss,
                    int32_t* hits, float* dw, float* db, void* ws, size_t ws_bytes);
int cstp_probe_predict(void* stream, const float* x, const float* mean, const float* inv_std, const float* w, const float* b,
                       int32_t n, int32_t d, int32_t c, int32_t n_top, int32_t* pred, float* score);

/* ---- linear-probe sweep: `heads` classifiers on the same batch in the same launches (csrc/probe.h) -------
 * A head is one classifier (W_h [c][d], b_h [c]).  w and b point at head 0; head h lies head_stride floats further on, in both, and
 * dw / db use the same stride.  probe.fit's arena layout is the intended one: seg = pad4(c d) + pad4(c) floats per head, W_h at
 * h * seg, b_h at h * seg + pad4(c d) (pad4: up to a multiple of 4), head_stride = seg.  x, rows, labels, mean, inv_std are shared.
 *
 * cstp_probe_sweep_step: for every head h what cstp_probe_step returns for (W_h, b_h) alone on the same x, rows, labels, mean,
 * inv_std -- loss[h], hits[h], dW_h, db_h -- BIT FOR BIT: the kernels are the single-head kernels with the head as a grid
 * dimension (logits, fold) or a factor of one (dw: z = head * S + slice, S as for one head), so every fmaf chain, wave reduction,
 * row slice and fold order is the single-head one.  Three launches whatever `heads` is, no atomics, no host read.
 * cstp_probe_sweep_score: loss[h] and hits[h] only, the same bits; nothing of size [m][c] or [c][d] is written.  Two launches.
 * Row indices outside [0, n) and labels outside [0, c) are treated as in cstp_probe_step, for every head.
 *
 * Workspace: head h owns bytes [h * round16(cstp_probe_workspace_bytes(m, d, c)), (h + 1) * the same), laid out as the single-head
 * workspace; cstp_probe_sweep_workspace_bytes(heads, m, d, c) = heads * round16(cstp_probe_workspace_bytes(m, d, c)), 0 on a bad
 * shape or heads outside 1..32.  Nothing is written outside loss [heads], hits [heads], the heads' dw / db extents ([c][d] and [c]
 * floats each: the padding between heads is left alone) and that many bytes of ws; the score writes only the row-loss and row-hit
 * parts of each head's workspace.
 *
 * Refused with a message before any HIP call: NULL among the required pointers (all but rows, mean, inv_std); heads outside
 * 1..32; c outside 2..1024; a bad shape (as cstp_probe_step); m > n without rows; head_stride not a multiple of 4 or smaller than
 * pad4(c d) + c; the dw / db extent of any head overlapping the w / b extent of any head; ws not 16-byte aligned or too small. */
size_t cstp_probe_sweep_workspace_bytes(int32_t heads, int32_t m, int32_t d, int32_t c);
int cstp_probe_sweep_step(void* stream, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                          const float* inv_std, const float* w, const float* b, int64_t head_stride, int32_t heads, int32_t m,
                          int32_t n, int32_t d, int32_t c, float* loss, int32_t* hits, float* dw, float* db, void* ws,
                          size_t ws_bytes);
int cstp_probe_sweep_score(void* stream, const float* x, const int32_t* rows, const int64_t* labels, const float* mean,
                           const float* inv_std, const float* w, const float* b, int64_t head_stride, int32_t heads, int32_t m,
                           int32_t n, int32_t d, int32_t c, float* loss, int32_t* hits, void* ws, size_t ws_bytes);

/* ---- fine-tuning regularisers: dropout and the stochastic-depth residual join (csrc/reg.h) -----------
 * Philox4x32-10 (Salmon et al., SC'11) on the host: out4 = Philox(ctr4, key2).  The function the dropout kernel evaluates,
 * exported so that its known answers can be checked without a device. */
int cstp_philox4x32_10(const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4);
/* Dropout with a counter-based mask, fp32, x [n] -> y [n] (y may alias x).  For element e:
 *   ctr = (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)),  key = (lo32(seed), hi32(seed))
 *   w   = Philox4x32-10(ctr, key)[e & 3],   u = (w >> 8) * 2^-24 (exact in fp32)
 *   y   = u >= p ? x * (1.0f / (1.0f - p)) : 0
 * No mask tensor exists: the backward pass is the same call on dy with the same (seed, offset).  offset numbers the call site
 * (the classifier head uses 0).  One Philox evaluation serves four consecutive elements; 16-byte accesses where x and y are
 * 16-byte aligned, element accesses for the tail and for unaligned views, with the same bits.  One launch, no atomics.
 * Refused before any HIP call: null pointers, n <= 0, p outside [0, 1) (NaN included). */
int cstp_dropout(void* stream, const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset);
/* Stochastic depth at the end of a residual block: y[b][i] = relu(scale[b] * z[b][i] + res[b][i]), rows of row = C*D*H*W
 * elements, n = samples * row.  z, res, y: all fp32 (bf16 == 0) or all bf16 (bf16 != 0: computed in fp32, rounded to nearest
 * even).  scale [samples] fp32: 0 for a dropped sample, 1 / (1 - p) for a kept one.  The sample index is a grid dimension.
 * y_absmax (optional, fp32 only): a cell that HOLDS 0 ON ENTRY and receives max |y| as an fp32 bit pattern, one atomicMax per
 * block (the only atomic; a cell that held something larger keeps it: an over-estimate).  One launch. */
int cstp_droppath_add_relu_forward(void* stream, const void* z, const void* res, const float* scale, void* y, int64_t n,
                                   int64_t row, int32_t bf16, uint32_t* y_absmax);
/* g = dy where y > 0, else 0;  dz = scale[b] * g;  dres = g.  One launch writes both; either output may be NULL (not both). */
int cstp_droppath_add_relu_backward(void* stream, const void* y, const void* dy, const float* scale, void* dz, void* dres,
                                    int64_t n, int64_t row, int32_t bf16);

/* ---- NT-Xent with a queue of extra negatives (csrc/ntxq.h, included from csrc/retrieve.hip) ----------
 * reps [R][f] fp32 = cat(zjs, zis) as for cstp_ntxent_*; queue [cap][f] fp32, constant rows of UNIT LENGTH (cstp_ntxq_push
 * writes them), of which rows [0, n_valid) count; T = temperature.  With the reference's cosine
 *   s_ij = <r_i, r_j> / max(|r_i| |r_j|, 1e-8),   c_ik = <r_i, queue_k> / max(|r_i|, 1e-8)   (|queue_k| is taken as 1)
 *   loss = 1/R sum_i [ -s_{i,(i + R/2) mod R} / T + log( sum_{j != i} exp(s_ij / T) + sum_{k < n_valid} exp(c_ik / T) ) ]
 * n_valid == 0 is cstp_ntxent_forward's loss.  The gradient reaches reps only: the queue is never written by forward or backward,
 * and rows from n_valid on are never read (they may hold anything, NaN included).
 * A dot product is one fp32 fmaf chain in ascending feature order on v_mfma_f32_32x32x2_f32 (cstp_simtopk's walk: 64 rows x
 * tiles of 128 queue rows), so a score does not depend on the tile or the split that computes it; the [R][n_valid] matrix
 * never exists.  Forward keeps a running (max, sum exp) per row and split and folds them, in split order, with the in-batch
 * row; the maximum is subtracted throughout, so 1/T = 100 is safe.  Backward recomputes the scores tile by tile, forms
 * p_ik = exp(c_ik / T - lse_i) and accumulates P x queue in registers per slice of 256 features; the partial [split][R][f]
 * sums are added in split order to the in-batch gradient (cstp_ntxent_backward's arithmetic with the new lse) through the
 * derivative of the normalisation, scaled by dloss / (R T).  No atomics: equal inputs give equal bits.
 * The workspace of forward must reach backward unchanged.  cstp_ntxq_workspace_bytes is a pure host function (0 on bad
 * arguments): cstp_ntxent_workspace_bytes(R, f) + nsplit * R * (2 + f) * 4, where
 *   nsplit = 0 for n_valid == 0, else max(1, min(256 / ceil(R / 64), ceil(n_valid / 128) / 2, 2^22 / (R f))), then
 *   rounded so that no split is empty -- the partial gradients take 16 MiB at the most, or one split.
 * Launches: forward 3 + 1 (+ 1 with a non-empty queue), backward 2 (+ 2).
 * Limits, refused with a message before any HIP call: a null pointer; R odd, < 4 or > 8192; f outside 1..2048; T <= 0;
 * cap outside [0, 2^30]; n_valid outside [0, cap]; ws smaller than cstp_ntxq_workspace_bytes(R, f, n_valid).
 *
 * cstp_ntxq_push: queue[ptr + i] = reps[i] / max(|reps[i]|, 1e-8) for i < R (a zero row is written as zeros); every other row
 * is left as it is.  One launch; run it after the loss's launches on the same stream.  Refused: a null pointer, R outside
 * 1..8192, f outside 1..2048, ptr < 0 or ptr + R > cap. */
size_t cstp_ntxq_workspace_bytes(int32_t R, int32_t f, int32_t n_valid);
int cstp_ntxq_forward(void* stream, const float* reps, const float* queue, float* loss, int32_t R, int32_t f, int32_t cap,
                      int32_t n_valid, float temperature, void* ws, size_t ws_bytes);
int cstp_ntxq_backward(void* stream, const float* reps, const float* queue, const float* dloss, float* dreps, int32_t R,
                       int32_t f, int32_t cap, int32_t n_valid, float temperature, void* ws, size_t ws_bytes);
int cstp_ntxq_push(void* stream, const float* reps, float* queue, int32_t R, int32_t f, int32_t cap, int32_t ptr);

/* ---- spherical k-means on cached features: Lloyd's iteration for R restarts at once (csrc/kmeans.h, included from
 * csrc/retrieve.hip) ------------------------------------------------------------------------------------
 * x [n][d] fp32 rows and cent [r][c][d] fp32 centroids of r independent restarts, both L2-normalised by the caller, FINITE.
 * A row belongs to the centroid with the largest dot product.
 *
 * cstp_kmeans_assign: for every restart s and row i
 *   best[s][i]   = max_j sim(i, j),  sim(i, j) = sum_f x[i][f] * cent[s][j][f]: cstp_simtopk's fmaf chain over ascending features on
 *                  v_mfma_f32_32x32x2_f32, so (best, assign) holds the bits of cstp_simtopk(x, cent[s], k = 1)
 *   assign[s][i] = the j that attains it, the LOWEST j where several similarities are bit-equal (int32)
 *   moved[s]     = the number of rows with assign[s][i] != prev[s][i] (int32); n when prev is NULL
 *   score[s]     = sum_i best[s][i] in fp64: the 64 rows of a tile through one shuffle tree, the tiles in ascending order strided
 *                  over 256 threads, those through one tree -- a fixed order that depends on n alone
 * One block owns 64 rows and one restart and streams that restart's centroids in tiles of 128 with a running best in registers:
 * no [n][c] table, no insertion list.  Two launches (the walk; the fold of the per-tile partials), no atomics, nothing read
 * back.  Restart s of a batch gets the bits it gets alone.  prev may not overlap assign.  Workspace: r * ceil(n / 64) doubles
 * and as many int32, each plane rounded up to 16 bytes = cstp_kmeans_workspace_bytes(n, d, c, r), a pure host function (0 on
 * bad arguments); ws must be 16-byte aligned.
 *
 * cstp_kmeans_update: cent_out[s][j] = sum / |sum| of the rows with assign[s][i] == j, counts[s][j] = their number (int32).
 *   sum[f]  = (((0 + x[i_1][f]) + x[i_2][f]) + ...) in fp32 over those rows in ASCENDING ROW ORDER: one chain per (cluster,
 *             feature); the order depends on (n, assign) alone -- never on the grid, the block count or r
 *   |sum|^2 = thread t of 256 folds sum[f]^2 by fmaf over f = t, t + 256, ... ascending; the 256 partials go through one fixed tree
 *   out[f]  = sum[f] * (1.0f / sqrtf(|sum|^2)), division and square root correctly rounded
 * A cluster with counts == 0, or whose |sum|^2 is not > 0, keeps cent_in[s][j] bit for bit.  An assign value outside 0..c-1
 * belongs to no cluster: it is compared, never used to form an address.  One launch, one block per (cluster, restart), no
 * workspace, no atomics.  cent_out may not overlap cent_in.  Once an assign call reports moved == 0, further assign / update
 * rounds reproduce cent and assign bit for bit: Lloyd's iteration is at a fixed point.
 *
 * Limits, refused with a message before any HIP call: 1 <= n <= 2^24, 1 <= d <= 4096, 1 <= c <= 4096, c <= n, 1 <= r <= 32; a
 * NULL among the required pointers (all but prev); overlapping cent_in / cent_out or prev / assign; ws unaligned or too small.
 * d need not be a multiple of 4 and no pointer need be 16-byte aligned (then operands are staged by scalar loads).
 * The limits are what the indexing supports, not a promise of speed: every update block reads all of assign[s], c * n * 4 bytes
 * per restart, which suits n ~ 10^4 - 10^5 and c ~ 10^2 (105 MB at n = 65 536, c = 400) and takes many seconds at the limits. */
size_t cstp_kmeans_workspace_bytes(int32_t n, int32_t d, int32_t c, int32_t r);
int cstp_kmeans_assign(void* stream, const float* x, const float* cent, const int32_t* prev, int32_t n, int32_t d, int32_t c,
                       int32_t r, int32_t* assign, float* best, int32_t* moved, double* score, void* ws, size_t ws_bytes);
int cstp_kmeans_update(void* stream, const float* x, const int32_t* assign, const float* cent_in, int32_t n, int32_t d, int32_t c,
                       int32_t r, float* cent_out, int32_t* counts);

/* ---- label-free collapse metrics on cached features (csrc/health.h, included from csrc/retrieve.hip) ----
 * x [n][d] fp32 rows, FINITE.  Two reductions that cstp_amd/health.py turns into rank, spread and uniformity figures; neither
 * builds an [n][n] tensor nor uses an atomic, and two calls on equal inputs give equal bits.
 *
 * cstp_feat_gram: gram [d][d] fp64 and colsum [d] fp64,
 *   gram[a][b] = sum_i x[i][a] * x[i][b]: the rows are dealt in slabs of 32; inside a slab the pair (a, b) is ONE fp32 fmaf chain
 *                over ascending i (v_mfma_f32_32x32x2_f32), the slab partials are widened and added in fp64 in ascending slab order.
 *                gram[a][b] and gram[b][a] are equal bit for bit (the two chains multiply the same factors).
 *   colsum[a]  = sum_i x[i][a] in fp64: parts of 1024 rows, each added in ascending row order, the parts in ascending order.
 *   The answer is a function of (x, n, d): no grid or split choice enters it.  Two launches.  Workspace: ceil(n / 1024) * d doubles
 *   + 256 bytes = cstp_feat_gram_workspace_bytes(n, d).
 *
 * cstp_pair_potential: rowsum [n] fp64 for rows L2-normalised by the caller and t > 0,
 *   rowsum[i] = sum_{j != i} expf(2 t (s_ij - 1)),  s_ij = sum_f x[i][f] * x[j][f] with the bits of cstp_simtopk's similarity (one
 *               fmaf chain over ascending features), the accurate expf, the diagonal left out BY INDEX (duplicates of row i count).
 *   Every term is widened to fp64.  The gallery tiles of 128 rows are dealt into S = at most 32 segments of ceil(tiles / 32)
 *   tiles, a function of n alone; inside a segment lane l of a wave adds columns l, 64 + l of its tiles in ascending order and the
 *   64 lanes go through one fixed tree; a second launch adds the S segment sums of a row in ascending order.  How many segments a
 *   block walks (the gallery split of the grid, more blocks with few row tiles) changes no bit.  Workspace: S * n doubles + 256
 *   bytes = cstp_pair_potential_workspace_bytes(n, d) <= 32 * 8 * n + 4096.
 *
 * Limits, refused with a message before any HIP call, nothing touched: n >= 1, 1 <= d <= 4096, n * d < 2^31; a NULL pointer; t not
 * finite or <= 0; gram, colsum, rowsum or ws not 8-byte aligned; ws too small.  The workspace functions are pure host functions (0
 * on a bad shape).  d need not be a multiple of 4 and x need not be 16-byte aligned (then it is staged by scalar loads). */
size_t cstp_feat_gram_workspace_bytes(int32_t n, int32_t d);
int cstp_feat_gram(void* stream, const float* x, int32_t n, int32_t d, double* gram, double* colsum, void* ws, size_t ws_bytes);
size_t cstp_pair_potential_workspace_bytes(int32_t n, int32_t d);
int cstp_pair_potential(void* stream, const float* x, int32_t n, int32_t d, float t, double* rowsum, void* ws, size_t ws_bytes);

/* ---- few-shot episodic evaluation on cached features (csrc/fewshot.h, included from csrc/retrieve.hip) --
 * N-way K-shot episodes scored by the cosine nearest-centroid classifier ("ProtoNet with cosine" on frozen features).
 * xs [ns][d], xq [nq][d] fp32, rows L2-normalised by the caller, FINITE.  sup_idx [E][N][Kmax] int32 rows of xs, qry_idx [E][N][Q]
 * int32 rows of xq; the query in slot (c, j) belongs to class slot c.  shots [S] is a HOST array k_1 < ... < k_S, read before the
 * launch, Kmax = k_S.  For episode e, shot count s and class slot c:
 *   p = sum_{j < k_s} xs[sup_idx[e][c][j]]       the FIRST k_s support columns, added in column order: the shot counts are nested,
 *                                                so the counts of one call are paired on the same episodes
 *   score[s][e][q][c] = (xq[qry_idx[e][q]] . p) / sqrtf(p . p),  0.0f where p . p == 0
 *   pred[s][e][q]     = the arg-max over c, the LOWEST slot on a tie
 *   hits[s][e]        = the number of queries q with pred[s][e][q] == q / Q
 * hits [S][E] int32 is always written; pred [S][E][N Q] int32 and score [S][E][N Q][N] fp32 may be NULL (the normal call: S * E
 * integers are all that is stored).  fp32 throughout.  The features go in slices of 128; within a slice a dot product is 16 fmaf
 * chains of 8 features (feature g, g + 16, ..., g + 112 of the slice in lane g) joined by one fixed tree, the slices are added in
 * ascending order.  Every sum's order is a function of d alone: episode e has the same bits alone and among 2^20 others, shot count
 * k the same bits alone and inside a list, and two calls on equal inputs give equal bits.  One launch, one 256-thread block per
 * episode, no atomics, no workspace.  THE INDEX TABLES ARE TRUSTED: an entry outside 0..ns-1 / 0..nq-1 is an out-of-bounds read
 * (ops.fewshot_episodes range-checks host tables before it uploads them); duplicates are fine.
 * Limits, refused with a message before any HIP call, nothing touched: 2 <= N <= 20, 1 <= Q <= 32, N Q <= 320, 1 <= S <= 4, shots
 * strictly ascending in 1..16, 1 <= d <= 8192, 1 <= E <= 2^20, ns, nq >= 1, a NULL among xs, xq, sup_idx, qry_idx, shots, hits.
 * d need not be a multiple of anything and no pointer 16-byte aligned (rows are read by 4-byte loads, 256 or 64 contiguous bytes
 * at a time). */
int cstp_fewshot_episodes(void* stream, const float* xs, int32_t ns, const float* xq, int32_t nq, int32_t d,
                          const int32_t* sup_idx, const int32_t* qry_idx, int32_t episodes, int32_t n_way, int32_t n_query,
                          const int32_t* shots, int32_t n_shots, int32_t* hits, int32_t* pred, float* score);

#ifdef __cplusplus
}
#endif
#endif /* CSTP_HIP_H */
