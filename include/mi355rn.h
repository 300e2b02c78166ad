/*
 * mi355rn.h — C-ABI of libmi355rn.so: the MI355X (gfx950) native ResNet-50 training hot path.
 *
 * This is the drop-in boundary for the path bonlime/sota_imagenet drives through torch's dispatcher:
 *   model(data)            reference call form  sota_imagenet/callbacks.py:316, built at train.py:64
 *   criterion(out, target) reference call form  sota_imagenet/callbacks.py:316, built at train.py:81
 *   loss.backward()        reference call form  sota_imagenet/callbacks.py:317
 *   optimizer.step()       reference call form  sota_imagenet/callbacks.py:309, built at train.py:92
 * The reference has no FFI of its own (it is pure Python on top of torch / cuDNN / NCCL), so every entry
 * point below cites the reference call site whose native work it replaces.
 *
 * Conventions
 *   - plain C types only: device pointers as void* / float*, sizes as int / size_t, streams as void*
 *     (a hipStream_t; pass torch.cuda.current_stream().cuda_stream).  No torch types cross the boundary.
 *   - every function returns 0 on success, a negative mi355_status otherwise; mi355_last_error() gives
 *     the message (thread-local).  Nothing throws across the boundary.
 *   - the caller (PyTorch-ROCm tensors) owns parameters / gradients / momentum / inputs / logits; the
 *     library owns only its workspace arena (saved activations, split-K partials) inside a ctx.
 *   - nothing in here synchronises the host with the device; all work is enqueued on `stream`.
 *   - there is NO CPU fallback: without a gfx950 device every compute call fails with MI355_E_HIP.
 *
 * Layouts
 *   activations  NHWC, dtype MI355_F32 or MI355_BF16           (the loader's NCHW fp32 batch,
 *                sota_imagenet/dali_dataloader.py:113-122, is converted once by mi355_ingest_*)
 *   conv weights KRSC = [Cout][KH][KW][Cin] fp32 master copy   (== a torch OIHW tensor in channels_last
 *                memory format, so state_dict() keeps torchvision names/shapes)
 *   BN / FC / loss / optimizer state: fp32.
 */
#ifndef MI355RN_H
#define MI355RN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mi355_status {
  MI355_OK = 0,
  MI355_E_ARG = -1,   /* bad argument (shape / dtype / null pointer / unsupported geometry) */
  MI355_E_HIP = -2,   /* a HIP runtime call failed (message holds file:line and hipGetErrorString) */
  MI355_E_STATE = -3, /* call order violated (e.g. backward before forward, params not bound) */
  MI355_E_NOMEM = -4  /* workspace too small / allocation failed */
} mi355_status;

/* MI355_FP8: OCP e4m3fn operand bytes — the *_fp8 entry points (their outputs are bf16) and the fp8 training step of the
 * whole-network executor (mi355_resnet50_create) */
typedef enum mi355_dtype { MI355_F32 = 0, MI355_BF16 = 1, MI355_FP8 = 2 } mi355_dtype;

/* ---- library ------------------------------------------------------------------------------------ */
const char* mi355_last_error(void);
int mi355_version(void);
/* number of HIP devices visible (0 on a GPU-less host); never fails */
int mi355_device_count(void);

/* ---- per-op entry points (unit parity tests; the executor below calls the same kernels) ----------
 * All pointers are device pointers.  `ws`/`ws_bytes` is caller-provided scratch; query the need with
 * mi355_conv2d_workspace_bytes().  Where a scratch or table size is stated below as a need (">="), the library takes
 * a larger buffer; the Python wrappers (sota_imagenet_amd/ops.py) allocate the scratch themselves or take EXACTLY the size
 * their *_scratch / sizing helper gives (xpad, the spectral scratch, the ortho-loss partial / tile_ss).                */

/* scratch needed by dgrad (transposed weights) / wgrad (split-K partials) for one conv geometry */
size_t mi355_conv2d_workspace_bytes(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW,
                                    int stride, int pad);

/* y[N,Ho,Wo,Cout] = conv(x[N,H,W,Cin], w[Cout,KH,KW,Cin]); x,w,y in `dtype`.  Cin%64==0, Cout%64==0.
 * replaces cuDNN conv fwd under model(data) — callbacks.py:316 (K2 of SURVEY §2.3)                  */
int mi355_conv2d_fwd(int dtype, const void* x, const void* w, void* y, int N, int H, int W, int Cin,
                     int Cout, int KH, int KW, int stride, int pad, void* stream);

/* dx[N,H,W,Cin] = conv_transpose(dy[N,Ho,Wo,Cout], w) (+ addend[N,H,W,Cin] if non-null).
 * replaces cuDNN dgrad under loss.backward() — callbacks.py:317 (K8)                                */
/* forward conv that also leaves the BatchNorm statistics of its output as per-workgroup partial rows ([nblk][2][Cout] floats:
 * sum, sum of squares of the values AS STORED) — what the executor's convs do; *nblk = 0 when this launch shape cannot produce
 * them (then run mi355_bn_fwd_train).  partial: >= 768 * 2 * Cout floats.  Consumed by mi355_bn_fwd_train_partial.          */
int mi355_conv2d_fwd_stats(int dtype, const void* x, const void* w, void* y, float* partial, size_t partial_bytes, int* nblk,
                           int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, void* stream);
int mi355_conv2d_dgrad(int dtype, const void* dy, const void* w, void* dx, const void* addend, int N,
                       int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, void* ws,
                       size_t ws_bytes, void* stream);
/* the forward conv with the PREVIOUS layer's BatchNorm + ReLU in its operand path, as the executor's training forward launches conv2 of a
 * bottleneck (model(data), /root/reference/sota_imagenet/callbacks.py:316: BatchNorm2d -> ReLU -> Conv2d of pytorch_tools' Bottleneck; BN
 * semantics /root/reference/train.py:76, /root/reference/sota_imagenet/arg_parser.py:132):
 *   a = relu(y_in * scale[c] + shift[c]) rounded to `dtype` (what mi355_bn_apply computes from the coefficients mi355_bn_fwd_train leaves),
 *   y = conv(a, w), + the BatchNorm statistics rows of y as mi355_conv2d_fwd_stats leaves them.
 * a_out [N,H,W,Cin] and a_bits (its ReLU mask, 1 byte per 8 channels) are written by the same launch as a by-product: the weight gradient and
 * the BatchNorm backward read them; no separate bn_apply pass runs.  scale_shift: [2][Cin] floats.  bf16, 3x3 / stride 1 at the shapes the
 * generated kernels cover (MI355_E_ARG elsewhere: apply the BatchNorm with mi355_bn_apply and call mi355_conv2d_fwd_stats).                  */
int mi355_conv2d_fwd_bn_in(int dtype, const void* y_in, const float* scale_shift, const void* w, void* y, void* a_out, uint8_t* a_bits,
                           float* partial, size_t partial_bytes, int* nblk, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                           int pad, void* stream);
/* the data gradient as the executor's backward launches it (loss.backward(), /root/reference/sota_imagenet/callbacks.py:317; the
 * residual add + ReLU + BatchNorm backward autograd runs around cuDNN's dgrad there, fused into the conv's epilogue here):
 *   dx = conv_transpose(dy, w) + (addend under addend_bits — the shortcut gradient under the block output's ReLU bit mask; bits null: plain)
 * and, when `partial` is non-null, the BN-backward sums of the layer whose post-ReLU activation dx is the gradient of, as partial
 * rows [*nblk][2][Cin] floats: sum dz and sum dz * xhat, dz = dx (as stored) under bn_bits, xhat = (bn_y - bn_mean) * bn_invstd
 * (bn_y laid out like dx, bn_mean / bn_invstd [Cin] floats, masks [N][H][W][Cin / V] with one byte per 16-byte vector, V = 16 /
 * sizeof(element); addend_bits masks the addend).  *nblk = 0 when the launch shape cannot produce them.
 * partial: >= 768 * 2 * Cin floats.  dx may alias addend.
 * addend_sub2 = 1: `addend` is [N][H/2][W/2][Cin] and stands for the full-resolution tensor that is zero at odd rows / columns — the
 * data gradient of the stride-2 1x1 downsample convolution of a stage's first block, which the executor then never writes at full size
 * (bf16, 1x1 / stride 1 launches with even H and W; MI355_E_ARG elsewhere).                                                         */
int mi355_conv2d_dgrad_bn(int dtype, const void* dy, const void* w, void* dx, const void* addend, const uint8_t* addend_bits, int addend_sub2,
                          const void* bn_y, const uint8_t* bn_bits, const float* bn_mean, const float* bn_invstd, float* partial,
                          size_t partial_bytes, int* nblk, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                          void* ws, size_t ws_bytes, void* stream);
/* the same with the sums under a LEAKY ReLU mask: dz = dx where the bit is set, dx * slope elsewhere — the activation of BASELINE configs[3]'s model
 * (`norm_act: leaky_relu`, /root/reference/configs/_old_configs/_first_attempts/BResNet50_encoder.yaml:41-51; autograd's LeakyReLU + BatchNorm backward
 * around cuDNN's dgrad under loss.backward(), /root/reference/sota_imagenet/callbacks.py:317).  slope = 0: mi355_conv2d_dgrad_bn.  slope = 0.01 at the
 * shapes of that model's bottlenecks (bf16, generated kernels with that epilogue); any other slope or shape: MI355_E_ARG (run the BatchNorm backward's
 * own reduction, mi355_bn_bwd).                                                                                                                    */
int mi355_conv2d_dgrad_bn_leaky(int dtype, const void* dy, const void* w, void* dx, const void* addend, const uint8_t* addend_bits, int addend_sub2,
                                const void* bn_y, const uint8_t* bn_bits, const float* bn_mean, const float* bn_invstd, float slope, float* partial,
                                size_t partial_bytes, int* nblk, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                void* ws, size_t ws_bytes, void* stream);

/* dw[Cout,KH,KW,Cin] (fp32) = sum_{n,oh,ow} dy (x) x.  beta=0 overwrites, beta=1 accumulates.
 * replaces cuDNN wgrad under loss.backward() — callbacks.py:317 (K8)                                */
int mi355_conv2d_wgrad(int dtype, const void* dy, const void* x, float* dw, float beta, int N, int H,
                       int W, int Cin, int Cout, int KH, int KW, int stride, int pad, void* ws,
                       size_t ws_bytes, void* stream);

/* real-image ingest: the GPU half of the reference's DALI pipelines, after the JPEG decoder —
 * train sota_imagenet/dali_dataloader.py:69-83 (random crop at decode, fn.resize size=S INTERP_TRIANGULAR, or INTERP_CUBIC by
 * coin), :85-114 (gaussian blur window 11, colour twist, grey via hsv saturation, random erasing with the mean), :116-125
 * (crop_mirror_normalize: mirror coin, mean 127.5 / std 51 (:27-29), FLOAT, NCHW); val :144-157 (resize_shorter, centre crop).
 * `packed` (device) holds the decoded u8 RGB crops of one batch back to back (HWC, tight rows); sample n is described by
 * crops[n]: resize its h x w rectangle to rh x rw (filter 0: triangular = antialiased bilinear, 1: a = -0.5 cubic), take the
 * S x S window at (oy, ox), [augment[n]: gaussian blur (sigma > 0), 3x4 colour matrix on 0..255 values + clamp, luma if gray,
 * up to 4 rectangles y0,x0,y1,x1 (window coordinates before the mirror) filled with the mean], mirror if asked, write
 * (v - mean) / std to out_nchw[n] (fp32 [N,3,S,S], what mi355_resnet50_forward takes).  Tables are passed twice: the host copy
 * is validated against packed_bytes before the launch (MI355_E_ARG on a rectangle that leaves the buffer or a window that
 * leaves the resized image), the device copy is what the kernels read.  `scratch` (N*3*S*S floats) is needed only when some
 * sample of the batch has blur_sigma > 0 (two launches then), else NULL.                                                */
typedef struct mi355_crop {
  unsigned long long offset;
  int h, w, rh, rw, oy, ox, mirror, filter;
} mi355_crop;
typedef struct mi355_augment {
  float color[12];
  float blur_sigma;
  int gray, nbox, pad;
  int box[4][4];
} mi355_augment;
int mi355_ingest_u8(const unsigned char* packed, size_t packed_bytes, const mi355_crop* crops_host, const mi355_crop* crops_dev,
                    int N, int S, float mean, float std, float* out_nchw, void* stream);
int mi355_ingest_u8_aug(const unsigned char* packed, size_t packed_bytes, const mi355_crop* crops_host,
                        const mi355_crop* crops_dev, const mi355_augment* aug_host, const mi355_augment* aug_dev, int N, int S,
                        float mean, float std, float* scratch, float* out_nchw, void* stream);

/* fp8 (OCP e4m3fn) operand path of the convolution — BASELINE.json configs[4] "fp8 MFMA convs" (the reference has no fp8
 * path; the conv calls being replaced are the same as above, callbacks.py:316-317).  Per-tensor scaling:
 *   q = mi355_quantize_fp8(x * scale)  (saturating, round to nearest even; n a multiple of 8; source f32 or bf16)
 *   y_bf16 = conv(xq, wq) * oscale,  oscale = 1 / (scale_x * scale_w), fp32 accumulation on v_mfma_f32_16x16x32_fp8_fp8.
 * Layouts as above with 1-byte elements (x NHWC, w KRSC; dgrad takes the weights already transposed to [Cin][KH][KW][Cout]);
 * Cin and Cout multiples of 128, output width >= 2 (MI355_E_ARG otherwise: there is no second fp8 kernel to fall back on).
 * Same 8-wave kernel as the bf16 path with half the operand bytes (conv_igemm8.hip).   */
int mi355_quantize_fp8(int src_dtype, const void* x, void* q, float scale, size_t n, void* stream);
int mi355_conv2d_fwd_fp8(const void* xq, const void* wq, void* y, float oscale, int N, int H, int W, int Cin, int Cout,
                         int KH, int KW, int stride, int pad, void* stream);
int mi355_conv2d_dgrad_fp8(const void* dyq, const void* wtq, void* dx, float oscale, int N, int H, int W, int Cin,
                           int Cout, int KH, int KW, int stride, int pad, void* stream);
/* dw fp32 KRSC = beta * dw + oscale * sum_pixels dyq (x) xq over e4m3 operands (v_mfma_f32_32x32x16_fp8_fp8; both operands are read
 * TRANSPOSED out of LDS with ds_read_b64_tr_b8 — the reduction index, the pixel, is the slow index of both NHWC tensors).
 * ws: mi355_conv2d_workspace_bytes(MI355_BF16, ...) + 256 bytes.                                                                   */
int mi355_conv2d_wgrad_fp8(const void* dyq, const void* xq, float* dw, float beta, float oscale, int N, int H, int W, int Cin,
                           int Cout, int KH, int KW, int stride, int pad, void* ws, size_t ws_bytes, void* stream);

/* the 7x7/2 stem on the loader's NCHW fp32 batch: ingest (NCHW fp32 -> zero-padded NHWC4 `dtype`),
 * forward y[N,H/2,W/2,64], and wgrad dw[64,7,7,3] fp32.  xpad is scratch of
 * mi355_stem_xpad_bytes() bytes that must be ZEROED once by the caller before the first ingest.
 * replaces DALI's NCHW hand-off + cuDNN stem conv — dali_dataloader.py:113-122, callbacks.py:316 (K1) */
size_t mi355_stem_xpad_bytes(int dtype, int N, int H, int W);
int mi355_stem_ingest(int dtype, const float* x_nchw, void* xpad, int N, int H, int W, void* stream);
int mi355_stem_fwd(int dtype, const void* xpad, const float* w_krsc, void* y, int N, int H, int W,
                   void* ws, size_t ws_bytes, void* stream);
int mi355_stem_wgrad(int dtype, const void* dy, const void* xpad, float* dw, float beta, int N, int H,
                     int W, void* ws, size_t ws_bytes, void* stream);
size_t mi355_stem_workspace_bytes(int dtype, int N, int H, int W);

/* BatchNorm2d, training mode, over x[M,C] (M = N*H*W rows, NHWC):
 *   mean/var over M (biased var to normalise, unbiased into running_var), eps inside the sqrt,
 *   running = (1-momentum)*running + momentum*batch.   Outputs save_mean/save_invstd [C] for backward.
 *   out = act(x_hat*gamma + beta (+ residual)),   act by `relu`: 0 identity, 1 ReLU, 2 leaky ReLU (slope 0.01 — the
 *   `norm_act: leaky_relu` of the BResNet-50 configs, BResNet50_encoder.yaml:49-50; same codes in mi355_bn_bwd).
 *   ws: >= mi355_bn_workspace_bytes(C) bytes.  gamma, beta, the running statistics and every other per-channel vector of the
 *   mi355_bn_* calls: [C] floats; residual, out, dout, dz_out, dx: laid out like x.
 * replaces cuDNN BatchNormalizationForwardTraining + ATen relu/add — callbacks.py:316 (K3,K4);
 * momentum semantics: train.py:76 / arg_parser.py:132                                              */
size_t mi355_bn_workspace_bytes(int C);
int mi355_bn_fwd_train(int dtype, const void* x, const void* residual, void* out, const float* gamma,
                       const float* beta, float* running_mean, float* running_var, float* save_mean,
                       float* save_invstd, int M, int C, float eps, float momentum, int relu, void* ws,
                       size_t ws_bytes, void* stream);
/* inference mode: uses running stats */
/* the same from partial rows a conv epilogue left (mi355_conv2d_fwd_stats): no pass over x for the statistics; ws: 2*C floats */
int mi355_bn_fwd_train_partial(int dtype, const void* x, const void* residual, void* out, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, float* save_mean,
                               float* save_invstd, int M, int C, float eps, float momentum, int relu, const float* partial,
                               int nblk, void* ws, size_t ws_bytes, void* stream);
int mi355_bn_fwd_eval(int dtype, const void* x, const void* residual, void* out, const float* gamma,
                      const float* beta, const float* running_mean, const float* running_var, int M,
                      int C, float eps, int relu, void* ws, size_t ws_bytes, void* stream);
/* backward of out = act(bn(x) (+residual)):  dz = dout * [out>0] (if relu),  dx = bn_bwd(dz),
 * dgamma/dbeta fp32 (beta_acc=0 overwrite / 1 accumulate).  If dz_out != NULL the masked gradient is
 * also stored (it is the residual branch's gradient).
 * replaces cuDNN BN bwd + ATen threshold_backward — callbacks.py:317 (K8)                           */
int mi355_bn_bwd(int dtype, const void* dout, const void* out, const void* x, const float* gamma,
                 const float* save_mean, const float* save_invstd, void* dx, void* dz_out,
                 float* dgamma, float* dbeta, float beta_acc, int M, int C, int relu, void* ws,
                 size_t ws_bytes, void* stream);
/* Every mi355_bn_* call refuses a null required pointer (residual, dz_out and the running statistics of the training forward, as a pair, are
 * optional) and M < 1 with MI355_E_ARG before any launch.
 *
 * The two BatchNorm calls of the executors, per op (bn_apply / bn_backward of resnet_exec.cpp, without the e4m3 twin).
 * mi355_bn_apply: out = act(x * scale[c] + shift[c] (+ residual | + x2 * scale2[c] + shift2[c])) on GIVEN fp32 coefficients, each product-sum one
 *   fma, the sum rounded to dtype once.  relu: 0 / 1 / 2 as above.  bits (optional, relu != 0): [M][C/V] u8, V = 16 / sizeof(element) values per
 *   byte, bit e of byte (m, v) = (the sum before the activation > 0) of channel v * V + e — clear for 0 and -0; the upper bits of an fp32
 *   byte are zero.  MI355_E_ARG, never another form: residual together with x2; relu = 2 with bits and an addend; bits with relu = 0.
 * mi355_bn_bwd_bits: dz = g where the bit is set, else g * slope (relu 1: slope 0; 2: 0.01; 0: no mask, bits NULL), rounded to dtype only where
 *   dz_out stores it; dbeta = sum dz, dgamma = sum dz * x_hat (beta_acc as above); dx = gamma * invstd * (dz - dbeta / M - x_hat * dgamma / M).
 *   partial / nblk: [nblk][2][C] fp32 rows of (sum dz, sum dz * x_hat) a fused data-gradient epilogue left (mi355_conv2d_dgrad_bn): the reduce
 *   pass is skipped — unless dz_out is given, which needs that pass; NULL / 0: the call reduces itself.  dx may alias g, dz_out may alias g.
 *   ws: >= mi355_bn_workspace_bytes(C) bytes.                                                                                               */
int mi355_bn_apply(int dtype, const void* x, const float* scale, const float* shift, const void* residual, const void* x2,
                   const float* scale2, const float* shift2, void* out, uint8_t* bits, int M, int C, int relu, void* stream);
int mi355_bn_bwd_bits(int dtype, const void* g, const uint8_t* bits, const void* x, const float* gamma, const float* mean,
                      const float* invstd, void* dx, void* dz_out, float* dgamma, float* dbeta, float beta_acc, int M, int C, int relu,
                      const float* partial, int nblk, void* ws, size_t ws_bytes, void* stream);

/* MaxPool 3x3 stride 2 pad 1 on NHWC; idx[N,Ho,Wo,C] uint8 = window position of the first maximum.  H, W even: Ho = H/2, Wo = W/2,
 * y and dy [N,Ho,Wo,C] like idx.
 * replaces ATen max_pool2d_with_indices fwd/bwd — callbacks.py:316-317 (K5)                         */
int mi355_maxpool_fwd(int dtype, const void* x, void* y, uint8_t* idx, int N, int H, int W, int C,
                      void* stream);
int mi355_maxpool_bwd(int dtype, const void* dy, const uint8_t* idx, void* dx, int N, int H, int W,
                      int C, void* stream);

/* The stem tail of the ResNet-50 executor, per op (what forward / backward_stem of resnet_exec.cpp launch).
 * Forward: p[N,H/2,W/2,C] = maxpool3x3/2/pad1(relu(y * scale[c] + shift[c])) from the raw conv output y[N,H,W,C] — the activation is
 *   rounded to dtype before the maximum and never stored; idx[N,H/2,W/2,C] u8 = kh * 3 + kw of the first maximum of the window in
 *   row-major scan order (in-image taps only, as mi355_maxpool_fwd); bits[N,H,W,C/V] u8, V = 16 / sizeof(element) values per byte:
 *   bit e of byte (n, h, w, v) = (y * scale + shift > 0) of channel v * V + e.  H, W even, C a multiple of 8.
 *   form  0: the launcher's own rule — what the executor runs (3 for bf16 with even H/2 and W/2 unless MI355_POOL_KEYS=0,
 *            2 for any other dtype / knob at such a shape, else 1)
 *         1: one thread per window;  2: one thread per 2 x 2 block of windows (H/2, W/2 even);
 *         3: packed (value, tap) integer keys (bf16, H/2, W/2 even); its bit is (stored value != 0), which differs from forms
 *            1 and 2 only for positive values below 2^-134.  NaN inputs: forms 1 and 2 propagate them, form 3 does not.
 *   A form the shape or dtype does not allow is MI355_E_ARG before any launch (never silently another form).
 * Backward: from dp[N,H/2,W/2,C], the gradient wrt p: g = the max pool's backward under idx (a pixel adds its windows in (oh, ow)
 *   order in fp32, the sum is rounded to dtype), zeroed where its bit is clear; then BatchNorm backward on y with the saved
 *   mean / invstd: dbeta = sum g, dgamma = sum g * x_hat (beta_acc = 0 overwrite / 1 accumulate), dx[N,H,W,C] = gamma * invstd *
 *   (g - dbeta / M - x_hat * dgamma / M), M = N*H*W.  The pool gradient at full resolution is never stored.
 *   C = 64, H, W even, N*H*W*C*sizeof(element) below 2^32 - 16 (32-bit buffer offsets); ws >= mi355_bn_workspace_bytes(C) bytes.
 * replaces cuDNN BN fwd/bwd + ATen relu / max_pool2d_with_indices fwd/bwd on the stem — callbacks.py:316-317 (K3-K5, K8) */
int mi355_bn_relu_maxpool(int dtype, const void* y, const float* scale, const float* shift, void* p, uint8_t* idx, uint8_t* bits,
                          int N, int H, int W, int C, int form, void* stream);
int mi355_stem_bwd(int dtype, const void* dp, const uint8_t* idx, const uint8_t* bits, const void* y, const float* gamma,
                   const float* mean, const float* invstd, void* dx, float* dgamma, float* dbeta, float beta_acc, int N, int H,
                   int W, int C, void* ws, size_t ws_bytes, void* stream);

/* global average pool x[N,HW,C] -> pooled[N,C] fp32, and its backward (broadcast of dpooled/HW).
 * replaces ATen mean / its backward — callbacks.py:316-317 (K6)                                     */
int mi355_gap_fwd(int dtype, const void* x, float* pooled, int N, int HW, int C, void* stream);
int mi355_gap_bwd(int dtype, const float* dpooled, void* dx, int N, int HW, int C, void* stream);

/* label-smoothed softmax cross-entropy on float (one-hot or soft) targets, reduction = mean:
 *   loss = mean_n[ (1-s) * -(sum_c y*logp) + s * -(mean_c logp) ],  logp = log_softmax(logits)
 *   dlogits = d loss / d logits (already divided by N) times grad_scale.
 * logits, target, dlogits: [N][C] floats.  loss: 1 float on device.  row_loss: N floats of scratch.  dlogits may be NULL (evaluation).
 * replaces pytorch_tools.losses.smooth.CrossEntropyLoss — arg_parser.py:140-142, callbacks.py:316 (K7)*/
int mi355_ce_loss(const float* logits, const float* target, float smoothing, float grad_scale,
                  float* loss, float* row_loss, float* dlogits, int N, int C, void* stream);

/* fused SGD with momentum on a flat fp32 range (torch.optim.SGD semantics, dampening 0, no nesterov):
 *   g = g*grad_scale + wd*p;  m = mu*m + g;  p -= lr*m       (m must start at 0 => first step m = g)
 * replaces torch.optim._multi_tensor.SGD.step — arg_parser.py:136-138, callbacks.py:309 (K10)       */
int mi355_sgd_step(float* p, const float* g, float* m, size_t n, float lr, float momentum,
                   float weight_decay, float grad_scale, void* stream);
/* the same step + the exponential moving average of the updated parameters in the same pass:
 *   ema += (1 - ema_decay) * (p_new - ema)      (= ema_decay * ema + (1 - ema_decay) * p_new)
 * replaces pytorch_tools' ModelEma callback over the parameters (train.py:111-112, `ema_decay` of
 * configs/_old_configs/_first_attempts/BResNet50_encoder.yaml:59) when the optimizer steps every batch */
int mi355_sgd_step_ema(float* p, const float* g, float* m, float* ema, size_t n, float lr, float momentum,
                       float weight_decay, float grad_scale, float ema_decay, void* stream);

/* fused Adam / AdamW on a flat fp32 range (torch.optim.Adam / AdamW semantics, amsgrad and maximize off), in the operation
 * order of torch's _single_tensor_adam; p, m (exp_avg), v (exp_avg_sq) in place, g read-only:
 *   g = g*grad_scale;  decoupled (AdamW): p *= 1 - lr*wd  |  else (Adam): g += wd*p      (both skipped when wd == 0)
 *   m = m + (1-beta1)*(g - m);  v = v*beta2 + (1-beta2)*g*g;  p -= step_size*m / (sqrt(v)/bc2_sqrt + eps)
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) for the range's step count t (t >= 1) are computed by the
 * caller in double, as torch does; beta1, beta2, lr and wd are doubles so that 1-beta and 1-lr*wd round as in torch.
 * Fails (-1) on a null or non-16-byte-aligned pointer, beta outside [0, 1), eps negative or not finite.
 * replaces torch.optim._multi_tensor.AdamW.step — train.py:92, configs/hydra_exp/5.r50_base_adamw_high-aug.yaml:17-20 */
int mi355_adam_step(float* p, const float* g, float* m, float* v, size_t n, double beta1, double beta2, float eps,
                    float step_size, float bc2_sqrt, double lr, double weight_decay, int decoupled, float grad_scale,
                    void* stream);
/* the same step + the moving average of the updated parameters in the same pass (ema_decay in [0, 1]):
 *   ema += (1 - ema_decay) * (p_new - ema)       replaces the ModelEma callback's lerp (train.py:111-112) under AdamW */
int mi355_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, double beta1, double beta2,
                        float eps, float step_size, float bc2_sqrt, double lr, double weight_decay, int decoupled,
                        float grad_scale, float ema_decay, void* stream);

/* fused MADGRAD on a flat fp32 range: src.optimizers.MADGRAD.step of the reference (sota_imagenet/optimizers.py:726-767,
 * configs/hydra_exp/54.r50_madgrad.yaml:21), in its operation order; p, grad_sum_sq, s in place, g and x0 read-only:
 *   g = g*grad_scale;  grad_sum_sq += lamb*g*g;  rms = cbrt(grad_sum_sq) + eps;  s += lamb*g;  z = x0 - s/rms
 *   p = p*momentum + (1 - momentum)*z;  p *= 1 - weight_decay          (decoupled and not scaled by lr, as the reference has it)
 * lamb = (lr + eps) * sqrt(k + 1) is formed here in double from the optimizer's global counter k (state["k"] BEFORE its increment).
 * x0 holds the parameters as they were before the first step; grad_sum_sq and s start at 0.
 * Fails (-1) before any launch on a null or non-16-byte-aligned pointer, momentum outside [0, 1), eps / lr / weight_decay negative or
 * not finite, k < 0. */
int mi355_madgrad_step(float* p, const float* g, float* grad_sum_sq, float* s, const float* x0, size_t n, double lr, double momentum,
                       double weight_decay, double eps, int k, float grad_scale, void* stream);
/* the same step + the moving average of the updated parameters in the same pass (ema_decay in [0, 1]):
 *   ema += (1 - ema_decay) * (p_new - ema)       replaces the ModelEma callback's lerp (train.py:111-112) under MADGRAD */
int mi355_madgrad_step_ema(float* p, const float* g, float* grad_sum_sq, float* s, const float* x0, float* ema, size_t n, double lr,
                           double momentum, double weight_decay, double eps, int k, float grad_scale, float ema_decay, void* stream);

/* AdaiS on flat fp32 ranges: src.optimizers.AdaiS.step of the reference (sota_imagenet/optimizers.py:569-639,
 * configs/hydra_exp/50.r50_adais.yaml:19), whose per-element momentum depends on a statistic of ALL parameters.  Three stages on one
 * stream, nothing read back by the host; `step` is the range's count after this step's increment (>= 1), bc2 = 1 - beta2^step:
 *  (a) mi355_adais_moments, once per range (optimizers.py:592-602):  g = g*grad_scale;  v = v*beta2 + (1 - beta2)*g*g  in place, and
 *      one double per workgroup — the sum of its elements' v / bc2 — into `workspace` (mi355_adais_workspace_bytes(n) bytes, 8-byte
 *      aligned).  No floating-point atomics; the number of workgroups depends on n alone, so the sums are reproducible bit for bit.
 *  (b) mi355_adais_mean, once per optimizer step (optimizers.py:605):  mean[0] = (sum of the workspace_bytes / 8 doubles of all ranges,
 *      laid out back to back, in a fixed order) / param_size.  param_size counts real parameter elements only: padding inside a range
 *      must hold v = 0 so that it adds nothing.
 *  (c) mi355_adais_step, once per range (optimizers.py:607-639), reading mean[0] from device memory; p, m, beta1_prod in place:
 *        p *= 1 - lr*weight_decay  (only when weight_decay != 0);   beta1 = clamp(1 - (v/bc2)/mean*beta0, 0, 1 - eps)
 *        beta1_prod *= beta1;   m = m*beta1 + (1 - beta1)*g;   p -= lr * m / (1 - beta1_prod)
 * v starts at ema_norm_init (1e-3), beta1_prod at 1, m at 0.
 * Each fails (-1) before any launch on a null or misaligned pointer (16 bytes for the element arrays), beta2 outside [0, 1),
 * step < 1, beta0 / eps / lr / weight_decay negative or not finite, an empty workspace or param_size = 0. */
size_t mi355_adais_workspace_bytes(size_t n);
int mi355_adais_moments(const float* g, float* v, size_t n, double beta2, int step, float grad_scale, void* workspace, void* stream);
int mi355_adais_mean(const void* workspace, size_t workspace_bytes, size_t param_size, float* mean, void* stream);
int mi355_adais_step(float* p, const float* g, float* m, const float* v, float* beta1_prod, const float* mean, size_t n, double lr,
                     double beta0, double beta2, double eps, double weight_decay, int step, float grad_scale, void* stream);
/* stage (c) + the moving average of the updated parameters in the same pass:  ema += (1 - ema_decay) * (p_new - ema) */
int mi355_adais_step_ema(float* p, const float* g, float* m, const float* v, float* beta1_prod, const float* mean, float* ema, size_t n,
                         double lr, double beta0, double beta2, double eps, double weight_decay, int step, float grad_scale,
                         float ema_decay, void* stream);

/* The layer-wise optimizers of the reference's own tree on flat fp32 arrays: MyNovograd (sota_imagenet/optimizers.py:35-161, recipe
 * configs/hydra_exp/47.r50_my-nov.yaml), NovogradApex (:189-290, 46.r50_nov.yaml), AdamLayerwise (:293-397, 49.r50_nov-adam.yaml) and
 * MyAdai (:400-519, 55.r50_adai_2.yaml).  Each uses ONE statistic per parameter tensor (the sum of squares of its gradient; of the
 * parameter itself for MyNovograd, :138) as a per-tensor scalar of the update.  Three stages on one stream, nothing read back, over two
 * tables of 16-byte records in device memory that the caller builds once per plan:
 *   items[]   { int64 off; int32 len; int32 tensor }   len <= mi355_lw_item_elems(), off a multiple of 4, cut from ONE tensor's own range
 *   tensors[] { int32 first; int32 count; double numel }   the tensor's consecutive items (= its entries of partial[])
 * A record that does not lie inside the arrays of the launch is skipped by the kernels.
 *  (a) mi355_lw_sumsq, once per (parameter, gradient) storage pair: partial[i] = sum over items[i] of (src*scale)^2, the product in float,
 *      the square and the sum in double, in a fixed order (no floating-point atomics).  Replaces grad.pow(2).sum() / .mean() per tensor
 *      (:138, :270, :369, :488 — the last with an .item() host sync).
 *  (b) mi355_lw_coef, once per param group: S = the tensor's partials summed in a fixed order -> sums[t]; stat = S, or S/numel with
 *      flag 1 (MEAN).  In double, rounded once on store into coef[t] = (den, beta1, gw, wdf):
 *        rule 0 (AdamLayerwise, NovogradApex) and rule 1 (MyNovograd), v = float32[n_tensors], updated in place (:140-146, :273-274, :370-371):
 *          v = v*beta2 + (1 - beta2)*stat;  den = sqrt(v) + eps;  gw = 1 - beta1
 *          wdf = 1 - lr*wd;  flag 2 (STABLE_WD): 1 - lr*wd/den (:388);  flag 4 (SOFT_WD, NovogradApex's wd_eps): lr*wd (:288)
 *        rule 2 (MyAdai, :487-517), v = double[n_tensors] READ ONLY — the class never writes its second moment back into its state —
 *          and `mean` the mean of those constants (:459), `beta1` the group's beta0:
 *          vt = v*beta2 + stat*(1 - beta2);  r = vt/mean (flag 16 SQRT_MOM: sqrt(r));  beta1 = clip(1 - r*beta0, 0, 1 - eps)
 *          gw = 1 - beta1, or 1 with flag 8 (SGD_MOM);  wdf = 1 - lr*wd;  flag 2: 1 - lr*wd/(1 - beta1)
 *  (c) mi355_lw_update, once per param group over that group's items; p, m in place, g read-only (:144-159, :277-288, :374-391, :504-517):
 *        g = g*grad_scale
 *        rule 0:  m = m*beta1 + gw*(g/den);  p += -lr*m        rule 1:  m = m*beta1 + gw*g;  p += -lr*(m/den)
 *        rule 2:  m = m*beta1 + gw*g;        p += -lr*m
 *        p *= wdf;   with soft_wd (rule 0 only):  p -= wdf * max(|p| - wd_eps, 0) * sign(p)
 *      mi355_lw_update_ema: + ema += (1 - ema_decay) * (p_new - ema) in the same pass (train.py:111-112).
 * p, g, m, ema are the arrays the item offsets count from, n their length.  Each fails (-1) before any launch on a null or misaligned
 * pointer (16 bytes for the arrays, the tables and coef), an empty table, a rule outside 0..2, betas outside [0, 1), eps / lr negative or not
 * finite. */
size_t mi355_lw_item_elems(void);
int mi355_lw_sumsq(const float* src, size_t n, const void* items, size_t n_items, int n_tensors, float scale, void* partial, void* stream);
int mi355_lw_coef(int rule, int flags, const void* partial, size_t n_partial, const void* tensors, size_t n_tensors, void* v, float* coef,
                  void* sums, double beta1, double beta2, double eps, double lr, double weight_decay, double mean, void* stream);
int mi355_lw_update(int rule, float* p, const float* g, float* m, size_t n, const void* items, size_t n_items, const float* coef, int n_tensors,
                    double lr, int soft_wd, double wd_eps, float grad_scale, void* stream);
int mi355_lw_update_ema(int rule, float* p, const float* g, float* m, float* ema, size_t n, const void* items, size_t n_items, const float* coef,
                        int n_tensors, double lr, int soft_wd, double wd_eps, float grad_scale, float ema_decay, void* stream);

/* unitwise_norm=True of MyNovograd and NovogradApex (sota_imagenet/optimizers.py:16-22, :134-135, :267-268; recipe
 * configs/hydra_exp/48.r50_my-nov-unit.yaml) on flat fp32 arrays.  The statistic is taken per SLOT: a whole tensor for tensors with ndim <= 1,
 * one index of dim 0 otherwise (a filter of a conv, a row of the FC: a contiguous run of unit_len = numel / shape[0] elements).  It is the NORM,
 * sqrt of the sum of squares — also for the 1-D tensors — where the layer-wise rule above takes the sum of squares itself.  With x = g*grad_scale
 * (NovogradApex, rule 0) or x = the PARAMETER (MyNovograd, rule 1, :135), per slot:
 *   S = sum of (double)x^2;  v = v*beta2 + (1 - beta2)*sqrt(S)  in double, rounded once to the float32 v[slot];  den = (float)(sqrt((double)v) + eps)
 * Stages on one stream, nothing read back, no floating-point atomics, over items[] of the layer-wise optimizers above (all tensors) and the tables
 * of the SAM callback below:
 *   pieces[]   { int64 off; int32 len; int32 slot }        len <= mi355_lw_item_elems(), off ANY element offset, cut from ONE unit
 *   slots[]    { int32 first; int32 count }                the slot's consecutive entries of partial[]
 *   tensors[]  { int64 start; int32 unit_len; int32 slot0 }   indexed by items[].tensor
 *  (a) mi355_lw_unit_sumsq, once per storage pair over the pieces of the unit slots: partial[i] = sum over pieces[i] of (src*scale)^2, the product
 *      in float, square and sum in double in a fixed order; one wave per piece.  The whole-tensor slots go through mi355_lw_sumsq over their items.
 *  (b) mi355_lw_unit_coef, once per param group over its (consecutive) slots: sums[slot] = S, the slot's entries of partial[] in a fixed order;
 *      v[slot] updated in place; den[slot] as above.  v, den, sums are indexed like slots[] (the pointers of the group's first slot).
 *  (c) mi355_lw_unit_update, once per param group over that group's items; p, m in place, g read-only, den[] the WHOLE array, n_slots its length:
 *        g = g*grad_scale;  den = den[tensors[t].slot0 + (element offset inside tensor t) / tensors[t].unit_len]
 *        rule 0:  m = m*beta1 + (1 - beta1)*(g/den);  p += -lr*m;      p *= 1 - lr*wd,  or with soft_wd  p -= lr*wd * max(|p| - wd_eps, 0) * sign(p)
 *        rule 1:  m = m*beta1 + (1 - beta1)*g;        p += -lr*(m/den);  p *= 1 - lr*wd
 *      beta1, 1 - beta1, -lr and 1 - lr*wd (lr*wd with soft_wd) are formed in double and rounded once to float32; the element update is float32.
 *      mi355_lw_unit_update_ema: + ema += (1 - ema_decay) * (p_new - ema) in the same pass.
 * A record that does not lie inside the arrays of the launch is skipped by the kernels.  Each fails (-1) before any launch on a null or
 * misaligned pointer (16 bytes for the arrays, items[], pieces[] and tensors[], 8 for partial[], slots[] and sums[], 4 for v[] and den[]), an
 * empty table, a rule outside 0..1, beta1 / beta2 outside [0, 1), eps or lr negative or not finite, scale / grad_scale not finite, soft_wd with
 * rule 1. */
int mi355_lw_unit_sumsq(const float* src, size_t n, const void* pieces, size_t n_pieces, int n_slots, float scale, void* partial, void* stream);
int mi355_lw_unit_coef(const void* partial, size_t n_partial, const void* slots, size_t n_slots, float* v, float* den, void* sums, double beta2,
                       double eps, void* stream);
int mi355_lw_unit_update(int rule, float* p, const float* g, float* m, size_t n, const void* items, size_t n_items, const void* tensors,
                         int n_tensors, const float* den, size_t n_slots, double beta1, double lr, double weight_decay, int soft_wd, double wd_eps,
                         float grad_scale, void* stream);
int mi355_lw_unit_update_ema(int rule, float* p, const float* g, float* m, float* ema, size_t n, const void* items, size_t n_items,
                             const void* tensors, int n_tensors, const float* den, size_t n_slots, double beta1, double lr, double weight_decay,
                             int soft_wd, double wd_eps, float grad_scale, float ema_decay, void* stream);

/* AdamP (`_target_: adamp.AdamP`, the reference's recipes configs/hydra_exp/51.r50_adamp.yaml:19-22 and 52.r50_adamp_low-eps.yaml:20-23) on
 * flat fp32 arrays: Adam whose update loses its component along the weight, and whose weight decay is scaled by wd_ratio, where gradient and weight
 * are nearly orthogonal.  PROVENANCE: the `adamp` package is neither part of the reference tree nor available where this was written; the rule
 * is the published adamp.AdamP.step (package 0.3.0) written down from memory of the public package, and parity is against a torch restatement of
 * it (tests/adamp_common.py), UNPINNED against the package itself.  pytorch_tools.optim.adamp.AdamP (recipes 12, 13) is a modified variant whose
 * code is not available and stays unresolved.  Per tensor, with bc1 = 1 - beta1^step, bc2 = 1 - beta2^step and ge = g*grad_scale:
 *   m = beta1*m + (1 - beta1)*ge;  v = beta2*v + ((1 - beta2)*ge)*ge;  den = sqrt(v)/sqrt(bc2) + eps;  u = m/den
 *                                                                      (nesterov: u = (beta1*m + (1 - beta1)*ge)/den)
 *   ndim > 1: for rows = the output units (one index of dim 0), then for the whole tensor as one row:
 *               cos = |sum(ge*p)| / (max(||ge||, eps) * max(||p||, eps)) per row;  if max over the rows < delta / sqrt(row length):
 *                 d = ||p||_row + eps;  u = u - (p/d) * (sum over the row of (p/d)*u);  ratio = wd_ratio;  stop
 *   p = p*(1 - lr*wd*ratio)  (wd > 0);   p = p + (-lr/bc1)*u        (ratio = 1 without a projection; the projection uses p before the decay)
 * Three stages on one stream, nothing read back, no floating-point atomics, over items[], pieces[], slots[] and tensors[] of the unit-wise
 * optimizers above (every tensor with ndim > 1 taken unit by unit, every other tensor one whole slot) and
 *   decide[]  { int32 slot0; int32 n_slots; int32 unit_len; int32 kind }   per tensor; kind 1: ndim > 1, 0: any other tensor
 * The element arithmetic is float32, one rounding per operation, written once for (a) and (c); beta1, 1 - beta1, beta2, 1 - beta2, sqrt(bc2) and
 * -lr/bc1 are formed in double and rounded once.
 *  (a) mi355_adamp_unit_sums, once per storage pair and param group over the pieces of its ndim > 1 tensors; reads p, g, m, v and writes none of
 *      them: u from the OLD m, v in registers, partial[4k .. 4k+3] = sums over pieces[k] of (ge^2, p^2, ge*p, p*u), operands converted to double
 *      before the product, in a fixed order; one wave per piece.
 *  (b) mi355_adamp_coef, once per param group, one workgroup per record of decide[] (the group's slice; coef[] and slots[] are the WHOLE arrays,
 *      wdf[] and mode[] the group's slices), in double: the slot sums = the slot's entries of partial[] in a fixed order, the layer sums = the slot
 *      sums in a fixed order;  mode 1 (the units) if max cos_slot < delta/sqrt(unit_len): coef[slot] = (d, s) = (sqrt(Spp) + eps, Spu/(sqrt(Spp) + eps))
 *      per slot;  else mode 2 (the layer) if cos_layer < delta/sqrt(n_slots*unit_len): every slot gets the layer's (d, s);  else mode 0 and (1, 0),
 *      as for kind 0.  wdf[t] = (float)(1 - lr*wd*(mode ? wd_ratio : 1)), exactly 1 for wd <= 0;  mode[t] = mode.
 *      s = sum(p*u)/d where the rule above has sum((p/d)*u): a deliberate rounding-level deviation that saves a second reduction pass.
 *  (c) mi355_adamp_update, once per storage pair and param group over that group's items; p, m, v in place, g read-only:
 *        (m, v, u) as in (a);  pn = p/d;  u = u - pn*s;  p = p*wdf[t];  p = p + (float)(-lr/bc1)*u     with (d, s) = coef[slot],
 *        slot = tensors[t].slot0 + (element offset inside tensor t) / tensors[t].unit_len, element by element where an item spans units.
 *      mi355_adamp_update_ema: + ema += (1 - ema_decay) * (p_new - ema) in the same pass.
 * 16 B / element in (a) + 28 B / element in (c), 36 B with the average.  A record that does not lie inside the arrays of the launch is skipped by
 * the kernels.  Each fails (-1) before any launch on a null or misaligned pointer (16 bytes for the arrays and the 16-byte tables, 8 for
 * partial[], slots[] and coef[], 4 for wdf[] and mode[]), an empty table, betas outside [0, 1), eps / lr / delta / wd_ratio negative or not
 * finite, weight_decay not finite, step < 1, grad_scale not finite. */
int mi355_adamp_unit_sums(const float* p, const float* g, const float* m, const float* v, size_t n, const void* pieces, size_t n_pieces,
                          int n_slots, double beta1, double beta2, double eps, int step, int nesterov, float grad_scale, void* partial,
                          void* stream);
int mi355_adamp_coef(const void* partial, size_t n_partial, const void* slots, size_t n_slots, const void* decide, size_t n_tensors, float* coef,
                     float* wdf, int* mode, double lr, double weight_decay, double eps, double delta, double wd_ratio, void* stream);
int mi355_adamp_update(float* p, const float* g, float* m, float* v, size_t n, const void* items, size_t n_items, const void* tensors,
                       int n_tensors, const float* coef, size_t n_slots, const float* wdf, double lr, double beta1, double beta2, double eps,
                       int step, int nesterov, float grad_scale, void* stream);
int mi355_adamp_update_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, const void* items, size_t n_items,
                           const void* tensors, int n_tensors, const float* coef, size_t n_slots, const float* wdf, double lr, double beta1,
                           double beta2, double eps, int step, int nesterov, float grad_scale, float ema_decay, void* stream);

/* The SAMOriginal callback of the reference (adaptive sharpness-aware minimization, sota_imagenet/callbacks.py:279-337; recipe
 * configs/hydra_exp/49.r50_nov-adam.yaml:46-48) on flat fp32 arrays: between the first backward and the optimizer step every parameter moves
 * along its gradient, weighted by its own magnitude and normalised by ONE statistic of all tensors; after a second forward / backward there
 * it moves back.  Four stages on one stream, nothing read back, over the items[] table of the layer-wise optimizers above and
 *   kind[]  int32 per tensor, indexed by items[].tensor: 1 = weight (a Parameter with ndim > 1), 0 = any other tensor.
 * With ge = g*grad_scale (float):
 *  (a) mi355_sam_sumsq, once per (parameter, gradient) storage pair (:327-337, the per-tensor norms):  partial[i] = sum over items[i] of w^2,
 *      w = ge*max(|p|, eta) for weights, w = ge otherwise, w in float, the square and the sum in double in a fixed order (no atomics).
 *  (b) mi355_sam_scale, once per step over ALL partials of the step (:337 the norm of the norms and its clamp, :297 the division):
 *      norm = max(sqrt(sum of partial[]), 2e-5);  out[0] = (float)(rho/norm);  out[1] = (float)norm.
 *  (c) mi355_sam_perturb, once per storage pair (:298-306):  e = (max(p*p, eta)*ge)*out[0] for weights, e = ge*out[0] otherwise;
 *      eps = e;  p = p + e.   eps is an array of the caller laid out like p.
 *  (d) mi355_sam_restore, after the second backward (:319-323):  p = p - eps over the same items.
 * p, g, eps are the arrays the item offsets count from, n their length; elements outside the items (alignment gaps, padding) are neither read into
 * the sum nor written.  Each fails (-1) before any launch on a null or misaligned pointer (16 bytes for the arrays and the table, 8 for partial[]
 * and out[], 4 for kind[]), an empty table, rho not finite or <= 0, eta not finite or negative, grad_scale not finite. */
int mi355_sam_sumsq(const float* p, const float* g, size_t n, const void* items, size_t n_items, const int* kind, int n_tensors, float eta,
                    float grad_scale, void* partial, void* stream);
int mi355_sam_scale(const void* partial, size_t n_partial, double rho, float* out, void* stream);
int mi355_sam_perturb(float* p, const float* g, float* eps, size_t n, const void* items, size_t n_items, const int* kind, int n_tensors,
                      const float* out, float eta, float grad_scale, void* stream);
int mi355_sam_restore(float* p, const float* eps, size_t n, const void* items, size_t n_items, int n_tensors, void* stream);

/* The SAM callback of the reference (sota_imagenet/callbacks.py:339-420 with unitwise_norm :269-276; the form the recipes write down,
 * configs/hydra_exp/32.nf_conv-act_sam.yaml:104-106) on flat fp32 arrays: the perturbation is scaled slot by slot, eps = ||w|| / ||g|| * g * rho.
 * A slot is a whole tensor (:389-391), or with unitwise (:386-387) one output unit of a tensor with more than one dimension: one index of
 * dim 0, a contiguous run of unit_len = numel / shape[0] elements.  Stages on one stream, nothing read back, no floating-point atomics, over
 * the items[] table of the layer-wise optimizers above (all tensors) and
 *   pieces[]   { int64 off; int32 len; int32 slot }        len <= mi355_lw_item_elems(), off ANY element offset, cut from ONE unit
 *   slots[]    { int32 first; int32 count }                the slot's consecutive entries of partial[]
 *   tensors[]  { int64 start; int32 unit_len; int32 slot0 }   indexed by items[].tensor: the tensor's first element, elements per slot (numel
 *                                                          for a whole-tensor slot), the slot of its first element
 * partial[] holds a PAIR of doubles per entry: (sum of ge^2, sum of p^2), ge = g*grad_scale formed in float, squares and sums in double in a
 * fixed order.  A record that does not lie inside the arrays of the launch is skipped by the kernels.
 *  (a)  mi355_sam_lw_sumsq, once per storage pair over the items of the whole-tensor slots:  partial[i] = the pair of sums over items[i].
 *  (a') mi355_sam_unit_sumsq, once per storage pair over the pieces of the unit slots:  partial[i] = the pair of sums over pieces[i];
 *       threads_per_piece = 64 (one wave per piece, four pieces per workgroup: what the callback uses) or 256 (one workgroup per piece).
 *  (b)  mi355_sam_lw_coef, once per step over ALL slots:  (Sg, Sp) = the slot's entries of partial[] summed in a fixed order;
 *       gn = max((float)sqrt(Sg), 1e-5f);  wn = max((float)sqrt(Sp), 1e-3f)  (:367-368, :386-391);  coef[slot] = wn / gn  (:395);
 *       norms[slot] = (gn, wn).
 *  (c)  mi355_sam_lw_perturb, once per storage pair over ALL its items (:396-404):  e = (coef[slot] * ge) * (float)rho;  eps = e;  p = p + e,
 *       slot = tensors[t].slot0 + (element offset inside tensor t) / tensors[t].unit_len, element by element where an item spans units.
 *  (d)  mi355_sam_restore above, after the second backward (:418).
 * p, g, eps are the arrays the offsets count from, n their length; elements outside the tables are neither read into a sum nor written.  Each
 * fails (-1) before any launch on a null or misaligned pointer (16 bytes for the arrays, items[], pieces[], tensors[] and partial[], 8 for
 * slots[] and norms[], 4 for coef[]), an empty table, rho not finite or negative (0 is legal: the recipes write rho: 0), grad_scale not finite,
 * threads_per_piece other than 64 or 256. */
int mi355_sam_lw_sumsq(const float* p, const float* g, size_t n, const void* items, size_t n_items, int n_tensors, float grad_scale, void* partial,
                       void* stream);
int mi355_sam_unit_sumsq(const float* p, const float* g, size_t n, const void* pieces, size_t n_pieces, int n_slots, float grad_scale,
                         void* partial, int threads_per_piece, void* stream);
int mi355_sam_lw_coef(const void* partial, size_t n_partial, const void* slots, size_t n_slots, float* coef, float* norms, void* stream);
int mi355_sam_lw_perturb(float* p, const float* g, float* eps, size_t n, const void* items, size_t n_items, const void* tensors, int n_tensors,
                         const float* coef, size_t n_slots, double rho, float grad_scale, void* stream);

/* Orthogonal initialisation: the reference's `src.callbacks.OrthoInitClb` (sota_imagenet/callbacks.py:250-266, torch.nn.init.orthogonal_ on every
 * nn.Conv2d / nn.Linear weight; recipes 46-48, 50-53, 55) over a flat fp32 array — csrc/init_ortho.hip.  The caller fills the matrices with N(0,1)
 * draws; one launch turns every matrix of the table, in place, into the Q of its QR factorisation with a positive diagonal of R, times gain.
 *   mats[]  { int64 off; int32 rows; int32 chans; int32 taps; int32 pad }   24 bytes;  cols = chans * taps
 *           logical element M[r][ci*taps + t] lives at w[off + r*cols + t*chans + ci]   (taps == 1: plain row-major [rows][cols], an FC weight;
 *           taps > 1: a conv weight [rows = Cout][taps = KH*KW][chans = Cin], KRSC memory under the logical [Cout][Cin*KH*KW] matrix)
 * Per record, as orthogonal_ does (transpose when rows < cols, qr, Q *= sign(diag R), transpose back):
 *   rows < cols   the vectors are the rows, in order r = 0, 1, ...
 *   otherwise     the vectors are the columns, in LOGICAL order c = ci*taps + t (not memory order when taps > 1)
 *   each vector loses its components along all earlier vectors and is normalised (Gram-Schmidt, every vector projected twice, sums in double in a
 *   fixed order, no floating-point atomics: two runs on the same input agree bit for bit); every stored element is then fl(q * gain), one float
 *   multiply, so gain == 1 stores q itself.  Elements outside the records (alignment gaps, the FC padding rows) are neither read nor written.
 * One workgroup per matrix, the matrices side by side, no workgroup waits on another.  Records must not overlap.  status[i] (device, n_mats ints):
 *   0  done
 *   1  a vector's residual norm was zero, non-finite or below 2^-12 of its norm before projection (rank-deficient input): that vector is zeroed,
 *      the vectors before it are orthonormal (gain not applied), the ones behind it keep their input — finite contents for finite input
 *   2  the record does not fit: off >= 0, rows, chans, taps >= 1 and off + rows*cols <= n are tested before anything is accessed through it;
 *      such a record is skipped and its memory untouched
 * Fails (-1) before the launch on a null or misaligned pointer (8 bytes for mats[], 4 for w and status[]), n == 0, an empty table, gain not finite. */
int mi355_ortho_init(float* w, size_t n, const void* mats, size_t n_mats, float gain, int* status, void* stream);

/* The log-histogram callback of the reference: `src.callbacks.GradDistributionTB` (sota_imagenet/callbacks.py:30-60; recipes 46, 49-55) over flat
 * fp32 arrays — csrc/optim_hist.hip.  The reference sorts |x| of every tensor, keeps every subsample-th value, sorts the concatenation, keeps every
 * subsample-th value again and draws a histogram of log10 of the rest.  The kept ranks 0, s, 2s, ... of a sorted tensor include exactly
 * ceil(c / s) values below a threshold, c the number of its elements below it, so the bin counts of the twice-subsampled set follow exactly from
 * per-tensor bin counts; no sort is made.  Integer arithmetic only: exact, and the same bit for bit in every run.
 *   bins     512 (csrc/absbin.h):  bin(x) = clamp((bits(x) with the sign cleared >> 20) - 618, 0, 511) — eight bins per octave, linear in the
 *            mantissa; bin 0 is everything below 2^-50 * 1.375 = 1.2212e-15 (zeros, denormals, all the reference clamps to -15), bin b >= 1
 *            starts at the float with bits (618 + b) << 20, bin 511 at 2^14 * 1.125 and also takes infinities and NaN.
 *   items[]  { int64 first; int32 len; int32 tensor }   the work-item table of the layer-wise optimizers above, len <= mi355_lw_item_elems(),
 *            but first may be ANY element offset (a state stored once per tensor or per output unit starts anywhere)
 *  mi355_absbin_hist ADDS the bin counts of the elements of items[i] into hist[items[i].tensor][512] (the caller zeroes the table; several
 *      launches — one per storage — fill one table): a workgroup histogram in LDS, then integer atomicAdd of its non-zero bins.  src is the array
 *      the offsets count from, n its length; elements outside the items (alignment gaps, the FC padding rows) are never read into a count, and a
 *      record that does not lie inside [0, n), or whose tensor is not in [0, n_tensors), is skipped.  Fails (-1) before any launch on a null or
 *      misaligned pointer (16 bytes for src, items[] and hist[]) or an empty table.
 *  mi355_subsample_counts, one workgroup:  c_t(k) = rep[t] * (sum of hist[t][0..k-1]);  C(k) = sum over t of ceil(c_t(k) / subsample);
 *      counts[k] = ceil(C(k+1) / subsample) - ceil(C(k) / subsample) for k = 0..511, in 64 bits.  rep[t] >= 1 (device memory) counts a state that
 *      is stored once and shown broadcast: rep[t] = shown elements per stored element.  Fails (-1) before the launch on a null or misaligned
 *      pointer (16 bytes for hist[], 8 for counts[], 4 for rep[]), n_tensors < 1 or subsample < 1.  rep[] lives on the device and is not read
 *      back before the launch: if any rep[t] < 1 the kernel writes ~0 (no possible count) into all of counts[], for the caller to test where it
 *      reads counts[] anyway. */
int mi355_absbin_hist(const float* src, size_t n, const void* items, size_t n_items, int n_tensors, uint32_t* hist, void* stream);
int mi355_subsample_counts(const uint32_t* hist, const int32_t* rep, int n_tensors, int subsample, uint64_t* counts, void* stream);

/* The per-epoch weight histograms of the reference: `WeightDistributionTB` (sota_imagenet/callbacks.py:11-17, added by train.py:140 when
 * `log.histogram` is set: recipes 4, 11-14, 45-55), which hands every entry of model.state_dict() to
 * tb_logger.add_histogram("model/<name>", p.flatten(), global_sample_step) — csrc/optim_wdist.hip.  add_histogram with its defaults copies the
 * tensor to the host and runs np.histogram(values.astype(float64), bins) over TensorBoard's default bins, then takes min, max, sum and the sum
 * of squares in double.  mi355_tbbin_hist is that over the work items of one flat fp32 array, in one pass:
 *   edges[]    the 774 positive edges, ascending, as doubles in device memory: v = 1e-12, v *= 1.1 while v < 1e20, formed by the caller with this
 *              recurrence in double (the table is the rule; ops.tbbin_edges()[775:]).  The full table is their negatives reversed, 0, and they:
 *              1549 edges E_0..E_1548, 1548 bins; bin i is [E_i, E_i+1), the last one also takes x == E_1548.  Every comparison is made in double.
 *   items[]    { int64 first; int32 len; int32 tensor }, len <= mi355_lw_item_elems(), first ANY element offset (as for mi355_absbin_hist)
 *   hist[][]   uint32 [n_tensors][1552]: the counts of items[i] are ADDED into hist[items[i].tensor][0..1547] (the caller zeroes the table; several
 *              launches — one per storage — fill one table); entry 1548 counts the elements that np.histogram puts in no bin: NaN, both
 *              infinities, everything below E_0 or above E_1548; entries 1549..1551 pad the row to 16 bytes and stay untouched.
 *   partial[]  double [n_items][5]: { min, max, sum, sum of squares, 1.0 if a NaN was seen else 0.0 } of the item's elements; min and max skip
 *              NaN (+inf / -inf if the item holds nothing else), the sums take every element.  Fixed order inside the workgroup, no floating-point
 *              atomics: the caller adds a tensor's items in table order and gets the same bits in every run.
 * Elements outside the items are never read; a record that does not lie inside [0, n), or whose tensor is not in [0, n_tensors), is skipped and its
 * partial[] entry stays as it was.  Fails (MI355_E_ARG) before the launch on a null or misaligned pointer (16 bytes for src, items[] and hist[],
 * 8 for edges[] and partial[]), an empty table, n_tensors < 1 or n_edges != 774. */
int mi355_tbbin_hist(const float* src, size_t n, const void* items, size_t n_items, int n_tensors, const double* edges, int n_edges, uint32_t* hist,
                     double* partial, void* stream);

/* Backward centred weight normalisation: the reference's `src.callbacks.WeightNorm` (sota_imagenet/callbacks.py:104-123; recipes 9, 10, 14, 37-39),
 * which after every optimizer step takes every module weight of 64 elements or more as a [size(0), -1] matrix, subtracts each row's mean and divides
 * each row by its L2 norm — csrc/weight_norm.hip.  One launch over a table of rows of a flat fp32 array, in place:
 *   items[]  { int64 first; int32 row_len; int32 n_rows }   16 bytes: n_rows consecutive rows of row_len elements, the first one at w[first] (ANY
 *            element offset: the stem's rows are 147 long); a conv weight in KRSC memory and an FC weight alike, a row is one contiguous run
 * Per row x[0..L), every operation rounded on its own:
 *   S1 = sum (double)x_i;   m = (float)(S1 / (double)L);   c_i = x_i - m (float);   S2 = sum (double)c_i * (double)c_i;   nrm = (float)sqrt(S2);
 *   x_i = c_i / nrm (float division)
 *   the sums: per thread in element order, then a fixed tree; no floating-point atomics, nothing summed across workgroups — a row's result depends
 *   on its elements alone (not on the item that holds it), and two runs on the same input agree bit for bit.  A constant row gives 0 / 0: the whole
 *   row becomes NaN, as in the reference, and nothing outside it changes.
 * One 256-thread workgroup per item; rows of at most mi355_wnorm_wave_row_max() elements take one wave each, longer rows the whole workgroup (the
 * result does not depend on which, beyond the order of the sums).  Items must not overlap.  Elements outside the items (alignment gaps, BatchNorm
 * tensors, biases, the FC padding rows) are neither read nor written.  status[i] (device, n_items ints), written with ordinary stores:
 *   0  done
 *   2  the item does not fit: first >= 0, row_len >= 1, n_rows >= 1 and first + row_len*n_rows <= n are tested before anything is accessed through
 *      it; such an item is skipped and its memory untouched
 * Fails (-1) before the launch on a null or misaligned pointer (16 bytes for w and items[], 4 for status[]), n == 0 or an empty table. */
int mi355_weight_norm_rows(float* w, size_t n, const void* items, size_t n_items, int* status, void* stream);
int mi355_wnorm_wave_row_max(void);

/* Forward weight transform per output filter: the reference's `weight_standardization: True` (train.py:66-67) and its ForwardWeightNorm callback
 * (sota_imagenet/callbacks.py:62-84) — csrc/weight_std.hip.  The plain ResNet-50 executor runs these itself once
 * mi355_resnet50_set_weight_transform has switched it on; the entry points serve the per-row tests and the callback's bake.
 *   rows[]  { int64 off; int32 len; int32 reserved }   16 bytes: one filter, len contiguous elements from element `off` of the flat fp32 arrays
 *           (ANY element offset: the stem's rows are 147 long); row k of the table owns invstd[k]
 *   mode    1 standardise (MI355_WS_STANDARDISE), 2 centre (MI355_WS_CENTRE)
 * Forward, per row w[0..L), every operation rounded on its own:
 *   S1 = sum (double)w_i;  S2 = sum (double)w_i * (double)w_i;  mu = S1 / L;  var = max(S2 / L - mu * mu, 0);
 *   is = (float)(1 / sqrt(var + eps)) (mode 1) or 1 (mode 2);  w_hat_i = (w_i - (float)mu) * is (float);  invstd[k] = is
 *   the sums: per lane in element order, then a fixed tree; no floating-point atomics, nothing summed across waves — two runs on the same input
 *   agree bit for bit.  A constant row gives zeros and a finite invstd, never NaN.  w_hat may be w itself (the transform baked in place).
 * Backward, per row of the slice [row_begin, row_end) of the table, g = the gradient wrt w_hat:
 *   m1 = (float)(sum (double)g_i / L);  m2 = (float)(sum (double)g_i * (double)w_hat_i / L) (mode 1) or 0 (mode 2);
 *   dw_i = (beta != 0 ? beta * dw_i : 0) + invstd[k] * (g_i - m1 - w_hat_i * m2)          (mode 2: invstd[k] * (g_i - m1))
 * One wave per row, one launch per call.  A record that does not lie inside [0, n) is skipped (nothing read or written through it); elements
 * outside the rows are neither read nor written.  The table must hold every row the call names.  Fails (MI355_E_ARG) before the launch on a
 * null or misaligned pointer (16 bytes for the arrays and rows[], 4 for invstd[]), a mode other than 1 or 2, n == 0, an empty table or slice,
 * eps < 0, or (backward) dw being the array g or w_hat is read from. */
#define MI355_WS_STANDARDISE 1
#define MI355_WS_CENTRE 2
#define MI355_WS_EPS 1e-5f /* the eps of the executor's own forward: oracle/bresnet50_ref.py::ws */
int mi355_weight_std_rows_fwd(const float* w, float* w_hat, float* invstd, size_t n, const void* rows, size_t n_rows, int mode, float eps,
                              void* stream);
int mi355_weight_std_rows_bwd(const float* g, const float* w_hat, const float* invstd, float* dw, size_t n, const void* rows, size_t row_begin,
                              size_t row_end, int mode, float beta, void* stream);

/* Forward spectral normalisation per convolution: the reference's ForwardSpectralNorm callback (sota_imagenet/callbacks.py:87-101), i.e.
 * torch.nn.utils.parametrizations.spectral_norm with dim 0, one power iteration and eps 1e-12 — csrc/spectral_norm.hip.  The plain ResNet-50
 * executor runs these itself once mi355_resnet50_set_spectral_norm has switched it on; the entry points serve the per-matrix tests, the warm
 * start and the callback's bake.
 *   mats[]  { int64 off; int32 len; int32 rows; int64 u0; int64 v0 }   32 bytes: `rows` rows of `len` contiguous elements from element `off` of
 *           the flat fp32 arrays (ANY element offset); the matrix owns u[u0 .. u0 + rows), v[v0 .. v0 + len) (v in memory order: (K,K,Cin) for
 *           a conv filter) and sigma[its index].  u0 and v0 are the running sums of rows and len: they ascend with the index.
 * One power iteration, every sum in double and in a fixed order, every operation rounded on its own:
 *   t_r = sum_c W_rc v_c;  u_r = (float)(t_r / max(sqrt(sum_r t_r^2), eps));  s_c = sum_r W_rc u_r;  v_c = (float)(s_c / max(sqrt(sum_c s_c^2), eps));
 *   sigma = (float) sum_c s_c v_c
 * mi355_spectral_fwd runs `iters` of them (1: a training forward; up to MI355_SN_WARM_ITERS: the warm start); iters == 0 is the eval rule: u and v
 * are left as they are and sigma = (float) sum_r u_r t_r.  Then, unless w_hat is NULL, w_hat_rc = W_rc / sigma (w_hat == w: in place).  A zero
 * matrix has sigma = 0 and becomes NaN, as in torch.  4 launches per iteration (2 for eval) and one for the division, over all matrices.
 * mi355_spectral_bwd, from g = the gradient wrt w_hat, for the matrices whose rows are the slice [row_begin, row_end) of u[] (whole matrices:
 * one that the slice cuts is skipped), u, v, sigma constants:   d = sum_rc g_rc w_hat_rc;
 *   dw_rc = (beta != 0 ? beta * dw_rc : 0) + (g_rc - ((float)d * u_r) * v_c) / sigma                                   2 launches.
 * No floating-point atomics; no workgroup waits on another: every sum across workgroups is taken by one owner from what an earlier launch on
 * the same stream left in `scratch` (mi355_spectral_scratch_doubles(n_u, n_v) doubles).  A record that does not lie inside [0, n), [0, n_u) and
 * [0, n_v) is skipped (nothing read or written through it); elements outside the matrices are neither read nor written.  Fails (MI355_E_ARG)
 * before any launch on a null or misaligned pointer (16 bytes for the arrays, mats[] and scratch, 4 for u, v, sigma), n, n_u, n_v or n_mats
 * of 0, n_mats > 65535, iters outside 0 .. MI355_SN_WARM_ITERS, an empty slice or one beyond n_u, or (backward) dw being g or w_hat. */
#define MI355_SN_EPS 1e-12f
#define MI355_SN_WARM_ITERS 15 /* power iterations torch runs when the parametrisation is registered */
#define MI355_SN_SLABS 16      /* row slabs per matrix of the column sums */
size_t mi355_spectral_scratch_doubles(size_t n_u, size_t n_v);
int mi355_spectral_fwd(const float* w, float* w_hat, float* u, float* v, float* sigma, double* scratch, size_t n, size_t n_u, size_t n_v,
                       const void* mats, size_t n_mats, int iters, void* stream);
int mi355_spectral_bwd(const float* g, const float* w_hat, const float* u, const float* v, const float* sigma, float* dw, double* scratch, size_t n,
                       size_t n_u, size_t n_v, const void* mats, size_t n_mats, size_t row_begin, size_t row_end, float beta, void* stream);

/* Weight penalties in the loss — csrc/ortho_loss.hip: the reference's OrthoLoss, type 1 (sota_imagenet/callbacks.py:126-156, appended to the
 * criterion by OrthoLossClb, :191-203) and NormLoss (:206-221, NormLossClb :224-229), over the flat fp32 parameter array.  They always read the
 * raw parameters (the reference penalises parametrizations.weight.original).
 * OrthoLoss.  Per conv weight viewed as W [O, K] (O rows of K contiguous elements, O <= K):  G = W W^T - I,  F = |G|_F;  where F / O > min_norm
 * the loss takes F and the gradient (2 / F) G W (0 where F == 0); elsewhere nothing.
 *   mats[]   { int64 off; int32 len; int32 rows; int64 g0; int64 t0 }   32 bytes: `rows` = O rows of `len` = K elements from element `off` of the
 *            flat arrays (ANY element offset); the matrix owns gram[g0 .. g0 + O*O) and, with nt = ceil(O / MI355_OL_TILE), the tiles
 *            tiles[t0 .. t0 + nt (nt + 1) / 2): tile (ti, tj <= ti) at t0 + ti (ti + 1) / 2 + tj
 *   tiles[]  { int32 mat; int32 ti | tj << 16; int32 item0; int32 n_slabs }   16 bytes: n_slabs = ceil(K / MI355_OL_KSLAB) consecutive items
 *   items[]  { int32 tile; int32 slab }   8 bytes — item tiles[t].item0 + j is { t, j }
 *   gitems[] { int32 mat; int32 ti; int32 tc; int32 0 }   16 bytes: row tile ti and the tile of MI355_OL_TILE columns tc of K
 * mi355_ortho_loss_fwd, 3 launches: every item's partial tile (v_mfma_f32_32x32x2_f32: exact fp32, k ascending) -> partial[]; per tile, G = (the
 * slab partials added in slab order) - I, stored with its mirror, and the tile's sum of G^2 in double -> tile_ss[]; ONE workgroup: per matrix, in
 * tile order, F = (float)sqrt(sum), ratio = F / (float)O, gate = ratio > min_norm, coef = gate && F > 0 ? 2 / F : 0 ->
 * stats[4m ..] = { F, ratio, gate, coef } and *loss = (float) sum_m gate F (double, matrix order).
 * mi355_ortho_loss_bwd, 1 launch:  dw[r, c] = (accumulate ? dw[r, c] : 0) + (s[0] * coef) * sum_j G[r, j] W[j, c], j ascending inside one
 * workgroup; s is a DEVICE scalar (the upstream gradient times the callback's weight).  gram[] and stats[] as mi355_ortho_loss_fwd left them.
 * NormLoss.  Per tensor viewed as R rows:  loss += mean_r (1 - n_r)^2, n_r = |row r|_2 in double;  d/dw = (2 / R)(n_r - 1) / n_r w, 0 where n_r == 0.
 *   items[]   { int64 off; int32 len; int32 count }   16 bytes: `count` consecutive whole rows of ONE tensor (the row record of the row kernels)
 *   tensors[] { int64 item0; int32 n_items; int32 rows }   16 bytes: the tensor's consecutive items and its R; item0 ascends with the index
 * mi355_norm_loss_fwd, 2 launches: part[item] = sum_r (1 - n_r)^2; ONE workgroup: tensor_loss[k] = (its parts in item order) / R and
 * *loss = (float) sum_k tensor_loss[k] in tensor order.  mi355_norm_loss_bwd, 1 launch:
 *   dw = (accumulate ? dw : 0) + (float)(s[0] (2 / R)(n_r - 1) / n_r) * w.
 * Every sum across threads is double in a fixed order; no floating-point atomics, no workgroup waits on another, nothing is read back to the
 * host; two runs agree bit for bit.  A record that does not lie inside its arrays ([0, n), gram[n_gram], the tables), that has rows > len, or that
 * disagrees with the records it points to is SKIPPED, as mi355_spectral_fwd skips one: nothing is read or written through it and its
 * statistics are 0 — an item that does not name its tile and slab writes no partial, and a tile with such an item writes no G and counts 0.  Elements outside the matrices / rows are neither read nor written.  Scratch: partial[mi355_ortho_loss_partial_floats(n_items)],
 * tile_ss[n_tiles] doubles, stats[mi355_ortho_loss_stats_floats(n_mats)], gram[n_gram]; part[n_items] and tensor_loss[n_tensors] doubles.  All
 * launches run on `stream`.  Fails (MI355_E_ARG) before any launch on a null or misaligned pointer (16 bytes for the arrays, the 16- and 32-byte
 * tables and stats; 8 for items[] of the Gram pass and the doubles; 4 for loss and s), a size of 0, n_mats or n_tensors > 65535, a NaN
 * min_norm, or dw being w. */
#define MI355_OL_TILE 64   /* rows and columns of a Gram tile; columns of K per gradient item */
#define MI355_OL_KSLAB 512 /* elements of K per Gram item */
size_t mi355_ortho_loss_partial_floats(size_t n_items);
size_t mi355_ortho_loss_stats_floats(size_t n_mats);
int mi355_ortho_loss_fwd(const float* w, size_t n, float* gram, size_t n_gram, float* partial, double* tile_ss, float* stats, float* loss,
                         const void* mats, size_t n_mats, const void* tiles, size_t n_tiles, const void* items, size_t n_items, float min_norm,
                         void* stream);
int mi355_ortho_loss_bwd(const float* w, float* dw, size_t n, const float* gram, size_t n_gram, const float* stats, const float* s,
                         const void* mats, size_t n_mats, size_t n_tiles, const void* gitems, size_t n_gitems, int accumulate, void* stream);
int mi355_norm_loss_fwd(const float* w, size_t n, double* part, double* tensor_loss, float* loss, const void* items, size_t n_items,
                        const void* tensors, size_t n_tensors, void* stream);
int mi355_norm_loss_bwd(const float* w, float* dw, size_t n, const float* s, const void* items, size_t n_items, const void* tensors,
                        size_t n_tensors, int accumulate, void* stream);

/* ---- BResNet-50 variant blocks (BASELINE configs[3]) ---------------------------------------------------------------
 * The reference builds that model as pytorch_tools.models.resnet50(stem_type="deep", antialias=True, attn_type="eca",
 * norm_layer="inplaceabn", norm_act="leaky_relu", drop_rate=0.2, drop_connect_rate=0.2) —
 * configs/_old_configs/_first_attempts/BResNet50_encoder.yaml:41-51 — and wraps every conv in weight standardisation
 * (train.py:66-67).  Convolutions and BN reuse the entry points above; these are the additional ops, all NHWC.
 *   blurpool    3x3 binomial [1,2,1]x[1,2,1]/16, stride 2, reflect padding 1 (anti-aliased down-sampling); H, W even; y, dy [N][H/2][W/2][C]
 *               (as for avgpool2)
 *   avgpool2    2x2 average, stride 2 (the anti-aliased shortcut of a stride-2 block)
 *   maxpool3s1  3x3 max, stride 1, pad 1 + u8 argmax (first maximum in window scan order): the anti-aliased stem pool; y, idx, dy like x
 *   eca         y = x * sigmoid(conv1d_k(GAP(x)))[n][c]; k odd <= 9, zero padded over the channel axis.  pooled / gate
 *               [N][C] fp32 are outputs kept for backward; eca_bwd returns dx and the k conv-weight gradients
 *               (beta = 0 overwrite / 1 accumulate), ws = 2*N*C + 1152 floats of scratch
 *   weight_std  w_hat[o] = (w[o] - mean_o) * rsqrt(var_o + eps) over the K = KH*KW*Cin weights of output channel o
 *               (biased variance) and its backward dw = invstd * (g - mean(g) - w_hat * mean(g * w_hat)); mean, invstd: [Cout] floats,
 *               w_hat, dw_hat, dw: [Cout][K] like w
 *   residual_act  out = act(branch * scale_n[n] + shortcut): drop-connect keep/scale per sample (scale_n may be NULL),
 *               shortcut add (may be NULL), activation code as in mi355_bn_fwd_train; backward from `out`
 *   keep_scale  keep[i] = u_i >= p ? 1/(1-p) : 0 from a counter-based generator (seed, counter): the drop-connect
 *               sample scales and, multiplied onto the pooled features (mi355_mul_f32), dropout                     */
int mi355_blurpool_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, void* stream);
int mi355_blurpool_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int mi355_avgpool2_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, void* stream);
int mi355_avgpool2_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, void* stream);
int mi355_maxpool3s1_fwd(int dtype, const void* x, void* y, uint8_t* idx, int N, int H, int W, int C, void* stream);
int mi355_maxpool3s1_bwd(int dtype, const void* dy, const uint8_t* idx, void* dx, int N, int H, int W, int C,
                         void* stream);
int mi355_eca_fwd(int dtype, const void* x, const float* w, int k, void* y, float* pooled, float* gate, int N,
                  int HW, int C, void* stream);
int mi355_eca_bwd(int dtype, const void* dy, const void* x, const float* w, int k, const float* pooled,
                  const float* gate, void* dx, float* dw, float beta, float* ws, int N, int HW, int C, void* stream);
int mi355_weight_std_fwd(const float* w, float* w_hat, float* mean, float* invstd, int Cout, int K, float eps,
                         void* stream);
int mi355_weight_std_bwd(const float* dw_hat, const float* w_hat, const float* invstd, float* dw, float beta,
                         int Cout, int K, void* stream);
int mi355_residual_act_fwd(int dtype, const void* branch, const float* scale_n, const void* shortcut, void* out,
                           int N, size_t HWC, int act, void* stream);
int mi355_residual_act_bwd(int dtype, const void* dout, const void* out, const float* scale_n, void* dbranch,
                           void* dshortcut, int N, size_t HWC, int act, void* stream);
int mi355_keep_scale(float* keep, size_t n, float p, unsigned long long seed, unsigned long long counter,
                     void* stream);
int mi355_mul_f32(const float* a, const float* b, float* out, size_t n, void* stream);

/* Mixup / CutMix with the previous batch, on the device (CutmixMixup — sota_imagenet/callbacks.py:232-247; the
 * pytorch_tools Cutmix / Mixup bases it combines mix the batch with the PREVIOUS one under a random permutation).
 *   mi355_mix_sample  draws one batch's decisions on the device from (seed, counter): apply at all (probability `prob`),
 *                     CutMix or Mixup (coin, callbacks.py:242; `allow`: 1 Mixup only, 2 CutMix only, 3 both, 0 neither),
 *                     lambda ~ Beta(alpha, alpha), the CutMix box, a permutation of the N <= 1024 samples; the result
 *                     stays in `params` (mi355_mix_params_bytes(N) bytes of device memory: {int mode 0/1/2, float lambda,
 *                     int y1, y2, x1, x2, float box_area_fraction, int pad, int perm[N]}) — no host round trip.
 *   mi355_mix_apply   out / tout <- data[N,C,H,W] fp32 (the loader's NCHW batch) and target[N,classes] fp32 soft targets
 *                     mixed with prev_in / tprev_in under perm (out may alias data, tout target: in place); the UNMIXED
 *                     batch is stored to prev_out / tprev_out for the next step (double-buffered: pass the two buffers
 *                     in alternating roles).
 *                     Mixup: lambda*x + (1-lambda)*prev[perm]; CutMix: the box is pasted from prev[perm], the target
 *                     weights are the real box area.  W and classes must be multiples of 4.                         */
size_t mi355_mix_params_bytes(int N);
int mi355_mix_sample(void* params, unsigned long long seed, unsigned long long counter, int N, int H, int W,
                     float cutmix_alpha, float mixup_alpha, float prob, int allow, void* stream);
int mi355_mix_apply(const float* data, float* out, const float* prev_in, float* prev_out, const float* target,
                    float* tout, const float* tprev_in, float* tprev_out, const void* params, int N, int C, int H,
                    int W, int num_classes, void* stream);

/* ---- whole-network executor: torchvision-layout ResNet-50 v1.5 ----------------------------------
 * replaces hydra.utils.call(cfg.model) -> pytorch_tools.models.resnet50 (train.py:64,
 * configs/hydra_exp/1.r50_baseline.yaml:22-23) and everything autograd runs beneath it.            */
typedef struct mi355_ctx mi355_ctx;

/* N = per-GPU batch, H = W = image size (multiple of 32), dtype = activation/compute dtype of the convs
 * (accumulation, BN statistics, FC, loss and optimizer state are always fp32).
 * device < 0 creates a LAYOUT-ONLY ctx (no HIP call, no memory): the tensor table, flat sizes, segment
 * ranges and FLOP counts can be queried on a GPU-less host; bind/forward/backward fail with E_STATE.  */
int mi355_resnet50_create(mi355_ctx** out, int device, int dtype, int N, int H, int W, int num_classes);
int mi355_resnet50_destroy(mi355_ctx* ctx);

/* Parameter / buffer table (torchvision names).  Flat layouts are in REVERSE execution order (fc
 * first, stem last) so that gradient buckets complete front-to-back during backward.
 *   kind: 0 = parameter (offset into flat params/grads), 1 = buffer (offset into flat buffers:
 *         running_mean / running_var; num_batches_tracked is kept host-side by the caller).
 *   shape: torch logical shape (conv: [Cout,Cin,KH,KW], stored channels_last = KRSC), zero beyond ndim.
 *   name: a buffer of name_cap > 0 bytes is required; kind / offset / ndim / shape may be NULL.
 * The table queries, bind, segment_range, bucket_plan, set_comm and set_grad_sync of both executors (ResNet-50 here,
 * BResNet-50 below) share one implementation and one contract.                                      */
int mi355_resnet50_num_tensors(const mi355_ctx* ctx);
int mi355_resnet50_tensor_info(const mi355_ctx* ctx, int idx, char* name, int name_cap, int* kind,
                               size_t* offset, int* ndim, int shape[4]);
size_t mi355_resnet50_flat_param_elems(const mi355_ctx* ctx);  /* incl. alignment / FC row padding */
size_t mi355_resnet50_flat_buffer_elems(const mi355_ctx* ctx);
size_t mi355_resnet50_workspace_bytes(const mi355_ctx* ctx);

/* caller-owned flat fp32 device arrays; must outlive the ctx.  Padding elements must be zero.  All three are required and
 * 256-byte aligned (MI355_E_ARG otherwise); a layout-only ctx refuses to bind (MI355_E_STATE). */
int mi355_resnet50_bind(mi355_ctx* ctx, float* params, float* grads, float* buffers);

/* logits[N,num_classes] fp32 = model(x_nchw[N,3,H,W] fp32).  training!=0: batch statistics, running
 * stats updated with `bn_momentum`, activations saved for backward.  training==0: running stats.
 * Streams: the dependent kernel chain is issued to `stream`; independent work (weight gradients, the
 * downsample branch) goes to a side stream the ctx owns, forked from / joined to `stream` with events, so
 * on return everything is ordered on `stream` as if it had run there (MI355_WGRAD_STREAM=0 in the
 * environment at create time keeps every kernel on `stream`).  Results are bit-identical either way.
 * fp32 contexts cut the tiles of a partial last round along K across workgroups (stream-K, bounded spins).  Should a
 * hand-off ever time out, the kernel raises an error word that is copied to pinned host memory behind the kernels
 * of the call (no host wait): forward / backward / profile_read of that context then fail with MI355_E_STATE from
 * the first call that finds it set — at the latest the call after the next host-device synchronisation.          */
int mi355_resnet50_forward(mi355_ctx* ctx, const float* x_nchw, float* logits, int training,
                           float bn_momentum, void* stream);

/* Backward is split into mi355_resnet50_num_segments() segments (0 = fc, then one per bottleneck block
 * from layer4.2 down to layer1.0, last = stem) so the caller can launch a gradient all-reduce on a side
 * stream as soon as a segment's slice [grad_begin, grad_end) of the flat gradient array is complete.
 * Segments must be run in order 0..n-1 after a training forward.  Gradients OVERWRITE the flat array
 * (accumulate != 0: add into it, for accumulate_steps > 1 — arg_parser.py:85-86).  Every call ends by
 * joining the side stream: prefer one call per gradient bucket over one call per segment.            */
int mi355_resnet50_num_segments(const mi355_ctx* ctx);
int mi355_resnet50_segment_range(const mi355_ctx* ctx, int seg, size_t* grad_begin, size_t* grad_end);
int mi355_resnet50_backward(mi355_ctx* ctx, const float* dlogits, int seg_begin, int seg_end,
                            int accumulate, void* stream);


/* ---- BResNet-50 (BASELINE configs[3]) as a static executor — csrc/bresnet_exec.cpp -------------------------------------
 * The model the reference builds with `_target_: pytorch_tools.models.resnet50` and the model_params of
 * configs/_old_configs/_first_attempts/BResNet50_encoder.yaml:41-51 (deep stem, anti-aliasing, ECA, leaky-ReLU ABN, drop-connect,
 * dropout) + weight standardisation of every conv (train.py:66-67): one call per forward (train.py:64 `model(data)` under
 * callbacks.py:316) and one per backward (callbacks.py:317).  Same protocol as mi355_resnet50_*: create (device < 0: layout-only,
 * works without a GPU), tensor table (pytorch_tools names; kind 0 parameter / 1 buffer; conv weights logical [Cout,Cin,KH,KW] over
 * [Cout][KH][KW][Cin] memory; FC rows padded to a multiple of 128 inside the flat array), bind the three flat fp32 arrays, run.
 *   forward   training != 0: batch statistics, running stats updated with `bn_momentum`, everything backward needs is kept.
 *             Drop-connect / dropout (training only, rates from mi355_bresnet50_set_drop): block i > 0 scales its branch by
 *             keep_scale(N, rate * i / 16, seed, step * 64 + i), the pooled features by keep_scale(N * 2048, drop_rate, seed,
 *             step * 64 + 63) (mi355_keep_scale).  keep_override != NULL replaces the generator: 16 pointers, entry i = the [N]
 *             sample scales of block i or NULL (none); dropout_override = [N][2048] scales or NULL (none) — the test hook.
 *   backward  of the last training forward; accumulate != 0 adds to the flat gradient array.                                   */
typedef struct mi355_bctx mi355_bctx;
int mi355_bresnet50_create(mi355_bctx** out, int device, int dtype, int N, int H, int W, int num_classes, int weight_std);
int mi355_bresnet50_destroy(mi355_bctx* ctx);
int mi355_bresnet50_num_tensors(const mi355_bctx* ctx);
int mi355_bresnet50_tensor_info(const mi355_bctx* ctx, int idx, char* name, int name_cap, int* kind, size_t* offset, int* ndim,
                                int* shape);
size_t mi355_bresnet50_flat_param_elems(const mi355_bctx* ctx);
size_t mi355_bresnet50_flat_buffer_elems(const mi355_bctx* ctx);
size_t mi355_bresnet50_workspace_bytes(const mi355_bctx* ctx);
int mi355_bresnet50_bind(mi355_bctx* ctx, float* params, float* grads, float* buffers);
int mi355_bresnet50_set_drop(mi355_bctx* ctx, float drop_rate, float drop_connect_rate, unsigned long long seed);
int mi355_bresnet50_forward(mi355_bctx* ctx, const float* x_nchw, float* logits, int training, float bn_momentum,
                            unsigned long long step, const float* const* keep_override, const float* dropout_override,
                            void* stream);
int mi355_bresnet50_backward(mi355_bctx* ctx, const float* dlogits, int accumulate, void* stream);
int mi355_bresnet50_flops(const mi355_bctx* ctx, double* fwd_flops, double* train_flops);
/* Data parallelism of this executor (reference: DistributedDataParallel at /root/reference/train.py:113-114 around the configs[3] model):
 * the backward call runs mi355_bresnet50_num_segments() segments — 0 = the head, then the bottlenecks last to first, then the stem;
 * the flat gradient array is laid out in FORWARD (pytorch_tools registration) order, so the segments descend through it — and, with a
 * communicator attached, issues ONE mean all-reduce per bucket of consecutive segments (>= bucket_cap_mb MiB, the last bucket cut once
 * more: the rule of mi355_resnet50_set_comm, which both executors share) on the communicator's stream as soon as the bucket's last segment has been enqueued on
 * both streams; the caller's stream waits for the last one before the call returns.  set_grad_sync(0): no collective (DDP.no_sync()). */
typedef struct mi355_comm mi355_comm;
int mi355_bresnet50_num_segments(const mi355_bctx* ctx);
int mi355_bresnet50_segment_range(const mi355_bctx* ctx, int seg, size_t* grad_begin, size_t* grad_end);
int mi355_bresnet50_bucket_plan(const mi355_bctx* ctx, double bucket_cap_mb, int cap, int* n_out, size_t* begins, size_t* ends, int* last_segs);
int mi355_bresnet50_set_comm(mi355_bctx* ctx, mi355_comm* comm, double bucket_cap_mb);
int mi355_bresnet50_set_grad_sync(mi355_bctx* ctx, int on);

/* Test hook of the BResNet-50 executor (as mi355_resnet50_debug_tensor): device pointer / shape of a tensor of the last forward, by
 * name: "<conv>.y" (conv output, channels padded to a multiple of 64), "<bn>.out" (where the last forward stored it: bn3 / the
 * downsample BN are applied inside the fused ECA pass by default and have none), "<bn>.save_mean|save_invstd", "stem.p" (the
 * anti-aliased pool's output = layer1.0's input), "<block>.out|gate|keep|a2b|scin" (block output, ECA gate [N][C], drop-connect
 * scales [N] when sampled, blur-pooled a2 / average-pooled input of a striding block).  Read-only use.                             */
int mi355_bresnet50_debug_tensor(const mi355_bctx* ctx, const char* name, void** ptr, int* dtype, int* ndim, int shape[4]);
/* test hook of the NEXT mi355_bresnet50_backward call (cleared by it): for block i (0 = layer1.0 ... 15 = layer4.2), record[i] (device memory, the
 * size of that block's output in the compute dtype, or null) receives the gradient wrt the block's output the moment the block's backward starts,
 * and replay[i] (or null) overwrites that gradient first — teacher forcing between backward segments: two builds / switch settings fed the SAME
 * incoming gradient per block must agree per segment to rounding, where free-running backward passes amplify a last-bit difference (the
 * counterpart of mi355_resnet50_force_grad; the reference has no such hook: autograd under loss.backward(), /root/reference/sota_imagenet/callbacks.py:317). */
int mi355_bresnet50_grad_hooks(mi355_bctx* ctx, void* const* record, const void* const* replay, int nblocks);

/* ---- gradient collective inside the boundary: RCCL over xGMI, one process per GPU ---------------------------------
 * replaces torch.nn.parallel.DistributedDataParallel(model, device_ids=[local_rank]) — train.py:113-114, process group
 * train.py:58-61 — i.e. the one-time rank-0 broadcast of parameters / buffers and the bucketed gradient MEAN all-reduce
 * overlapped with backward.  RCCL is bound at run time (librccl.so.1); mi355_comm_available() says whether it was found.
 *   bootstrap  rank 0 calls mi355_comm_unique_id(id) (MI355_COMM_ID_BYTES bytes) and hands `id` to the other ranks through
 *              the launcher's own channel (the reference has one: init_process_group("nccl", "env://"), train.py:61);
 *              every rank then calls mi355_comm_create(&comm, id, nranks, rank, device) (collective: ncclCommInitRank).
 *   data path  mi355_resnet50_set_comm(ctx, comm, bucket_cap_mb): consecutive backward segments form buckets of at least
 *              bucket_cap_mb MiB of the flat gradient array (the last bucket is cut once more: its trailing segments up to
 *              bucket_cap_mb / 8 — stem, layer 1, the end of layer 2 — form a small bucket of their own, so that only a few MB
 *              are reduced after backward has ended); mi355_resnet50_backward then launches, when a bucket's last
 *              segment has been enqueued, ONE mean all-reduce over the bucket's contiguous slice on a HIP stream the
 *              communicator owns, ordered by events behind the kernels that produce it (both executor streams), and makes
 *              `stream` wait for the last one before it returns — so ONE backward call covers all segments, the collective
 *              overlaps the rest of backward, and the caller's next kernel (the optimizer step) sees reduced gradients.
 *              No host thread, no host wait.  comm == NULL detaches.  mi355_resnet50_bucket_plan reports the buckets a
 *              cap would produce (works on a layout-only ctx; n_out = number of buckets, arrays filled up to `cap`).
 *   xGMI is point-to-point (7 links per GPU, ring collectives are per-link bound): keep buckets few and large.      */
#define MI355_COMM_ID_BYTES 128
/* (mi355_comm: declared above, with the BResNet-50 executor's data-parallel entry points) */
int mi355_comm_available(void);
int mi355_comm_unique_id(void* id_out);
int mi355_comm_create(mi355_comm** out, const void* id, int nranks, int rank, int device);
int mi355_comm_destroy(mi355_comm* comm);
int mi355_comm_nranks(const mi355_comm* comm);
/* in-place collectives on fp32 device arrays, enqueued on `stream` (construction-time broadcast of rank `root`'s
 * parameters / BN buffers; a plain mean all-reduce for callers that keep their own schedule) */
int mi355_comm_broadcast(mi355_comm* comm, float* buf, size_t n, int root, void* stream);
int mi355_comm_allreduce_mean(mi355_comm* comm, float* buf, size_t n, void* stream);
int mi355_resnet50_set_comm(mi355_ctx* ctx, mi355_comm* comm, double bucket_cap_mb);
/* CUs this library leaves to the communication library's kernels while a step runs (RCCL's all-reduce kernels need CUs of their own;
 * the reference leaves that to NCCL and the CUDA scheduler, /root/reference/train.py:113-114): every grid sized from the CU count plans
 * for CUs - n.  n: a non-negative multiple of 8 (the same number per XCD).  Process-global; call before creating contexts.        */
int mi355_set_reserved_cus(int n);
/* the per-launch tile knobs (MI355_IGEMM8, MI355_IGEMM_BIG, MI355_STEM_DIRECT, MI355_STEM_TH, MI355_STEM_DBG: test hooks / A/B switches)
 * are read from the environment once; this re-reads them (tests flip them between launches of one process)                          */
int mi355_reload_knobs(void);
/* name of the kernel the calling thread's last convolution / weight-gradient launch went to: the symbol of a generated gfx950 kernel
 * (dconv_l3_s1, po_k256_b256_s2_a2, wg3_l2 ...) or the implicit-GEMM tile family (igemm<bf16,128,128,2> ...).  A debugging query: the
 * tests pin the selection rules with it (cuDNN's own algorithm choice under /root/reference/sota_imagenet/callbacks.py:316-317 is not
 * observable in the reference).  The string stays valid until the thread's next launch.                                            */
const char* mi355_last_conv_kernel(void);
/* measurement stand-in for a collective's CU footprint on one GPU: `workgroups` 256-thread workgroups (16 KiB of LDS each) that hold
 * their CU slots for `usec` microseconds without memory traffic (tools/reserve_cus_ab.py; not part of the training path)           */
int mi355_comm_standin(int workgroups, int usec, void* stream);
/* DistributedDataParallel.no_sync() (gradient accumulation, accumulate_steps > 1 — arg_parser.py:85-86, the Runner's inner step):
 * on == 0 makes the following backward calls of this ctx skip the bucket all-reduces (gradients stay rank-local and keep
 * accumulating); the last micro-step runs with on != 0 (the default) and reduces the accumulated sums once.        */
int mi355_resnet50_set_grad_sync(mi355_ctx* ctx, int on);
/* Record of every collective issued through `comm` since creation / the last reset, in issue order (at most 4096 kept):
 * kinds[i] 0 = bucket mean all-reduce issued by mi355_resnet50_backward over [begins[i], ends[i]) of the flat gradient array
 * (elements), 1 = mi355_comm_broadcast of ends[i] elements, 2 = mi355_comm_allreduce_mean of ends[i] elements.
 * n_out = number of records (arrays are filled up to `cap`); reset != 0 clears the record afterwards.  Host-side only —
 * lets a test assert that one backward reduced every gradient element exactly once, in bucket order.              */
int mi355_comm_stats(mi355_comm* comm, int reset, int cap, int* n_out, int* kinds, size_t* begins, size_t* ends);
int mi355_resnet50_bucket_plan(const mi355_ctx* ctx, double bucket_cap_mb, int cap, int* n_out, size_t* begins,
                               size_t* ends, int* last_segs);

/* dtype MI355_FP8 in mi355_resnet50_create = BASELINE.json configs[4] "fp8 MFMA convs": every tensor stays bf16 (fp32 accumulation,
 * statistics, master weights as in the bf16 step) and the forward / data-gradient convolutions of every layer whose channel counts
 * are multiples of 128 on both sides (layers 2-4) read OCP e4m3 twins of their operands through v_mfma_f32_16x16x32_fp8_fp8; the
 * weight gradients, the stem, layer 1 and the FC stay on bf16 operands.  No standalone quantise pass exists: the BN-apply /
 * BN-backward-apply kernels that produce an activation / gradient tensor write its twin in the same pass (q = e4m3(bf16(v) *
 * scale), saturating) and the weight preparation writes the weights' twins.  Scaling is per tensor and DELAYED: a producer also
 * records max|v| (atomicMax), and scale(step k+1) = 448 / (2 * amax(step k)).  The first training step of a ctx has no amaxes
 * yet: it runs bf16 operands and only records them (forward and backward); from the 2nd step on the convs read the twins.
 * Inference forwards always read the bf16 tensors.  mi355_resnet50_fp8_state: whether the last training step's
 * forward / backward convs read the twins, and how many layers do.  Conv call sites replaced: callbacks.py:316-317; stage
 * schema this dtype is used with: arg_parser.py:65-72, dali_dataloader.py:213-239.
 * debug_tensor names of an fp8 ctx: "<conv>.xq" / ".wq" / ".wtq" (e4m3 bytes, dtype MI355_FP8), "<conv>.sx" / ".sw" / ".sdy" (scales). */
int mi355_resnet50_fp8_state(const mi355_ctx* ctx, int* fwd_on, int* bwd_on, int* n_fwd_layers, int* n_dgrad_layers);

/* algorithmic work of the ctx's conv/FC kernels (2 FLOP/MAC, padding-free): forward and fwd+bwd */
int mi355_resnet50_flops(const mi355_ctx* ctx, double* fwd_flops, double* train_flops);
/* which kernel each convolution of the network went to in its last forward / data-gradient / weight-gradient launch, one text line
 * per layer: "<conv name> fwd=<kernel> dgrad=<kernel> wgrad=<kernel>" ('-' = not launched yet; names as mi355_last_conv_kernel).
 * Writes at most cap bytes (NUL-terminated) and the size a complete table needs.  A debugging query: the tests assert the selection
 * rules of the bs-256 plan with it (the reference's counterpart, cuDNN's algorithm choice under
 * /root/reference/sota_imagenet/callbacks.py:316-317, is not observable).                                                         */
int mi355_resnet50_kernel_table(const mi355_ctx* ctx, char* out, size_t cap, size_t* needed);

/* Test hook: device pointer / shape of an internal tensor of the last step, by name:
 *   "<conv>.y" raw conv output, "<block>.a1|a2|out" post-activation tensors (e.g. "layer1.0.out"),
 *   "<bn>.save_mean|save_invstd", "stem.p0" (the stem's BN+ReLU+maxpool output; the 112x112 activation itself
 *   is never stored), "pooled", "dpooled", "gG0".."gG1" (block-output gradients of the last backward),
 *   "grad.cur" (between two backward segments: the gradient the next segment starts from);
 *   with a weight transform on: "<conv>.w_hat" (fp32 [Cout,K,K,Cin], what the last forward convolved with) and "<conv>.ws_invstd" ([Cout]).
 * shape is NHWC (ndim 4) or [n] / [N,C]; dtype is MI355_F32 or the ctx dtype.  Read-only use.     */
int mi355_resnet50_debug_tensor(const mi355_ctx* ctx, const char* name, void** ptr, int* dtype, int* ndim,
                                int shape[4]);
/* Per-filter forward weight transform of every convolution (the FC is left alone): mode 0 off (the default), 1 standardise — the reference's
 * `weight_standardization: True` (train.py:66-67), w_hat = (w - mean) / sqrt(var + 1e-5) per output filter over K*K*Cin, biased variance —,
 * 2 centre — ForwardWeightNorm(use_std=False), sota_imagenet/callbacks.py:62-84: w_hat = w - mean.  The bound parameters and gradients stay
 * those of the raw w.  With a mode on, every forward (training and inference) starts with ONE launch of the forward kernel of
 * csrc/weight_std.hip over all 53 convolutions and convolves with w_hat; every weight gradient is formed wrt w_hat in a scratch array and one
 * backward launch per backward segment (a bottleneck's three or four convolutions, or the stem) writes beta*dw + the gradient wrt w into the
 * bound gradients, behind that segment's weight gradients on their stream: 17 launches per backward, and a segment's gradients are complete when
 * the backward call that ran it returns.  The scratch (w_hat and the gradient wrt it, each the size of the flat parameter array, one invstd
 * per filter, the row table) is allocated when a mode other than 0 is first set and kept until the context is destroyed; mode 0 launches
 * nothing and reads the parameters as before.  Fails with MI355_E_ARG on a mode outside 0..2 or any mode other than 0 on a MI355_FP8
 * context, MI355_E_STATE on a layout-only context or between a training forward and the end of its backward, MI355_E_NOMEM if the scratch
 * cannot be allocated.                                                                                                                  */
int mi355_resnet50_set_weight_transform(mi355_ctx* ctx, int mode);
/* Forward spectral normalisation of every convolution (csrc/spectral_norm.hip; the reference's ForwardSpectralNorm callback): on != 0 — every
 * forward runs mi355_spectral_fwd over the 53 conv filters at its head (training: one power iteration, which advances u and v; eval: none) and
 * convolves with w_hat = w / sigma; every backward segment runs mi355_spectral_bwd on the weight-gradient stream behind that segment's weight
 * gradients and leaves the gradients wrt the raw weights in the bound array.  u (one float per filter of the model, 26 560) and v (one per
 * filter element of each convolution, sum of K*K*Cin over the 53, in (K,K,Cin) order) are caller-owned device arrays that must outlive the
 * switch: every context of a model is given the same two and advances one state.  A switch of its own, not a mode of
 * mi355_resnet50_set_weight_transform, and the two exclude each other: MI355_E_ARG when the other one is in force (from either call), on
 * null u or v with on != 0, or on a MI355_FP8 context; MI355_E_STATE on a layout-only context or between a training forward and the end of its
 * backward; MI355_E_NOMEM if the scratch (w_hat, the gradient wrt it, sigma, the table, the sums' scratch) cannot be allocated.  It is
 * allocated at the first on != 0 and kept; on == 0 launches nothing and reads the parameters as before. */
int mi355_resnet50_set_spectral_norm(mi355_ctx* ctx, int on, float* u, float* v);
/* Test hook (teacher forcing): between two calls of mi355_resnet50_backward() that split the segments, replace the gradient the next
 * segment starts from ("grad.cur": wrt that block's output, or wrt the stem's pooled output before the last segment) by `g` (device
 * memory, the ctx dtype, exactly the tensor's bytes).  The BN-backward sums the producing kernel's epilogue left for that tensor are
 * dropped (the next segment re-reduces them from g).  Two kernel selections fed the SAME incoming gradient per segment differ by
 * that segment's own kernels only: what autograd's per-node gradcheck does for the graph under loss.backward()
 * (/root/reference/sota_imagenet/callbacks.py:317).  MI355_E_STATE outside a split backward.                                       */
int mi355_resnet50_force_grad(mi355_ctx* ctx, const void* g, size_t bytes, void* stream);

/* HIP-event timing of kernel classes inside a step, recorded on the stream the kernels are launched on.
 * mi355_resnet50_profile(ctx, class_mask): bit k set => every launch of class k is bracketed by a pair of
 * hipEvents from now on (mask 0 switches it off; calling it also clears earlier records).  Classes:
 *   0 igemm_kernel<T,128|256,128|256,...> (conv fwd + dgrad, >=128 output channels)   1 igemm_kernel<T,128,64,...> (incl. stem)
 *   2 wgrad_kernel<T,128,*>   3 wgrad_kernel<T,64,*> (incl. stem)   4 bn_reduce_kernel (stats + bwd sums)
 *   5 bn_apply_kernel   6 other (ingest, pools, FC, weight prep)   7 bn_bwd_apply_kernel
 *   profile_read kind 8: the 3x3 convolutions (fwd + dgrad) among the recorded launches of classes 0 and 1
 *   profile_read kind 9: the launches that ran on e4m3 operands (fp8 ctx) among the recorded launches
 * (one class = one kernel symbol, so the averages can be checked against rocprofv3 --kernel-trace --stats)
 * mi355_resnet50_profile_read(ctx, k, ...) waits for the recorded events of class k and returns their
 * summed duration (ms), launch count and the algorithmic FLOPs / bytes those launches represent.    */
int mi355_resnet50_profile(mi355_ctx* ctx, int class_mask);
int mi355_resnet50_profile_read(mi355_ctx* ctx, int kind, double* total_ms, int* launches,
                                double* alg_flops, double* alg_bytes);

#ifdef __cplusplus
}
#endif
#endif /* MI355RN_H */
