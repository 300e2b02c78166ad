// optim.hip — fused Adam / AdamW step on a flat fp32 range (gfx950), next to misc.hip's sgd_kernel.
// Replaces torch.optim._multi_tensor.AdamW.step (configs/hydra_exp/5.r50_base_adamw_high-aug.yaml:17-20 of the reference, built
// at train.py:92).  Per element it follows the operation order of torch's _single_tensor_adam:
//   g  = g * grad_scale
//   AdamW: p *= (1 - lr*wd)                 Adam: g = g + wd * p            (both skipped when wd == 0, as torch does)
//   m  = m + (1 - b1) * (g - m)             (torch's lerp for a weight < 0.5)
//   v  = v * b2 + ((1 - b2) * g) * g        (mul_ + addcmul_)
//   p  = p + (-step_size * m) / (sqrt(v) / bc2_sqrt + eps)     (addcdiv_), step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t)
//   EMA: ema = ema + (1 - decay) * (p - ema)
// The library builds with -ffp-contract=off, and sqrtf / '/' stay correctly rounded (no fast-math forms).
// Every element-wise kernel here states its arrays and its rule; the loop over them is flat_sweep (optim_sweep.h).
#include <cmath>

#include "common.h"
#include "dispatch.h"
#include "optim_sum.h"
#include "optim_sweep.h"
#include "vec.h"

namespace mi355 {
namespace {

struct AdamArgs {
  float b1w;        // 1 - beta1 (rounded from double, as torch rounds the lerp weight)
  float b2;         // beta2
  float b2w;        // 1 - beta2
  float eps;
  float neg_step;   // -step_size
  float bc2_sqrt;
  float decay;      // AdamW: 1 - lr*wd (from double)
  float wd;         // Adam: the L2 coefficient
  bool apply_wd;    // torch skips the weight decay term when wd == 0
  float gscale;
  float ema_w;      // 1 - ema_decay
};

template <bool DECOUPLED, bool EMA>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& e, const AdamArgs& a) {
  float ge = g * a.gscale;
  float pe = p;
  if (a.apply_wd) {
    if constexpr (DECOUPLED) pe = pe * a.decay;
    else ge = ge + a.wd * pe;
  }
  m = m + a.b1w * (ge - m);
  v = v * a.b2 + (a.b2w * ge) * ge;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  pe = pe + (a.neg_step * m) / denom;
  p = pe;
  if constexpr (EMA) e = e + a.ema_w * (pe - e);
}

// flat_sweep (optim_sweep.h: f32x4 grid-stride loop + scalar tail), as sgd_kernel: 28 B / element (36 B with the average).
// Measured on the 25.6 M-element array: sgd_kernel's 4096-workgroup cap and plain gradient loads gave 138 us (5.2 TB/s); up to
// 16384 workgroups and a non-temporal gradient load give 110 us (6.5 TB/s, the rate of sgd_kernel) — profiles/adamw_step.json
template <bool DECOUPLED, bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ ema, size_t n4, size_t n, AdamArgs a) {
  const auto rule = [&](float& pk, float& gk, float& mk, float& vk, float& ek) { adam_elem<DECOUPLED, EMA>(pk, gk, mk, vk, ek, a); };
  flat_sweep(n4, n, rule, upd(p), last(g), upd(m), upd(v), upd_if<EMA>(ema));
}

int adam_grid(size_t n4) {
  size_t b = (n4 + 255) / 256;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

// decoupled = 0: Adam, 1: AdamW; + the parameter average when ema != nullptr
static int launch_adam(float* p, const float* g, float* m, float* v, size_t n, double beta1, double beta2, float eps, float step_size,
                       float bc2_sqrt, double lr, double wd, int decoupled, float gscale, hipStream_t s, float* ema = nullptr,
                       float ema_decay = 0.f) {
  MI355_ARG(p && g && m && v, "adam: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema), "adam: pointers must be 16-byte aligned");
  MI355_ARG(beta1 >= 0.0 && beta1 < 1.0, "adam: beta1=%g outside [0, 1)", beta1);
  MI355_ARG(beta2 >= 0.0 && beta2 < 1.0, "adam: beta2=%g outside [0, 1)", beta2);
  MI355_ARG(std::isfinite(eps) && eps >= 0.f, "adam: eps=%g must be finite and >= 0", (double)eps);
  MI355_ARG(std::isfinite(step_size), "adam: step_size=%g is not finite", (double)step_size);
  MI355_ARG(std::isfinite(bc2_sqrt) && bc2_sqrt > 0.f, "adam: bc2_sqrt=%g must be finite and > 0 (step count >= 1)", (double)bc2_sqrt);
  MI355_ARG(std::isfinite(lr) && std::isfinite(wd), "adam: lr / weight_decay not finite");
  MI355_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "adam: ema_decay=%g outside [0, 1]", (double)ema_decay);
  AdamArgs a;
  a.b1w = (float)(1.0 - beta1);
  a.b2 = (float)beta2;
  a.b2w = (float)(1.0 - beta2);
  a.eps = eps;
  a.neg_step = -step_size;
  a.bc2_sqrt = bc2_sqrt;
  a.decay = (float)(1.0 - lr * wd);
  a.wd = (float)wd;
  a.apply_wd = wd != 0.0;
  a.gscale = gscale;
  a.ema_w = ema ? 1.f - ema_decay : 0.f;
  const size_t n4 = n / 4;
  const dim3 grid(adam_grid(n4)), block(256);
  return with_bool(decoupled != 0, [&](auto DECOUPLED) -> int {
    return with_bool(ema != nullptr, [&](auto EMA) -> int {
      hipLaunchKernelGGL((adam_kernel<DECOUPLED, EMA>), grid, block, 0, s, p, g, m, v, ema, n4, n, a);
      MI355_LAUNCH_CHECK();
      return 0;
    });
  });
}
extern "C" int mi355_adam_step(float* p, const float* g, float* m, float* v, size_t n, double beta1, double beta2, float eps,
                               float step_size, float bc2_sqrt, double lr, double weight_decay, int decoupled, float grad_scale,
                               void* stream) {
  return launch_adam(p, g, m, v, n, beta1, beta2, eps, step_size, bc2_sqrt, lr, weight_decay, decoupled, grad_scale,
                     (hipStream_t)stream);
}
extern "C" int mi355_adam_step_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, double beta1, double beta2,
                                   float eps, float step_size, float bc2_sqrt, double lr, double weight_decay, int decoupled,
                                   float grad_scale, float ema_decay, void* stream) {
  MI355_ARG(ema, "adam_step_ema: null ema");
  return launch_adam(p, g, m, v, n, beta1, beta2, eps, step_size, bc2_sqrt, lr, weight_decay, decoupled, grad_scale,
                     (hipStream_t)stream, ema, ema_decay);
}

// ---- MADGRAD: src.optimizers.MADGRAD.step of the reference (sota_imagenet/optimizers.py:726-767), in its operation order --------------------
//   g   = g * grad_scale
//   gss = gss + (lamb * g) * g               (addcmul_, value = lamb), lamb = (lr + eps) * sqrt(k + 1) from the host, in double
//   rms = cbrt(gss) + eps                    (pow(1/3).add_(eps))
//   s   = s + lamb * g
//   z   = x0 + (-s) / rms                    (addcdiv, value = -1)
//   p   = p * momentum + ck * z              (mul_(1 - ck).add_(z, alpha = ck), ck = 1 - momentum)
//   p   = p * (1 - weight_decay)             (decoupled and NOT scaled by lr: as the reference has it)
// 32 B / element (p, gss, s read + write, g, x0 read), 40 B with the average.  Padding (p = g = gss = s = x0 = 0) stays 0 for eps > 0.
namespace {

struct MadgradArgs {
  float lamb, eps, mom, ck, wd_mul, gscale, ema_w;
};

template <bool EMA>
__device__ __forceinline__ void madgrad_elem(float& p, float g, float& gss, float& s, float x0, float& e, const MadgradArgs& a) {
  const float ge = g * a.gscale;
  gss = gss + (a.lamb * ge) * ge;
  const float rms = cbrtf(gss) + a.eps;
  s = s + a.lamb * ge;
  const float z = x0 + (-s) / rms;
  float pe = p * a.mom + a.ck * z;
  pe = pe * a.wd_mul;
  p = pe;
  if constexpr (EMA) e = e + a.ema_w * (pe - e);
}

template <bool EMA>
__global__ __launch_bounds__(256) void madgrad_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ gss,
                                                      float* __restrict__ s, const float* __restrict__ x0, float* __restrict__ ema, size_t n4,
                                                      size_t n, MadgradArgs a) {
  const auto rule = [&](float& pk, float& gk, float& qk, float& sk, float& xk, float& ek) { madgrad_elem<EMA>(pk, gk, qk, sk, xk, ek, a); };
  flat_sweep(n4, n, rule, upd(p), last(g), upd(gss), upd(s), rd(x0), upd_if<EMA>(ema));
}

}  // namespace

static int launch_madgrad(float* p, const float* g, float* gss, float* s, const float* x0, size_t n, double lr, double momentum, double wd,
                          double eps, int k, float gscale, hipStream_t st, float* ema = nullptr, float ema_decay = 0.f) {
  MI355_ARG(p && g && gss && s && x0, "madgrad: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(gss) && aligned16(s) && aligned16(x0) && aligned16(ema),
            "madgrad: pointers must be 16-byte aligned");
  MI355_ARG(momentum >= 0.0 && momentum < 1.0, "madgrad: momentum=%g outside [0, 1)", momentum);
  MI355_ARG(std::isfinite(eps) && eps >= 0.0, "madgrad: eps=%g must be finite and >= 0", eps);
  MI355_ARG(std::isfinite(lr) && lr >= 0.0, "madgrad: lr=%g must be finite and >= 0", lr);
  MI355_ARG(std::isfinite(wd) && wd >= 0.0, "madgrad: weight_decay=%g must be finite and >= 0", wd);
  MI355_ARG(k >= 0, "madgrad: step counter k=%d must be >= 0", k);
  MI355_ARG(std::isfinite(gscale), "madgrad: grad_scale=%g is not finite", (double)gscale);
  MI355_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "madgrad: ema_decay=%g outside [0, 1]", (double)ema_decay);
  const double ck = 1.0 - momentum;
  MadgradArgs a;
  a.lamb = (float)((lr + eps) * std::pow((double)k + 1.0, 0.5));
  a.eps = (float)eps;
  a.mom = (float)(1.0 - ck);  // the reference multiplies by 1 - ck, not by momentum
  a.ck = (float)ck;
  a.wd_mul = (float)(1.0 - wd);
  a.gscale = gscale;
  a.ema_w = ema ? 1.f - ema_decay : 0.f;
  const size_t n4 = n / 4;
  const dim3 grid(adam_grid(n4)), block(256);
  return with_bool(ema != nullptr, [&](auto EMA) -> int {
    hipLaunchKernelGGL((madgrad_kernel<EMA>), grid, block, 0, st, p, g, gss, s, x0, ema, n4, n, a);
    MI355_LAUNCH_CHECK();
    return 0;
  });
}
extern "C" int mi355_madgrad_step(float* p, const float* g, float* grad_sum_sq, float* s, const float* x0, size_t n, double lr, double momentum,
                                  double weight_decay, double eps, int k, float grad_scale, void* stream) {
  return launch_madgrad(p, g, grad_sum_sq, s, x0, n, lr, momentum, weight_decay, eps, k, grad_scale, (hipStream_t)stream);
}
extern "C" int mi355_madgrad_step_ema(float* p, const float* g, float* grad_sum_sq, float* s, const float* x0, float* ema, size_t n, double lr,
                                      double momentum, double weight_decay, double eps, int k, float grad_scale, float ema_decay,
                                      void* stream) {
  MI355_ARG(ema, "madgrad_step_ema: null ema");
  return launch_madgrad(p, g, grad_sum_sq, s, x0, n, lr, momentum, weight_decay, eps, k, grad_scale, (hipStream_t)stream, ema, ema_decay);
}

// ---- AdaiS: src.optimizers.AdaiS.step of the reference (sota_imagenet/optimizers.py:569-639) as three device stages on one stream ----------------
// (a) adais_moments_kernel, one launch per flat range:  g = g * grad_scale;  v = v * beta2 + ((1 - beta2) * g) * g;  workgroup b writes the sum of
//     its elements' v / bc2 (bc2 = 1 - beta2^step of the range) to partial[b].  The sum is taken in double, per thread in element order and then by
//     a fixed LDS tree: no floating-point atomics, and the grid is a function of n alone, so partial[] does not depend on scheduling.
// (b) adais_mean_kernel, one workgroup of 1024:  mean = (sum of all partials of all ranges, fixed order, double) / param_size  -> one float on the device.
// (c) adais_step_kernel, one launch per flat range, reading that float:
//       p      = p * (1 - lr*wd)                           (only when wd != 0)
//       beta1  = clamp(1 - ((v / bc2) / mean) * beta0, 0, 1 - eps)
//       b1prod = b1prod * beta1
//       m      = m * beta1 + (1 - beta1) * g
//       p      = p + (-lr) * (m / (1 - b1prod))
// 12 + 32 = 44 B / element (+ 8 with the average).  Padding holds v = 0 (not ema_norm_init), so it adds nothing to the sum; there beta1 = 1 - eps,
// b1prod = m = 0 and p stays 0 for every eps.
namespace {

__global__ __launch_bounds__(256) void adais_moments_kernel(const float* __restrict__ g, float* __restrict__ v, double* __restrict__ partial,
                                                            size_t n4, size_t n, float b2, float b2w, float bc2, float gscale) {
  __shared__ double sh[256];
  double acc = 0.0;
  const auto rule = [&](float& gk, float& vk) {
    const float ge = gk * gscale;
    vk = vk * b2 + (b2w * ge) * ge;
    acc += (double)(vk / bc2);
  };
  flat_sweep(n4, n, rule, rd(g), upd(v));  // g is read again by the step kernel: a plain load
  const double tot = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(1024) void adais_mean_kernel(const double* __restrict__ partial, size_t count, double param_size, float* __restrict__ mean) {
  __shared__ double sh[1024];
  double acc = 0.0;
#pragma unroll 4
  for (size_t i = threadIdx.x; i < count; i += 1024) acc += partial[i];
  const double tot = block_sum<1024>(acc, sh);
  if (threadIdx.x == 0) mean[0] = (float)(tot / param_size);
}

struct AdaisArgs {
  float decay;     // 1 - lr*wd (from double)
  bool apply_wd;   // the reference skips the multiply when wd == 0
  float bc2, beta0, b1max, neg_lr, gscale, ema_w;
};

template <bool EMA>
__device__ __forceinline__ void adais_elem(float& p, float g, float& m, float v, float& bp, float& e, float mean, const AdaisArgs& a) {
  const float ge = g * a.gscale;
  float pe = p;
  if (a.apply_wd) pe = pe * a.decay;
  float beta1 = 1.0f - ((v / a.bc2) / mean) * a.beta0;
  beta1 = fminf(fmaxf(beta1, 0.0f), a.b1max);
  bp = bp * beta1;
  m = m * beta1 + (1.0f - beta1) * ge;
  pe = pe + a.neg_lr * (m / (1.0f - bp));
  p = pe;
  if constexpr (EMA) e = e + a.ema_w * (pe - e);
}

template <bool EMA>
__global__ __launch_bounds__(256) void adais_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         const float* __restrict__ v, float* __restrict__ bp, float* __restrict__ ema,
                                                         const float* __restrict__ mean_ptr, size_t n4, size_t n, AdaisArgs a) {
  const float mean = mean_ptr[0];
  const auto rule = [&](float& pk, float& gk, float& mk, float& vk, float& bk, float& ek) { adais_elem<EMA>(pk, gk, mk, vk, bk, ek, mean, a); };
  flat_sweep(n4, n, rule, upd(p), last(g), upd(m), rd(v), upd(bp), upd_if<EMA>(ema));
}

// bc2 = 1 - beta2^step in double, as the reference's Python does
int adais_bc2(const char* who, double beta2, int step, float* bc2) {
  MI355_ARG(beta2 >= 0.0 && beta2 < 1.0, "%s: beta2=%g outside [0, 1)", who, beta2);
  MI355_ARG(step >= 1, "%s: step=%d must be >= 1 (the count after this step's increment)", who, step);
  *bc2 = (float)(1.0 - std::pow(beta2, (double)step));
  return 0;
}

}  // namespace

// the doubles mi355_adais_moments writes for a range of n elements: one per workgroup
extern "C" size_t mi355_adais_workspace_bytes(size_t n) { return (size_t)adam_grid(n / 4) * sizeof(double); }

extern "C" int mi355_adais_moments(const float* g, float* v, size_t n, double beta2, int step, float gscale, void* workspace, void* stream) {
  double* partial = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(g && v && partial, "adais_moments: null pointer");
  MI355_ARG(aligned16(g) && aligned16(v), "adais_moments: g and v must be 16-byte aligned");
  MI355_ARG((uintptr_t)partial % 8 == 0, "adais_moments: the workspace must be 8-byte aligned");
  float bc2;
  MI355_TRY(adais_bc2("adais_moments", beta2, step, &bc2));
  MI355_ARG(std::isfinite(gscale), "adais_moments: grad_scale=%g is not finite", (double)gscale);
  const size_t n4 = n / 4;
  hipLaunchKernelGGL(adais_moments_kernel, dim3(adam_grid(n4)), dim3(256), 0, st, g, v, partial, n4, n, (float)beta2, (float)(1.0 - beta2), bc2,
                     gscale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_adais_mean(const void* workspace, size_t workspace_bytes, size_t param_size, float* mean, void* stream) {
  const double* partial = (const double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(workspace_bytes % sizeof(double) == 0, "adais_mean: workspace_bytes=%zu is not a whole number of partial sums", workspace_bytes);
  const size_t count = workspace_bytes / sizeof(double);
  MI355_ARG(partial && mean, "adais_mean: null pointer");
  MI355_ARG((uintptr_t)partial % 8 == 0 && (uintptr_t)mean % 4 == 0, "adais_mean: misaligned pointer");
  MI355_ARG(count >= 1 && param_size >= 1, "adais_mean: count=%zu and param_size=%zu must be >= 1", count, param_size);
  hipLaunchKernelGGL(adais_mean_kernel, dim3(1), dim3(1024), 0, st, partial, count, (double)param_size, mean);
  MI355_LAUNCH_CHECK();
  return 0;
}

static int launch_adais_step(float* p, const float* g, float* m, const float* v, float* b1prod, const float* mean, size_t n, double lr,
                             double beta0, double beta2, double eps, double wd, int step, float gscale, hipStream_t st, float* ema = nullptr,
                             float ema_decay = 0.f) {
  MI355_ARG(p && g && m && v && b1prod && mean, "adais_step: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(b1prod) && aligned16(ema),
            "adais_step: pointers must be 16-byte aligned");
  MI355_ARG((uintptr_t)mean % 4 == 0, "adais_step: misaligned mean");
  MI355_ARG(std::isfinite(lr) && lr >= 0.0, "adais_step: lr=%g must be finite and >= 0", lr);
  MI355_ARG(std::isfinite(beta0) && beta0 >= 0.0, "adais_step: beta0=%g must be finite and >= 0", beta0);
  MI355_ARG(std::isfinite(eps) && eps >= 0.0, "adais_step: eps=%g must be finite and >= 0", eps);
  MI355_ARG(std::isfinite(wd) && wd >= 0.0, "adais_step: weight_decay=%g must be finite and >= 0", wd);
  MI355_ARG(std::isfinite(gscale), "adais_step: grad_scale=%g is not finite", (double)gscale);
  MI355_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "adais_step: ema_decay=%g outside [0, 1]", (double)ema_decay);
  AdaisArgs a;
  MI355_TRY(adais_bc2("adais_step", beta2, step, &a.bc2));
  a.decay = (float)(1.0 - lr * wd);
  a.apply_wd = wd != 0.0;
  a.beta0 = (float)beta0;
  a.b1max = (float)(1.0 - eps);
  a.neg_lr = (float)(-lr);
  a.gscale = gscale;
  a.ema_w = ema ? 1.f - ema_decay : 0.f;
  const size_t n4 = n / 4;
  const dim3 grid(adam_grid(n4)), block(256);
  return with_bool(ema != nullptr, [&](auto EMA) -> int {
    hipLaunchKernelGGL((adais_step_kernel<EMA>), grid, block, 0, st, p, g, m, v, b1prod, ema, mean, n4, n, a);
    MI355_LAUNCH_CHECK();
    return 0;
  });
}
extern "C" int mi355_adais_step(float* p, const float* g, float* m, const float* v, float* beta1_prod, const float* mean, size_t n, double lr,
                                double beta0, double beta2, double eps, double weight_decay, int step, float grad_scale, void* stream) {
  return launch_adais_step(p, g, m, v, beta1_prod, mean, n, lr, beta0, beta2, eps, weight_decay, step, grad_scale, (hipStream_t)stream);
}
extern "C" int mi355_adais_step_ema(float* p, const float* g, float* m, const float* v, float* beta1_prod, const float* mean, float* ema,
                                    size_t n, double lr, double beta0, double beta2, double eps, double weight_decay, int step,
                                    float grad_scale, float ema_decay, void* stream) {
  MI355_ARG(ema, "adais_step_ema: null ema");
  return launch_adais_step(p, g, m, v, beta1_prod, mean, n, lr, beta0, beta2, eps, weight_decay, step, grad_scale, (hipStream_t)stream, ema,
                           ema_decay);
}

}  // namespace mi355
