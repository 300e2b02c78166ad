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
#include <cmath>

#include "common.h"
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

// f32x4 grid-stride loop + scalar tail (n not a multiple of 4), the shape of sgd_kernel: 28 B / element (36 B with the average).
// Measured on the 25.6 M-element array: sgd_kernel's 4096-workgroup cap and plain gradient loads gave 138 us (5.2 TB/s); up to
// 16384 workgroups and a non-temporal gradient load give 110 us (6.5 TB/s, the rate of sgd_kernel) — profiles/adamw_step.json
template <bool DECOUPLED, bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ ema, size_t n4, size_t n, AdamArgs a) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);  // last use of the gradient
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 ev = {0.f, 0.f, 0.f, 0.f};
    if constexpr (EMA) ev = reinterpret_cast<f32x4*>(ema)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = pv[k], mk = mv[k], vk = vv[k], ek = ev[k];
      adam_elem<DECOUPLED, EMA>(pk, gv[k], mk, vk, ek, a);
      pv[k] = pk, mv[k] = mk, vv[k] = vk, ev[k] = ek;
    }
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(p)[i] = pv;
    if constexpr (EMA) reinterpret_cast<f32x4*>(ema)[i] = ev;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = n4 * 4 + threadIdx.x;
    float pk = p[i], mk = m[i], vk = v[i], ek = EMA ? ema[i] : 0.f;
    adam_elem<DECOUPLED, EMA>(pk, g[i], mk, vk, ek, a);
    m[i] = mk, v[i] = vk, p[i] = pk;
    if constexpr (EMA) ema[i] = ek;
  }
}

int adam_grid(size_t n4) {
  size_t b = (n4 + 255) / 256;
  if (b > 16384) b = 16384;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

int launch_adam(float* p, const float* g, float* m, float* v, size_t n, double beta1, double beta2, float eps, float step_size,
                float bc2_sqrt, double lr, double wd, int decoupled, float gscale, hipStream_t s, float* ema, float ema_decay) {
  MI355_ARG(p && g && m && v, "adam: null pointer");
  MI355_ARG(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0) &&
                ((uintptr_t)ema % 16 == 0),
            "adam: pointers must be 16-byte aligned");
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
  if (decoupled) {
    if (ema) hipLaunchKernelGGL((adam_kernel<true, true>), grid, block, 0, s, p, g, m, v, ema, n4, n, a);
    else hipLaunchKernelGGL((adam_kernel<true, false>), grid, block, 0, s, p, g, m, v, ema, n4, n, a);
  } else {
    if (ema) hipLaunchKernelGGL((adam_kernel<false, true>), grid, block, 0, s, p, g, m, v, ema, n4, n, a);
    else hipLaunchKernelGGL((adam_kernel<false, false>), grid, block, 0, s, p, g, m, v, ema, n4, n, a);
  }
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
