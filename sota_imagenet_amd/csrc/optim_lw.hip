// optim_lw.hip — the layer-wise and unit-wise optimizers of the reference's own tree (sota_imagenet/optimizers.py: MyNovograd :35-161, NovogradApex :189-290,
// AdamLayerwise :293-397, MyAdai :400-519) on flat fp32 arrays (gfx950).  Each of them needs one statistic PER PARAMETER TENSOR — the sum of
// squares of its gradient, or of the parameter itself for MyNovograd — and uses it as a per-tensor scalar in the update.  A step is three
// stages on one stream, nothing read back by the host, over a work-item table the host builds once per plan:
//   item   = (element offset, length <= mi355_lw_item_elems(), tensor index), cut from one tensor's own dense range: never across two tensors,
//            never in padding, the cuts a function of the tensor's numel alone; the items of one tensor are consecutive.
//   (a) lw_sumsq_kernel, one workgroup per item: x = src * scale in float, x * x summed in double — per thread in element order, then the
//       fixed LDS tree of optim_sum.h — into partial[item].  No floating-point atomics: partial[] does not depend on scheduling.
//   (b) lw_coef_kernel, one workgroup (one wave) per tensor of a param group: S = sum of the tensor's partials in a fixed order, then in double,
//       rounded once on store,
//         rules 0 and 1:  v = v*beta2 + (1 - beta2)*stat  (held in float32 as the reference holds it; stat = S, or S / numel with LW_MEAN)
//                         den = sqrt(v) + eps;  wdf = 1 - lr*wd,  or 1 - lr*wd/den (LW_STABLE_WD),  or lr*wd (LW_SOFT_WD)
//         rule 2 (MyAdai): vt = v0*beta2 + (S/numel)*(1 - beta2)   with v0 the constant the class keeps in its state (it never writes vt back)
//                         beta1 = clip(1 - (vt/mean or sqrt(vt/mean))*beta0, 0, 1 - eps);  gw = 1 (LW_SGD_MOM) or 1 - beta1
//                         wdf = 1 - lr*wd, or 1 - lr*wd/(1 - beta1) (LW_STABLE_WD)
//       -> coef[tensor] = (den, beta1, gw, wdf) in float32
//   (c) lw_update_kernel<RULE, EMA>, one workgroup per item of a param group, the item's coefficients read once per workgroup:
//         g = g * grad_scale
//         rule 0 (AdamLayerwise, NovogradApex):  m = m*beta1 + gw*(g/den);  p = p + (-lr)*m
//         rule 1 (MyNovograd):                   m = m*beta1 + gw*g;        p = p + (-lr)*(m/den)
//         rule 2 (MyAdai):                       m = m*beta1 + gw*g;        p = p + (-lr)*m
//         p = p*wdf,  or with LW_SOFT_WD (NovogradApex's wd_eps)  p = p - wdf*(max(|p| - wd_eps, 0)*sign(p))
//         EMA: ema = ema + (1 - decay)*(p - ema)
// 4 B / element in (a) + 20 B / element in (c) (p, m read + write, g read once more, non-temporal: its last use), 28 B with the average.
// unitwise_norm=True (MyNovograd, NovogradApex; recipe 48, optimizers.py:16-22, :134-135, :267-268) takes the statistic per SLOT — a whole tensor
// with ndim <= 1, one index of dim 0 otherwise — and it is the NORM, sqrt of the sum of squares, also for the 1-D tensors:
//   (a') lw_unit_sumsq_kernel, one wave per piece of a unit (optim_items.h: any element offset), four pieces per workgroup; the 1-D tensors go
//        through lw_sumsq_kernel over their items.  One double per piece or item.
//   (b') lw_unit_coef_kernel, one wave per slot, four slots per workgroup, one launch per param group: S = the slot's consecutive partials in a
//        fixed order; v[slot] = v*beta2 + (1 - beta2)*sqrt(S) in double, rounded once to float32; den[slot] = (float)(sqrt((double)v) + eps).
//   (c') lw_unit_update_kernel<RULE, EMA>, rules 0 and 1, one workgroup per item: beta1, 1 - beta1, -lr and wdf are the same for the whole launch
//        (formed in double, rounded once, as lw_coef_kernel stores them); den comes from the slot of each element, slot0 + (offset inside the
//        tensor) / unit_len: unit_item_sweep (optim_items.h).
// The library builds with -ffp-contract=off, and sqrt / '/' stay correctly rounded.  The loop of (a) and (c) over an item's elements is item_sweep
// (optim_sweep.h: 256 threads, f32x4 body, scalar tail).
#include <cmath>

#include "common.h"
#include "dispatch.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "optim_sweep.h"
#include "vec.h"

namespace mi355 {
namespace {

struct LwTensor {
  int first, count;  // its items in the table (and its partial sums in partial[])
  double numel;
};
static_assert(sizeof(LwTensor) == 16, "table records are 16 bytes");

enum { LW_MEAN = 1, LW_STABLE_WD = 2, LW_SOFT_WD = 4, LW_SGD_MOM = 8, LW_SQRT_MOM = 16 };

__global__ __launch_bounds__(256) void lw_sumsq_kernel(const float* __restrict__ src, size_t n, const LwItem* __restrict__ items,
                                                       double* __restrict__ partial, int n_tensors, float scale) {
  __shared__ double sh[256];
  const LwItem it = items[blockIdx.x];
  double acc = 0.0;
  if (item_ok(it, n, n_tensors)) {
    const auto rule = [&](float& x) {
      const double e = (double)(x * scale);
      acc += e * e;
    };
    item_sweep(it.len, rule, rd(src + it.off));  // read again by the update kernel: a plain load
  }
  const double tot = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

struct LwCoefArgs {
  double beta1, beta2, eps, lr, wd, mean;  // beta1: beta0 for rule 2;  mean: rule 2 only
  int rule, flags;
};

__global__ __launch_bounds__(64) void lw_coef_kernel(const double* __restrict__ partial, size_t n_partial, const LwTensor* __restrict__ tens,
                                                     void* __restrict__ vstate, float* __restrict__ coef, double* __restrict__ sums, LwCoefArgs a) {
  __shared__ double sh[64];
  const LwTensor t = tens[blockIdx.x];
  const UnitSlot span{t.first, t.count};
  const bool ok = slot_ok(span, n_partial);
  double acc[1] = {};
  if (ok) slot_gather<64>(span, partial, threadIdx.x, acc);
  const double S = block_sum<64>(acc[0], sh);
  if (threadIdx.x != 0 || !ok) return;
  sums[blockIdx.x] = S;
  const double stat = (a.flags & LW_MEAN) ? S / t.numel : S;
  const double lrwd = a.lr * a.wd;
  double den = 1.0, b1 = a.beta1, gw = 1.0 - a.beta1, wdf = 1.0 - lrwd;
  if (a.rule != 2) {
    float* v = reinterpret_cast<float*>(vstate) + blockIdx.x;
    const float vn = (float)((double)v[0] * a.beta2 + (1.0 - a.beta2) * stat);
    v[0] = vn;
    den = sqrt((double)vn) + a.eps;
    if (a.flags & LW_STABLE_WD) wdf = 1.0 - lrwd / den;
    if (a.flags & LW_SOFT_WD) wdf = lrwd;
  } else {
    const double v0 = reinterpret_cast<const double*>(vstate)[blockIdx.x];
    const double vt = v0 * a.beta2 + stat * (1.0 - a.beta2);
    const double r = vt / a.mean;
    b1 = 1.0 - ((a.flags & LW_SQRT_MOM) ? sqrt(r) : r) * a.beta1;
    b1 = fmin(fmax(b1, 0.0), 1.0 - a.eps);
    gw = (a.flags & LW_SGD_MOM) ? 1.0 : 1.0 - b1;
    if (a.flags & LW_STABLE_WD) wdf = 1.0 - lrwd / (1.0 - b1);
  }
  f32x4 c = {(float)den, (float)b1, (float)gw, (float)wdf};
  reinterpret_cast<f32x4*>(coef)[blockIdx.x] = c;
}

struct LwUpdArgs {
  float neg_lr, gscale, ema_w, wd_eps;
  bool soft_wd;
};

LwUpdArgs lw_upd_args(double lr, int soft_wd, double wd_eps, float gscale, const float* ema, float ema_decay) {
  LwUpdArgs a;
  a.neg_lr = (float)(-lr);
  a.gscale = gscale;
  a.ema_w = ema ? 1.f - ema_decay : 0.f;
  a.wd_eps = soft_wd ? (float)wd_eps : 0.f;
  a.soft_wd = soft_wd != 0;
  return a;
}

template <int RULE, bool EMA>
__device__ __forceinline__ void lw_elem(float& p, float g, float& m, float& e, const f32x4& c, const LwUpdArgs& a) {
  const float ge = g * a.gscale;
  float pe;
  if constexpr (RULE == 0) {
    m = m * c[1] + c[2] * (ge / c[0]);
    pe = p + a.neg_lr * m;
  } else if constexpr (RULE == 1) {
    m = m * c[1] + c[2] * ge;
    pe = p + a.neg_lr * (m / c[0]);
  } else {
    m = m * c[1] + c[2] * ge;
    pe = p + a.neg_lr * m;
  }
  if (RULE == 0 && a.soft_wd) pe = pe - c[3] * copysignf(fmaxf(fabsf(pe) - a.wd_eps, 0.0f), pe);
  else pe = pe * c[3];
  p = pe;
  if constexpr (EMA) e = e + a.ema_w * (pe - e);
}

template <int RULE, bool EMA>
__global__ __launch_bounds__(256) void lw_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ ema, size_t n, const LwItem* __restrict__ items,
                                                        const float* __restrict__ coef, int n_tensors, LwUpdArgs a) {
  const LwItem it = items[blockIdx.x];
  if (!item_ok(it, n, n_tensors)) return;
  const f32x4 c = reinterpret_cast<const f32x4*>(coef)[it.tensor];
  const auto rule = [&](float& pk, float& gk, float& mk, float& ek) { lw_elem<RULE, EMA>(pk, gk, mk, ek, c, a); };
  item_sweep(it.len, rule, upd(p + it.off), last(g + it.off), upd(m + it.off), upd_if<EMA>(ema + it.off));
}

__global__ __launch_bounds__(256) void lw_unit_sumsq_kernel(const float* __restrict__ src, size_t n, const UnitPiece* __restrict__ pieces,
                                                            size_t n_pieces, int n_slots, double* __restrict__ partial, float scale) {
  const auto add = [&](double(&acc)[1], float x) {
    const double e = (double)(x * scale);
    acc[0] += e * e;
  };
  __shared__ double sh[256];
  piece_sums<64>(pieces, n_pieces, n, n_slots, partial, {sh}, add, src);
}

__global__ __launch_bounds__(256) void lw_unit_coef_kernel(const double* __restrict__ partial, size_t n_partial, const UnitSlot* __restrict__ slots,
                                                           size_t n_slots, float* __restrict__ v, float* __restrict__ den,
                                                           double* __restrict__ sums, double beta2, double eps) {
  __shared__ double sh[256];
  const int l = threadIdx.x & 63;
  const size_t s = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
  double acc[1] = {};
  bool ok = false;
  if (s < n_slots) {
    const UnitSlot sl = slots[s];
    ok = slot_ok(sl, n_partial);
    if (ok) slot_gather<64>(sl, partial, l, acc);
  }
  const double S = group_sum<64>(acc[0], sh);
  if (l != 0 || !ok) return;
  sums[s] = S;
  const float vn = (float)((double)v[s] * beta2 + (1.0 - beta2) * sqrt(S));  // the NORM, where the layer-wise rule takes S itself
  v[s] = vn;
  den[s] = (float)(sqrt((double)vn) + eps);
}

template <int RULE, bool EMA>
__global__ __launch_bounds__(256) void lw_unit_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ ema, size_t n, const LwItem* __restrict__ items,
                                                             const UnitTensor* __restrict__ tens, int n_tensors, const float* __restrict__ den,
                                                             int n_slots, f32x4 c0, LwUpdArgs a) {
  const LwItem it = items[blockIdx.x];
  if (!item_ok(it, n, n_tensors)) return;
  UnitSpan sp;
  if (!unit_span(it, tens[it.tensor], n_slots, sp)) return;
  const float* d = den + sp.slot0;
  const auto coef_of = [&](int unit) {
    f32x4 c = c0;
    c[0] = d[unit];
    return c;
  };
  const auto elem = [&](const f32x4& c, float& pk, float& gk, float& mk, float& ek) { lw_elem<RULE, EMA>(pk, gk, mk, ek, c, a); };
  unit_item_sweep(it.len, sp, coef_of, elem, upd(p + it.off), last(g + it.off), upd(m + it.off), upd_if<EMA>(ema + it.off));
}

}  // namespace

extern "C" size_t mi355_lw_item_elems(void) { return kLwItemElems; }

extern "C" int mi355_lw_sumsq(const float* src, size_t n, const void* items, size_t n_items, int n_tensors, float scale, void* partial_,
                              void* stream) {
  double* partial = (double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(src && items && partial, "lw_sumsq: null pointer");
  MI355_ARG(aligned16(src) && aligned16(items) && (uintptr_t)partial % 8 == 0, "lw_sumsq: misaligned pointer (16 bytes for the array and the table)");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "lw_sumsq: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  MI355_ARG(std::isfinite(scale), "lw_sumsq: scale=%g is not finite", (double)scale);
  hipLaunchKernelGGL(lw_sumsq_kernel, dim3((unsigned)n_items), dim3(256), 0, st, src, n, (const LwItem*)items, partial, n_tensors, scale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_lw_coef(int rule, int flags, const void* partial_, size_t n_partial, const void* tensors, size_t n_tensors, void* v,
                             float* coef, void* sums_, double beta1, double beta2, double eps, double lr, double wd, double mean, void* stream) {
  const double* partial = (const double*)partial_;
  double* sums = (double*)sums_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(partial && tensors && v && coef && sums, "lw_coef: null pointer");
  MI355_ARG((uintptr_t)partial % 8 == 0 && aligned16(tensors) && aligned16(coef) && (uintptr_t)sums % 8 == 0 &&
                (uintptr_t)v % (rule == 2 ? 8 : 4) == 0,
            "lw_coef: misaligned pointer");
  MI355_ARG(rule >= 0 && rule <= 2, "lw_coef: rule=%d outside 0..2", rule);
  MI355_ARG((flags & ~(LW_MEAN | LW_STABLE_WD | LW_SOFT_WD | LW_SGD_MOM | LW_SQRT_MOM)) == 0, "lw_coef: unknown flag in %d", flags);
  MI355_ARG(n_tensors >= 1 && n_tensors <= kLwMaxGrid && n_partial >= 1, "lw_coef: n_tensors=%zu, n_partial=%zu out of range", n_tensors, n_partial);
  MI355_ARG(beta1 >= 0.0 && beta1 < 1.0, "lw_coef: beta1=%g outside [0, 1)", beta1);
  MI355_ARG(beta2 >= 0.0 && beta2 < 1.0, "lw_coef: beta2=%g outside [0, 1)", beta2);
  MI355_ARG(std::isfinite(eps) && eps >= 0.0, "lw_coef: eps=%g must be finite and >= 0", eps);
  MI355_ARG(std::isfinite(lr) && lr >= 0.0, "lw_coef: lr=%g must be finite and >= 0", lr);
  MI355_ARG(std::isfinite(wd), "lw_coef: weight_decay=%g is not finite", wd);
  MI355_ARG(rule != 2 || (std::isfinite(mean) && mean > 0.0), "lw_coef: mean=%g must be finite and > 0", mean);
  LwCoefArgs a{beta1, beta2, eps, lr, wd, mean, rule, flags};
  hipLaunchKernelGGL(lw_coef_kernel, dim3((unsigned)n_tensors), dim3(64), 0, st, partial, n_partial, (const LwTensor*)tensors, v, coef, sums, a);
  MI355_LAUNCH_CHECK();
  return 0;
}

static int launch_lw_update(int rule, float* p, const float* g, float* m, float* ema, size_t n, const void* items, size_t n_items,
                            const float* coef, int n_tensors, double lr, int soft_wd, double wd_eps, float gscale, float ema_decay,
                            hipStream_t st) {
  MI355_ARG(p && g && m && items && coef, "lw_update: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(ema) && aligned16(items) && aligned16(coef),
            "lw_update: pointers must be 16-byte aligned");
  MI355_ARG(rule >= 0 && rule <= 2, "lw_update: rule=%d outside 0..2", rule);
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "lw_update: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  MI355_ARG(std::isfinite(lr) && lr >= 0.0, "lw_update: lr=%g must be finite and >= 0", lr);
  MI355_ARG(!soft_wd || (rule == 0 && std::isfinite(wd_eps)), "lw_update: wd_eps=%g needs rule 0 and a finite value", wd_eps);
  MI355_ARG(std::isfinite(gscale), "lw_update: grad_scale=%g is not finite", (double)gscale);
  MI355_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "lw_update: ema_decay=%g outside [0, 1]", (double)ema_decay);
  const LwUpdArgs a = lw_upd_args(lr, soft_wd, wd_eps, gscale, ema, ema_decay);
  const dim3 grid((unsigned)n_items);
  const LwItem* it = (const LwItem*)items;
  return with_int<0, 1, 2>(rule, "lw_update", [&](auto RULE) -> int {
    return with_bool(ema != nullptr, [&](auto EMA) -> int {
      hipLaunchKernelGGL((lw_update_kernel<RULE, EMA>), grid, dim3(256), 0, st, p, g, m, ema, n, it, coef, n_tensors, a);
      MI355_LAUNCH_CHECK();
      return 0;
    });
  });
}
extern "C" int mi355_lw_update(int rule, float* p, const float* g, float* m, size_t n, const void* items, size_t n_items, const float* coef,
                               int n_tensors, double lr, int soft_wd, double wd_eps, float grad_scale, void* stream) {
  return launch_lw_update(rule, p, g, m, nullptr, n, items, n_items, coef, n_tensors, lr, soft_wd, wd_eps, grad_scale, 0.f, (hipStream_t)stream);
}
extern "C" int mi355_lw_update_ema(int rule, float* p, const float* g, float* m, float* ema, size_t n, const void* items, size_t n_items,
                                   const float* coef, int n_tensors, double lr, int soft_wd, double wd_eps, float grad_scale, float ema_decay,
                                   void* stream) {
  MI355_ARG(ema, "lw_update_ema: null ema");
  return launch_lw_update(rule, p, g, m, ema, n, items, n_items, coef, n_tensors, lr, soft_wd, wd_eps, grad_scale, ema_decay,
                          (hipStream_t)stream);
}

extern "C" int mi355_lw_unit_sumsq(const float* src, size_t n, const void* pieces, size_t n_pieces, int n_slots, float scale, void* partial_,
                                   void* stream) {
  double* partial = (double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(src && pieces && partial, "lw_unit_sumsq: null pointer");
  MI355_ARG(aligned16(src) && aligned16(pieces) && (uintptr_t)partial % 8 == 0,
            "lw_unit_sumsq: misaligned pointer (16 bytes for the array and the table, 8 for partial[])");
  MI355_ARG(n_pieces >= 1 && n_pieces <= kLwMaxGrid && n_slots >= 1, "lw_unit_sumsq: n_pieces=%zu, n_slots=%d out of range", n_pieces, n_slots);
  MI355_ARG(std::isfinite(scale), "lw_unit_sumsq: scale=%g is not finite", (double)scale);
  hipLaunchKernelGGL(lw_unit_sumsq_kernel, dim3((unsigned)((n_pieces + 3) / 4)), dim3(256), 0, st, src, n, (const UnitPiece*)pieces, n_pieces,
                     n_slots, partial, scale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_lw_unit_coef(const void* partial_, size_t n_partial, const void* slots, size_t n_slots, float* v, float* den, void* sums_,
                                  double beta2, double eps, void* stream) {
  const double* partial = (const double*)partial_;
  double* sums = (double*)sums_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(partial && slots && v && den && sums, "lw_unit_coef: null pointer");
  MI355_ARG((uintptr_t)partial % 8 == 0 && (uintptr_t)slots % 8 == 0 && (uintptr_t)v % 4 == 0 && (uintptr_t)den % 4 == 0 && (uintptr_t)sums % 8 == 0,
            "lw_unit_coef: misaligned pointer (8 bytes for partial[], slots[] and sums[], 4 for v[] and den[])");
  MI355_ARG(n_partial >= 1 && n_partial <= kLwMaxGrid && n_slots >= 1 && n_slots <= kLwMaxGrid, "lw_unit_coef: n_partial=%zu, n_slots=%zu out of range",
            n_partial, n_slots);
  MI355_ARG(beta2 >= 0.0 && beta2 < 1.0, "lw_unit_coef: beta2=%g outside [0, 1)", beta2);
  MI355_ARG(std::isfinite(eps) && eps >= 0.0, "lw_unit_coef: eps=%g must be finite and >= 0", eps);
  hipLaunchKernelGGL(lw_unit_coef_kernel, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, st, partial, n_partial, (const UnitSlot*)slots, n_slots,
                     v, den, sums, beta2, eps);
  MI355_LAUNCH_CHECK();
  return 0;
}

static int launch_lw_unit_update(int rule, float* p, const float* g, float* m, float* ema, size_t n, const void* items, size_t n_items,
                                 const void* tensors, int n_tensors, const float* den, size_t n_slots, double beta1, double lr, double wd,
                                 int soft_wd, double wd_eps, float gscale, float ema_decay, hipStream_t st) {
  MI355_ARG(p && g && m && items && tensors && den, "lw_unit_update: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(ema) && aligned16(items) && aligned16(tensors) && (uintptr_t)den % 4 == 0,
            "lw_unit_update: misaligned pointer (16 bytes for the arrays and the tables, 4 for den[])");
  MI355_ARG(rule >= 0 && rule <= 1, "lw_unit_update: rule=%d outside 0..1", rule);
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1 && n_slots >= 1 && n_slots <= 0x7fffffffu,
            "lw_unit_update: n_items=%zu, n_tensors=%d, n_slots=%zu out of range", n_items, n_tensors, n_slots);
  MI355_ARG(beta1 >= 0.0 && beta1 < 1.0, "lw_unit_update: beta1=%g outside [0, 1)", beta1);
  MI355_ARG(std::isfinite(lr) && lr >= 0.0, "lw_unit_update: lr=%g must be finite and >= 0", lr);
  MI355_ARG(std::isfinite(wd), "lw_unit_update: weight_decay=%g is not finite", wd);
  MI355_ARG(!soft_wd || (rule == 0 && std::isfinite(wd_eps)), "lw_unit_update: wd_eps=%g needs rule 0 and a finite value", wd_eps);
  MI355_ARG(std::isfinite(gscale), "lw_unit_update: grad_scale=%g is not finite", (double)gscale);
  MI355_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "lw_unit_update: ema_decay=%g outside [0, 1]", (double)ema_decay);
  const LwUpdArgs a = lw_upd_args(lr, soft_wd, wd_eps, gscale, ema, ema_decay);
  const double lrwd = lr * wd;
  const f32x4 c0 = {1.f, (float)beta1, (float)(1.0 - beta1), (float)(soft_wd ? lrwd : 1.0 - lrwd)};  // what lw_coef_kernel stores, den aside
  const dim3 grid((unsigned)n_items);
  const LwItem* it = (const LwItem*)items;
  const UnitTensor* tn = (const UnitTensor*)tensors;
  return with_int<0, 1>(rule, "lw_unit_update", [&](auto RULE) -> int {
    return with_bool(ema != nullptr, [&](auto EMA) -> int {
      hipLaunchKernelGGL((lw_unit_update_kernel<RULE, EMA>), grid, dim3(256), 0, st, p, g, m, ema, n, it, tn, n_tensors, den, (int)n_slots, c0, a);
      MI355_LAUNCH_CHECK();
      return 0;
    });
  });
}
extern "C" int mi355_lw_unit_update(int rule, float* p, const float* g, float* m, size_t n, const void* items, size_t n_items, const void* tensors,
                                    int n_tensors, const float* den, size_t n_slots, double beta1, double lr, double weight_decay, int soft_wd,
                                    double wd_eps, float grad_scale, void* stream) {
  return launch_lw_unit_update(rule, p, g, m, nullptr, n, items, n_items, tensors, n_tensors, den, n_slots, beta1, lr, weight_decay, soft_wd,
                               wd_eps, grad_scale, 0.f, (hipStream_t)stream);
}
extern "C" int mi355_lw_unit_update_ema(int rule, float* p, const float* g, float* m, float* ema, size_t n, const void* items, size_t n_items,
                                        const void* tensors, int n_tensors, const float* den, size_t n_slots, double beta1, double lr,
                                        double weight_decay, int soft_wd, double wd_eps, float grad_scale, float ema_decay, void* stream) {
  MI355_ARG(ema, "lw_unit_update_ema: null ema");
  return launch_lw_unit_update(rule, p, g, m, ema, n, items, n_items, tensors, n_tensors, den, n_slots, beta1, lr, weight_decay, soft_wd, wd_eps,
                               grad_scale, ema_decay, (hipStream_t)stream);
}

}  // namespace mi355
