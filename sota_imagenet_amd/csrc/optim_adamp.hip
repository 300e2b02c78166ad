// optim_adamp.hip — AdamP (`_target_: adamp.AdamP`; the reference's recipes configs/hydra_exp/51.r50_adamp.yaml and 52.r50_adamp_low-eps.yaml) on
// flat fp32 arrays (gfx950): Adam plus a data-dependent projection.  For every tensor with more than one dimension the cosine between gradient
// and weight is taken per output unit and then per whole tensor; where it is under delta / sqrt(row length) the update loses its component along
// the weight and the weight decay is scaled by wd_ratio.
// PROVENANCE: the `adamp` package is neither in the reference tree nor available where this was written.  The rule is the published
// adamp.AdamP.step (package 0.3.0) written down from memory of the public package (include/mi355rn.h states it in full); parity is against a
// torch restatement (tests/adamp_common.py) and is UNPINNED against the package itself.  pytorch_tools.optim.adamp.AdamP (recipes 12, 13) is a
// modified variant whose code is not available: it stays unresolved.
// A step is three stages on one stream, nothing read back by the host, no floating-point atomics, over the tables of optim_items.h exactly as
// item_plan.plan_units builds them (every tensor with ndim > 1 unit by unit, any other tensor one whole slot) and one record per tensor for (b):
//   AdampTensor = { slot0, n_slots, unit_len, kind }, kind 1 for ndim > 1.
// The element arithmetic, float32 with one rounding per operation (-ffp-contract=off; sqrt and '/' correctly rounded), is adamp_elem, which (a)
// and (c) both call, so that both see the same u:
//   ge = g*grad_scale;  m' = b1*m + gw*ge;  v' = b2*v + (g2*ge)*ge;  den = sqrtf(v')/sq2 + eps;  u = m'/den   (nesterov: (b1*m' + gw*ge)/den)
// with b1, gw = 1 - beta1, b2, g2 = 1 - beta2, sq2 = sqrt(1 - beta2^step) and nss = -lr/(1 - beta1^step) formed in double and rounded once.
//   (a) adamp_unit_sums_kernel, one wave per piece, four pieces per workgroup (piece_walk<64>, group_sum<64>): reads p, g, m, v — the OLD m and
//       v, which only (c) writes, later on the same stream — forms u in registers and writes partial[4k .. 4k+3] = (sum ge^2, sum p^2, sum ge*p,
//       sum p*u) of piece k, the operands converted to double before the product, per thread in element order and then the fixed LDS tree.
//   (b) adamp_coef_kernel, one 256-thread workgroup per tensor record of a param group, in double: every slot's consecutive partials summed in
//       order by one thread, cos_slot = |Sgp| / (max(sqrt(Sgg), eps) * max(sqrt(Spp), eps)), its maximum over the slots, the layer sums as the
//       block_sum of the slot sums.  max cos_slot < delta/sqrt(unit_len): mode 1, coef[slot] = (d, s) = (sqrt(Spp) + eps, Spu / (sqrt(Spp) + eps))
//       per slot;  else cos_layer < delta/sqrt(n_slots*unit_len): mode 2, every slot gets the layer's (d, s);  else, and for kind 0, mode 0 and
//       (1, 0).  wdf[tensor] = (float)(1 - lr*wd*(mode ? wd_ratio : 1)), exactly 1 for wd <= 0;  mode[tensor] = mode.
//       s = sum(p*u)/d where the package forms sum((p/d)*u): a deliberate rounding-level deviation — the sum of p*u comes out of (a)'s one pass,
//       the package's form would need a second reduction pass after d is known.
//   (c) adamp_update_kernel<EMA>, one workgroup per item: (m', v', u) from adamp_elem;  pn = p/d;  u = u - pn*s;  p = p*wdf;  p = p + nss*u;
//       m', v', p stored.  With mode 0, (d, s) = (1, 0), this is the plain Adam step.  The slot of an element is slot0 + (offset inside the
//       tensor)/unit_len: unit_item_sweep (optim_items.h).  EMA: ema += (1 - decay)*(p_new - ema).
// Traffic: 16 B / element in (a), 28 B in (c) (36 B with the average): 44 B a step against AdamW's 28 B.  There is no separate moments pass.
// Every table record is checked against the arrays of the launch before any access through it.
#include <cmath>

#include "common.h"
#include "dispatch.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "optim_sweep.h"
#include "vec.h"

namespace mi355 {
namespace {

struct AdampTensor {
  int slot0, n_slots;  // the tensor's consecutive slots
  int unit_len;        // elements per slot
  int kind;            // 1: ndim > 1, the projection applies; 0: any other tensor
};
static_assert(sizeof(AdampTensor) == 16, "table records are 16 bytes");

struct AdampArgs {
  float b1, gw, b2, g2, sq2, eps, nss, gscale, ema_w;
  bool nesterov;
};

// the moments and the Adam direction of one element; (a) and (c) see the same u because both call this
__device__ __forceinline__ void adamp_elem(float g, float m, float v, const AdampArgs& a, float& mn, float& vn, float& u) {
  const float ge = g * a.gscale;
  mn = a.b1 * m + a.gw * ge;
  vn = a.b2 * v + (a.g2 * ge) * ge;
  const float den = sqrtf(vn) / a.sq2 + a.eps;
  u = a.nesterov ? (a.b1 * mn + a.gw * ge) / den : mn / den;
}

// (86 VGPRs, 5 waves per SIMD.  Bound to 8 waves the compiler takes 62 VGPRs without scratch and the kernel takes the same time: 80.8 against
// 80.5 us on the ResNet-50 array, so it is left alone)
__global__ __launch_bounds__(256) void adamp_unit_sums_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                              const float* __restrict__ m, const float* __restrict__ v, size_t n,
                                                              const UnitPiece* __restrict__ pieces, size_t n_pieces, int n_slots,
                                                              double* __restrict__ partial, AdampArgs a) {
  const auto add = [&](double(&acc)[4], float pk, float gk, float mk, float vk) {
    float mn, vn, u;
    adamp_elem(gk, mk, vk, a, mn, vn, u);
    const double ge = (double)(gk * a.gscale), pd = (double)pk;
    acc[0] += ge * ge;
    acc[1] += pd * pd;
    acc[2] += ge * pd;
    acc[3] += pd * (double)u;
  };
  __shared__ double sh[4][256];
  piece_sums<64>(pieces, n_pieces, n, n_slots, partial, {sh[0], sh[1], sh[2], sh[3]}, add, p, g, m, v);
}

struct AdampCoefArgs {
  double lr, wd, eps, delta, wd_ratio;
};

__device__ __forceinline__ double adamp_cos(double Sgg, double Spp, double Sgp, double eps) {
  return fabs(Sgp) / (fmax(sqrt(Sgg), eps) * fmax(sqrt(Spp), eps));
}

__global__ __launch_bounds__(256) void adamp_coef_kernel(const double* __restrict__ partial, size_t n_partial, const UnitSlot* __restrict__ slots,
                                                         size_t n_slots, const AdampTensor* __restrict__ tens, float* __restrict__ coef,
                                                         float* __restrict__ wdf, int* __restrict__ mode, AdampCoefArgs a) {
  __shared__ double sh[256];
  __shared__ int bad;
  const AdampTensor t = tens[blockIdx.x];
  if (t.slot0 < 0 || t.n_slots <= 0 || t.unit_len <= 0 || (size_t)t.slot0 + (size_t)t.n_slots > n_slots) return;  // (the same for every thread)
  float2* c = reinterpret_cast<float2*>(coef) + t.slot0;
  const double lrwd = a.lr * a.wd;
  int md = 0;
  double dl = 1.0, sl = 0.0;  // the layer's (d, s)
  if (t.kind == 1) {
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    // the sums of slot j, its consecutive entries of partial[] in order
    const auto slot_sums = [&](int j, double& Sgg, double& Spp, double& Sgp, double& Spu) {
      const UnitSlot s = slots[t.slot0 + j];
      Sgg = Spp = Sgp = Spu = 0.0;
      if (!slot_ok(s, n_partial)) return false;
      for (int i = 0; i < s.count; ++i) {
        const double* q = partial + 4 * ((size_t)s.first + i);
        Sgg += q[0], Spp += q[1], Sgp += q[2], Spu += q[3];
      }
      return true;
    };
    double lgg = 0.0, lpp = 0.0, lgp = 0.0, lpu = 0.0, cmax = 0.0;
    for (int j = threadIdx.x; j < t.n_slots; j += 256) {
      double Sgg, Spp, Sgp, Spu;
      if (!slot_sums(j, Sgg, Spp, Sgp, Spu)) bad = 1;
      lgg += Sgg, lpp += Spp, lgp += Sgp, lpu += Spu;
      const double cs = adamp_cos(Sgg, Spp, Sgp, a.eps);
      cmax = (cs > cmax || cs != cs) ? cs : cmax;  // a NaN cosine is never under the threshold: keep it
    }
    // block_sum ends on a barrier after its last write and before its result is read: sh may be reused after one more barrier
    const double Lgg = block_sum<256>(lgg, sh);
    __syncthreads();
    const double Lpp = block_sum<256>(lpp, sh);
    __syncthreads();
    const double Lgp = block_sum<256>(lgp, sh);
    __syncthreads();
    const double Lpu = block_sum<256>(lpu, sh);
    __syncthreads();
    sh[threadIdx.x] = cmax;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) {
        const double x = sh[threadIdx.x], y = sh[threadIdx.x + w];
        sh[threadIdx.x] = (y > x || y != y) ? y : x;
      }
      __syncthreads();
    }
    const double cunits = sh[0];
    if (bad) return;  // a slot record outside partial[]: the tensor is skipped (the same for every thread)
    const double len = (double)t.unit_len;
    if (cunits < a.delta / sqrt(len)) {
      md = 1;
      for (int j = threadIdx.x; j < t.n_slots; j += 256) {
        double Sgg, Spp, Sgp, Spu;
        slot_sums(j, Sgg, Spp, Sgp, Spu);
        const double d = sqrt(Spp) + a.eps;
        c[j] = make_float2((float)d, (float)(Spu / d));
      }
    } else if (adamp_cos(Lgg, Lpp, Lgp, a.eps) < a.delta / sqrt((double)t.n_slots * len)) {
      md = 2;
      dl = sqrt(Lpp) + a.eps;
      sl = Lpu / dl;
    }
  }
  if (md != 1) {
    const float2 cl = make_float2((float)dl, (float)sl);
    for (int j = threadIdx.x; j < t.n_slots; j += 256) c[j] = cl;
  }
  if (threadIdx.x == 0) {
    wdf[blockIdx.x] = a.wd > 0.0 ? (float)(1.0 - lrwd * (md ? a.wd_ratio : 1.0)) : 1.0f;
    mode[blockIdx.x] = md;
  }
}

template <bool EMA>
__device__ __forceinline__ void adamp_step_elem(float& p, float g, float& m, float& v, float& e, float d, float s, float wdf, const AdampArgs& a) {
  float mn, vn, u;
  adamp_elem(g, m, v, a, mn, vn, u);
  const float pn = p / d;
  u = u - pn * s;
  float pe = p * wdf;
  pe = pe + a.nss * u;
  m = mn, v = vn, p = pe;
  if constexpr (EMA) e = e + a.ema_w * (pe - e);
}

template <bool EMA>
__global__ __launch_bounds__(256) void adamp_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ ema, size_t n,
                                                           const LwItem* __restrict__ items, const UnitTensor* __restrict__ tens, int n_tensors,
                                                           const float* __restrict__ coef, int n_slots, const float* __restrict__ wdfs,
                                                           AdampArgs a) {
  const LwItem it = items[blockIdx.x];
  if (!item_ok(it, n, n_tensors)) return;
  UnitSpan sp;
  if (!unit_span(it, tens[it.tensor], n_slots, sp)) return;
  const float2* c = reinterpret_cast<const float2*>(coef) + sp.slot0;
  const float wdf = wdfs[it.tensor];
  const auto elem = [&](const float2& ds, float& pk, float& gk, float& mk, float& vk, float& ek) {
    adamp_step_elem<EMA>(pk, gk, mk, vk, ek, ds.x, ds.y, wdf, a);
  };
  unit_item_sweep(it.len, sp, [&](int unit) { return c[unit]; }, elem, upd(p + it.off), last(g + it.off), upd(m + it.off), upd(v + it.off),
                  upd_if<EMA>(ema + it.off));
}

// the scalars both (a) and (c) need, formed in double and rounded once; false with a message for values outside the rule's domain
bool adamp_args(const char* who, double beta1, double beta2, double eps, double lr, int step, int nesterov, float gscale, AdampArgs& a) {
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return set_error("%s: betas=(%g, %g) outside [0, 1)", who, beta1, beta2), false;
  if (!(std::isfinite(eps) && eps >= 0.0)) return set_error("%s: eps=%g must be finite and >= 0", who, eps), false;
  if (!(std::isfinite(lr) && lr >= 0.0)) return set_error("%s: lr=%g must be finite and >= 0", who, lr), false;
  if (step < 1) return set_error("%s: step=%d must be >= 1 (the count after this step's increment)", who, step), false;
  if (!std::isfinite(gscale)) return set_error("%s: grad_scale=%g is not finite", who, (double)gscale), false;
  const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
  a.b1 = (float)beta1, a.gw = (float)(1.0 - beta1), a.b2 = (float)beta2, a.g2 = (float)(1.0 - beta2);
  a.sq2 = (float)std::sqrt(bc2), a.eps = (float)eps, a.nss = (float)(-lr / bc1);
  a.gscale = gscale, a.ema_w = 0.f, a.nesterov = nesterov != 0;
  return true;
}

}  // namespace

extern "C" int mi355_adamp_unit_sums(const float* p, const float* g, const float* m, const float* v, size_t n, const void* pieces,
                                     size_t n_pieces, int n_slots, double beta1, double beta2, double eps, int step, int nesterov, float gscale,
                                     void* partial_, void* stream) {
  double* partial = (double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && g && m && v && pieces && partial, "adamp_unit_sums: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(pieces) && (uintptr_t)partial % 8 == 0,
            "adamp_unit_sums: misaligned pointer (16 bytes for the arrays and the table, 8 for partial[])");
  MI355_ARG(n_pieces >= 1 && n_pieces <= kLwMaxGrid && n_slots >= 1, "adamp_unit_sums: n_pieces=%zu, n_slots=%d out of range", n_pieces, n_slots);
  AdampArgs a;
  if (!adamp_args("adamp_unit_sums", beta1, beta2, eps, 0.0, step, nesterov, gscale, a)) return MI355_E_ARG;
  hipLaunchKernelGGL(adamp_unit_sums_kernel, dim3((unsigned)((n_pieces + 3) / 4)), dim3(256), 0, st, p, g, m, v, n, (const UnitPiece*)pieces,
                     n_pieces, n_slots, partial, a);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_adamp_coef(const void* partial_, size_t n_partial, const void* slots, size_t n_slots, const void* tensors, size_t n_tensors,
                                float* coef, float* wdf, int* mode, double lr, double wd, double eps, double delta, double wd_ratio,
                                void* stream) {
  const double* partial = (const double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(partial && slots && tensors && coef && wdf && mode, "adamp_coef: null pointer");
  MI355_ARG((uintptr_t)partial % 8 == 0 && (uintptr_t)slots % 8 == 0 && aligned16(tensors) && (uintptr_t)coef % 8 == 0 && (uintptr_t)wdf % 4 == 0 &&
                (uintptr_t)mode % 4 == 0,
            "adamp_coef: misaligned pointer (16 bytes for the tensor records, 8 for partial[], slots[] and coef[], 4 for wdf[] and mode[])");
  MI355_ARG(n_partial >= 1 && n_partial <= kLwMaxGrid && n_slots >= 1 && n_slots <= 0x7fffffffu && n_tensors >= 1 && n_tensors <= kLwMaxGrid,
            "adamp_coef: n_partial=%zu, n_slots=%zu, n_tensors=%zu out of range", n_partial, n_slots, n_tensors);
  MI355_ARG(std::isfinite(lr) && lr >= 0.0, "adamp_coef: lr=%g must be finite and >= 0", lr);
  MI355_ARG(std::isfinite(wd), "adamp_coef: weight_decay=%g is not finite", wd);
  MI355_ARG(std::isfinite(eps) && eps >= 0.0, "adamp_coef: eps=%g must be finite and >= 0", eps);
  MI355_ARG(std::isfinite(delta) && delta >= 0.0, "adamp_coef: delta=%g must be finite and >= 0", delta);
  MI355_ARG(std::isfinite(wd_ratio) && wd_ratio >= 0.0, "adamp_coef: wd_ratio=%g must be finite and >= 0", wd_ratio);
  const AdampCoefArgs a{lr, wd, eps, delta, wd_ratio};
  hipLaunchKernelGGL(adamp_coef_kernel, dim3((unsigned)n_tensors), dim3(256), 0, st, partial, n_partial, (const UnitSlot*)slots, n_slots,
                     (const AdampTensor*)tensors, coef, wdf, mode, a);
  MI355_LAUNCH_CHECK();
  return 0;
}

static int launch_adamp_update(float* p, const float* g, float* m, float* v, float* ema, size_t n, const void* items, size_t n_items,
                               const void* tensors, int n_tensors, const float* coef, size_t n_slots, const float* wdf, double lr, double beta1,
                               double beta2, double eps, int step, int nesterov, float gscale, float ema_decay, hipStream_t st) {
  MI355_ARG(p && g && m && v && items && tensors && coef && wdf, "adamp_update: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(ema) && aligned16(items) && aligned16(tensors) &&
                (uintptr_t)coef % 8 == 0 && (uintptr_t)wdf % 4 == 0,
            "adamp_update: misaligned pointer (16 bytes for the arrays and the tables, 8 for coef[], 4 for wdf[])");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1 && n_slots >= 1 && n_slots <= 0x7fffffffu,
            "adamp_update: n_items=%zu, n_tensors=%d, n_slots=%zu out of range", n_items, n_tensors, n_slots);
  MI355_ARG(!ema || (ema_decay >= 0.f && ema_decay <= 1.f), "adamp_update: ema_decay=%g outside [0, 1]", (double)ema_decay);
  AdampArgs a;
  if (!adamp_args("adamp_update", beta1, beta2, eps, lr, step, nesterov, gscale, a)) return MI355_E_ARG;
  a.ema_w = ema ? 1.f - ema_decay : 0.f;
  const dim3 grid((unsigned)n_items);
  return with_bool(ema != nullptr, [&](auto EMA) -> int {
    hipLaunchKernelGGL((adamp_update_kernel<EMA>), grid, dim3(256), 0, st, p, g, m, v, ema, n, (const LwItem*)items, (const UnitTensor*)tensors,
                       n_tensors, coef, (int)n_slots, wdf, a);
    MI355_LAUNCH_CHECK();
    return 0;
  });
}
extern "C" int mi355_adamp_update(float* p, const float* g, float* m, float* v, size_t n, const void* items, size_t n_items, const void* tensors,
                                  int n_tensors, const float* coef, size_t n_slots, const float* wdf, double lr, double beta1, double beta2,
                                  double eps, int step, int nesterov, float grad_scale, void* stream) {
  return launch_adamp_update(p, g, m, v, nullptr, n, items, n_items, tensors, n_tensors, coef, n_slots, wdf, lr, beta1, beta2, eps, step,
                             nesterov, grad_scale, 0.f, (hipStream_t)stream);
}
extern "C" int mi355_adamp_update_ema(float* p, const float* g, float* m, float* v, float* ema, size_t n, const void* items, size_t n_items,
                                      const void* tensors, int n_tensors, const float* coef, size_t n_slots, const float* wdf, double lr,
                                      double beta1, double beta2, double eps, int step, int nesterov, float grad_scale, float ema_decay,
                                      void* stream) {
  MI355_ARG(ema, "adamp_update_ema: null ema");
  return launch_adamp_update(p, g, m, v, ema, n, items, n_items, tensors, n_tensors, coef, n_slots, wdf, lr, beta1, beta2, eps, step, nesterov,
                             grad_scale, ema_decay, (hipStream_t)stream);
}

}  // namespace mi355
