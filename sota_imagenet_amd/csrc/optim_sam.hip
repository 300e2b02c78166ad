// optim_sam.hip — the device side of the SAMOriginal callback (adaptive sharpness-aware minimization; the reference's
// sota_imagenet/callbacks.py:279-337) on flat fp32 arrays (gfx950).  Between the first backward and the optimizer step the callback moves every
// parameter along its gradient, weighted by the parameter's own magnitude and normalised by ONE statistic of the whole model, runs a second
// forward / backward there, and moves the parameters back.  Four stages on one stream, nothing read back by the host, over the work-item table of
// the layer-wise optimizers (optim_items.h: an item is cut from one tensor's own range, never from padding) and kind[tensor] = 1 for a weight
// (a Parameter with ndim > 1), 0 for every other tensor:
//   ge = g * grad_scale                                                                 (float)
//   (a) sam_sumsq_kernel, one workgroup per item:  w = ge * max(|p|, eta) for weights, w = ge otherwise (float); w * w summed in double — per
//       thread in element order, then the fixed LDS tree of optim_sum.h — into partial[item].  No floating-point atomics.
//   (b) sam_scale_kernel, one workgroup:  S = all partials of the step in a fixed order (double);  norm = max(sqrt(S), 2e-5);
//       out[0] = (float)(rho / norm),  out[1] = (float)norm, each rounded once.
//   (c) sam_perturb_kernel, one workgroup per item, scale = out[0] read once per workgroup:
//       e = (max(p * p, eta) * ge) * scale for weights,  e = ge * scale otherwise;   eps = e;  p = p + e
//   (d) sam_restore_kernel:  p = p - eps over the same items  ((p + e) - e is in general not p bit for bit: the reference's behaviour, kept)
// 8 B / element in (a) (p, g read), 16 B in (c) (p, g read; eps, p written), 12 B in (d) (p, eps read; p written).  Alignment gaps and padding are
// neither read into the sum nor written.  The library builds with -ffp-contract=off: every product and sum above is rounded on its own.
// The loop of (a), (c) and (d) over an item's elements is item_sweep (optim_sweep.h: 256 threads, f32x4 body, scalar tail).
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "optim_sweep.h"
#include "vec.h"

namespace mi355 {
namespace {

__device__ __forceinline__ float sam_w(float p, float ge, bool weight, float eta) { return weight ? ge * fmaxf(fabsf(p), eta) : ge; }
__device__ __forceinline__ float sam_e(float p, float ge, bool weight, float eta, float scale) {
  return weight ? (fmaxf(p * p, eta) * ge) * scale : ge * scale;
}

__global__ __launch_bounds__(256) void sam_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t n,
                                                        const LwItem* __restrict__ items, const int* __restrict__ kind, int n_tensors,
                                                        double* __restrict__ partial, float eta, float gscale) {
  __shared__ double sh[256];
  const LwItem it = items[blockIdx.x];
  double acc = 0.0;
  if (item_ok(it, n, n_tensors)) {
    const bool weight = kind[it.tensor] != 0;
    const auto rule = [&](float& pk, float& gk) {
      const double w = (double)sam_w(pk, gk * gscale, weight, eta);
      acc += w * w;
    };
    item_sweep(it.len, rule, rd(p + it.off), rd(g + it.off));  // both read again by the perturbation: plain loads
  }
  const double tot = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void sam_scale_kernel(const double* __restrict__ partial, size_t n_partial, double rho, float* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  const double S = block_sum<256>(acc, sh);
  if (threadIdx.x != 0) return;
  const double norm = fmax(sqrt(S), 2e-5);
  out[0] = (float)(rho / norm);
  out[1] = (float)norm;
}

__global__ __launch_bounds__(256) void sam_perturb_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ eps, size_t n,
                                                          const LwItem* __restrict__ items, const int* __restrict__ kind, int n_tensors,
                                                          const float* __restrict__ out, float eta, float gscale) {
  const LwItem it = items[blockIdx.x];
  if (!item_ok(it, n, n_tensors)) return;
  const bool weight = kind[it.tensor] != 0;
  const float scale = out[0];
  const auto rule = [&](float& pk, float& gk, float& ek) {
    ek = sam_e(pk, gk * gscale, weight, eta, scale);  // eps is written, never read
    pk = pk + ek;
  };
  item_sweep(it.len, rule, upd(p + it.off), rd(g + it.off), upd(eps + it.off));
}

__global__ __launch_bounds__(256) void sam_restore_kernel(float* __restrict__ p, const float* __restrict__ eps, size_t n,
                                                          const LwItem* __restrict__ items, int n_tensors) {
  const LwItem it = items[blockIdx.x];
  if (!item_ok(it, n, n_tensors)) return;
  item_sweep(it.len, [](float& pk, float& ek) { pk = pk - ek; }, upd(p + it.off), last(eps + it.off));
}

}  // namespace

extern "C" int mi355_sam_sumsq(const float* p, const float* g, size_t n, const void* items, size_t n_items, const int* kind, int n_tensors,
                               float eta, float gscale, void* partial_, void* stream) {
  double* partial = (double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && g && items && kind && partial, "sam_sumsq: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(items) && (uintptr_t)kind % 4 == 0 && (uintptr_t)partial % 8 == 0,
            "sam_sumsq: misaligned pointer (16 bytes for the arrays and the table, 8 for the partial sums)");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "sam_sumsq: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  MI355_ARG(std::isfinite(eta) && eta >= 0.f, "sam_sumsq: eta=%g must be finite and >= 0", (double)eta);
  MI355_ARG(std::isfinite(gscale), "sam_sumsq: grad_scale=%g is not finite", (double)gscale);
  hipLaunchKernelGGL(sam_sumsq_kernel, dim3((unsigned)n_items), dim3(256), 0, st, p, g, n, (const LwItem*)items, kind, n_tensors, partial, eta,
                     gscale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_sam_scale(const void* partial_, size_t n_partial, double rho, float* out, void* stream) {
  const double* partial = (const double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(partial && out, "sam_scale: null pointer");
  MI355_ARG((uintptr_t)partial % 8 == 0 && (uintptr_t)out % 8 == 0, "sam_scale: misaligned pointer (8 bytes for the partial sums and the result)");
  MI355_ARG(n_partial >= 1 && n_partial <= kLwMaxGrid, "sam_scale: n_partial=%zu out of range", n_partial);
  MI355_ARG(std::isfinite(rho) && rho > 0.0, "sam_scale: rho=%g must be finite and > 0", rho);
  hipLaunchKernelGGL(sam_scale_kernel, dim3(1), dim3(256), 0, st, partial, n_partial, rho, out);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_sam_perturb(float* p, const float* g, float* eps, size_t n, const void* items, size_t n_items, const int* kind,
                                 int n_tensors, const float* out, float eta, float gscale, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && g && eps && items && kind && out, "sam_perturb: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(eps) && aligned16(items) && (uintptr_t)kind % 4 == 0 && (uintptr_t)out % 8 == 0,
            "sam_perturb: misaligned pointer (16 bytes for the arrays and the table, 8 for the result of sam_scale)");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "sam_perturb: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  MI355_ARG(std::isfinite(eta) && eta >= 0.f, "sam_perturb: eta=%g must be finite and >= 0", (double)eta);
  MI355_ARG(std::isfinite(gscale), "sam_perturb: grad_scale=%g is not finite", (double)gscale);
  hipLaunchKernelGGL(sam_perturb_kernel, dim3((unsigned)n_items), dim3(256), 0, st, p, g, eps, n, (const LwItem*)items, kind, n_tensors, out, eta,
                     gscale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_sam_restore(float* p, const float* eps, size_t n, const void* items, size_t n_items, int n_tensors, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && eps && items, "sam_restore: null pointer");
  MI355_ARG(aligned16(p) && aligned16(eps) && aligned16(items), "sam_restore: misaligned pointer (16 bytes for the arrays and the table)");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "sam_restore: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  hipLaunchKernelGGL(sam_restore_kernel, dim3((unsigned)n_items), dim3(256), 0, st, p, eps, n, (const LwItem*)items, n_tensors);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
