// optim_sam_lw.hip — the device side of the SAM callback (the reference's sota_imagenet/callbacks.py:339-420 with unitwise_norm :269-276) on flat
// fp32 arrays (gfx950).  Where SAMOriginal (optim_sam.hip) normalises by ONE statistic of the whole model, SAM scales the perturbation slot by
// slot: a slot is a whole tensor, or — unit-wise, for tensors with more than one dimension — one output unit of it, a contiguous run of
// unit_len = numel / shape[0] elements (a filter of a conv, a row of the FC).  With ge = g * grad_scale (float), per slot:
//   gn = max(||ge||_2, 1e-5)   wn = max(||p||_2, 1e-3)   c = wn / gn        e = (c * ge) * rho;  eps = e;  p = p + e
// Stages on one stream, nothing read back by the host, no floating-point atomics:
//   (a) sam_lw_sumsq_kernel, one workgroup per work item (optim_items.h) of the whole-tensor slots:  partial[2i] = sum (double)ge^2,
//       partial[2i+1] = sum (double)p^2 — per thread in element order, then the fixed LDS tree of optim_sum.h.
//   (a') sam_unit_sumsq_kernel<G>, G = 64 or 256 threads per piece, 256 / G pieces per workgroup: the same two sums over a table of pieces
//       { int64 off; int32 len; int32 slot } cut from ONE unit each (a unit longer than an item is several pieces).  A unit starts at any
//       element offset (the stem's rows are 147 long): a scalar head up to the next 16-byte boundary, an f32x4 body, a scalar tail.
//   (b) sam_lw_coef_kernel, one wave per slot, 4 slots per workgroup: Sg, Sp = the slot's consecutive partials in a fixed order (double);
//       gn = fmaxf((float)sqrt(Sg), 1e-5f);  wn = fmaxf((float)sqrt(Sp), 1e-3f);  coef[slot] = wn / gn;  norms[slot] = (gn, wn).
//   (c) sam_lw_perturb_kernel, one workgroup per work item of ALL tensors.  The slot of an element is slot0 + (its offset inside its tensor) /
//       unit_len, from the tensor's 16-byte record { int64 start; int32 unit_len; int32 slot0 }: unit_item_sweep (optim_items.h).
//   (d) restore: sam_restore_kernel of optim_sam.hip, unchanged.
// 8 B / element in (a) and (a'), 16 B in (c): the bytes of sam_sumsq_kernel and sam_perturb_kernel.  Alignment gaps and padding are neither read
// into a sum nor written.  Every record is checked against the arrays of the launch before any access through it.  -ffp-contract=off: every
// product and sum is rounded on its own.
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "optim_sweep.h"
#include "vec.h"

namespace mi355 {
namespace {

__global__ __launch_bounds__(256) void sam_lw_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t n,
                                                           const LwItem* __restrict__ items, int n_tensors, double* __restrict__ partial,
                                                           float gscale) {
  __shared__ double shg[256], shp[256];
  const LwItem it = items[blockIdx.x];
  double ag = 0.0, ap = 0.0;
  if (item_ok(it, n, n_tensors)) {
    const auto rule = [&](float& pk, float& gk) {
      const double ge = (double)(gk * gscale), pd = (double)pk;
      ag += ge * ge;
      ap += pd * pd;
    };
    item_sweep(it.len, rule, rd(p + it.off), rd(g + it.off));  // both read again by the perturbation: plain loads
  }
  const double sg = block_sum<256>(ag, shg), sp = block_sum<256>(ap, shp);
  if (threadIdx.x == 0) {
    partial[2 * (size_t)blockIdx.x] = sg;
    partial[2 * (size_t)blockIdx.x + 1] = sp;
  }
}

template <int G>
__global__ __launch_bounds__(256) void sam_unit_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g, size_t n,
                                                             const UnitPiece* __restrict__ pieces, size_t n_pieces, int n_slots,
                                                             double* __restrict__ partial, float gscale) {
  const auto add = [&](double(&acc)[2], float pk, float gk) {
    const double ge = (double)(gk * gscale), pd = (double)pk;
    acc[0] += ge * ge;
    acc[1] += pd * pd;
  };
  __shared__ double shg[256], shp[256];
  piece_sums<G>(pieces, n_pieces, n, n_slots, partial, {shg, shp}, add, p, g);
}

__global__ __launch_bounds__(256) void sam_lw_coef_kernel(const double* __restrict__ partial, size_t n_partial, const UnitSlot* __restrict__ slots,
                                                          size_t n_slots, float* __restrict__ coef, float* __restrict__ norms) {
  __shared__ double shg[256], shp[256];
  const int l = threadIdx.x & 63;
  const size_t s = (size_t)blockIdx.x * 4 + threadIdx.x / 64;
  // slot_ok and slot_gather<64, 2> written out: with them this kernel measured 0.5 % slower (profiles/optim_units_ab.json)
  double ag = 0.0, ap = 0.0;
  bool ok = false;
  if (s < n_slots) {
    const UnitSlot sl = slots[s];
    ok = sl.first >= 0 && sl.count > 0 && (size_t)sl.first + (size_t)sl.count <= n_partial;
    if (ok)
      for (int i = l; i < sl.count; i += 64) {
        ag += partial[2 * ((size_t)sl.first + i)];
        ap += partial[2 * ((size_t)sl.first + i) + 1];
      }
  }
  const double Sg = group_sum<64>(ag, shg), Sp = group_sum<64>(ap, shp);
  if (l != 0 || !ok) return;
  const float gn = fmaxf((float)sqrt(Sg), 1e-5f), wn = fmaxf((float)sqrt(Sp), 1e-3f);
  coef[s] = wn / gn;
  norms[2 * s] = gn;
  norms[2 * s + 1] = wn;
}

__global__ __launch_bounds__(256) void sam_lw_perturb_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ eps, size_t n,
                                                             const LwItem* __restrict__ items, const UnitTensor* __restrict__ tens, int n_tensors,
                                                             const float* __restrict__ coef, int n_slots, float rho, float gscale) {
  const LwItem it = items[blockIdx.x];
  if (!item_ok(it, n, n_tensors)) return;
  UnitSpan sp;
  if (!unit_span(it, tens[it.tensor], n_slots, sp)) return;
  const float* c = coef + sp.slot0;
  const auto elem = [&](const float& ck, float& pk, float& gk, float& ek) {
    ek = (ck * (gk * gscale)) * rho;  // eps is written, never read
    pk = pk + ek;
  };
  unit_item_sweep(it.len, sp, [&](int unit) { return c[unit]; }, elem, upd(p + it.off), rd(g + it.off), upd(eps + it.off));
}

}  // namespace

extern "C" int mi355_sam_lw_sumsq(const float* p, const float* g, size_t n, const void* items, size_t n_items, int n_tensors, float gscale,
                                  void* partial_, void* stream) {
  double* partial = (double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && g && items && partial, "sam_lw_sumsq: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(items) && aligned16(partial),
            "sam_lw_sumsq: misaligned pointer (16 bytes for the arrays, the table and the pairs of partial sums)");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "sam_lw_sumsq: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  MI355_ARG(std::isfinite(gscale), "sam_lw_sumsq: grad_scale=%g is not finite", (double)gscale);
  hipLaunchKernelGGL(sam_lw_sumsq_kernel, dim3((unsigned)n_items), dim3(256), 0, st, p, g, n, (const LwItem*)items, n_tensors, partial, gscale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_sam_unit_sumsq(const float* p, const float* g, size_t n, const void* pieces, size_t n_pieces, int n_slots, float gscale,
                                    void* partial_, int threads_per_piece, void* stream) {
  double* partial = (double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && g && pieces && partial, "sam_unit_sumsq: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(pieces) && aligned16(partial),
            "sam_unit_sumsq: misaligned pointer (16 bytes for the arrays, the table and the pairs of partial sums)");
  MI355_ARG(n_pieces >= 1 && n_pieces <= kLwMaxGrid && n_slots >= 1, "sam_unit_sumsq: n_pieces=%zu, n_slots=%d out of range", n_pieces, n_slots);
  MI355_ARG(std::isfinite(gscale), "sam_unit_sumsq: grad_scale=%g is not finite", (double)gscale);
  MI355_ARG(threads_per_piece == 64 || threads_per_piece == 256, "sam_unit_sumsq: threads_per_piece=%d must be 64 or 256", threads_per_piece);
  const UnitPiece* pc = (const UnitPiece*)pieces;
  if (threads_per_piece == 64)
    hipLaunchKernelGGL(sam_unit_sumsq_kernel<64>, dim3((unsigned)((n_pieces + 3) / 4)), dim3(256), 0, st, p, g, n, pc, n_pieces, n_slots, partial,
                       gscale);
  else
    hipLaunchKernelGGL(sam_unit_sumsq_kernel<256>, dim3((unsigned)n_pieces), dim3(256), 0, st, p, g, n, pc, n_pieces, n_slots, partial, gscale);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_sam_lw_coef(const void* partial_, size_t n_partial, const void* slots, size_t n_slots, float* coef, float* norms,
                                 void* stream) {
  const double* partial = (const double*)partial_;
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(partial && slots && coef && norms, "sam_lw_coef: null pointer");
  MI355_ARG(aligned16(partial) && (uintptr_t)slots % 8 == 0 && (uintptr_t)coef % 4 == 0 && (uintptr_t)norms % 8 == 0,
            "sam_lw_coef: misaligned pointer (16 bytes for the pairs of partial sums, 8 for the slot table and norms[], 4 for coef[])");
  MI355_ARG(n_partial >= 1 && n_partial <= kLwMaxGrid && n_slots >= 1 && n_slots <= kLwMaxGrid, "sam_lw_coef: n_partial=%zu, n_slots=%zu out of range",
            n_partial, n_slots);
  hipLaunchKernelGGL(sam_lw_coef_kernel, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, st, partial, n_partial, (const UnitSlot*)slots, n_slots,
                     coef, norms);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_sam_lw_perturb(float* p, const float* g, float* eps, size_t n, const void* items, size_t n_items, const void* tensors,
                                    int n_tensors, const float* coef, size_t n_slots, double rho, float gscale, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(p && g && eps && items && tensors && coef, "sam_lw_perturb: null pointer");
  MI355_ARG(aligned16(p) && aligned16(g) && aligned16(eps) && aligned16(items) && aligned16(tensors) && (uintptr_t)coef % 4 == 0,
            "sam_lw_perturb: misaligned pointer (16 bytes for the arrays and the tables, 4 for coef[])");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1 && n_slots >= 1 && n_slots <= kLwMaxGrid,
            "sam_lw_perturb: n_items=%zu, n_tensors=%d, n_slots=%zu out of range", n_items, n_tensors, n_slots);
  MI355_ARG(std::isfinite(rho) && rho >= 0.0, "sam_lw_perturb: rho=%g must be finite and >= 0", rho);
  MI355_ARG(std::isfinite(gscale), "sam_lw_perturb: grad_scale=%g is not finite", (double)gscale);
  hipLaunchKernelGGL(sam_lw_perturb_kernel, dim3((unsigned)n_items), dim3(256), 0, st, p, g, eps, n, (const LwItem*)items,
                     (const UnitTensor*)tensors, n_tensors, coef, (int)n_slots, (float)rho, gscale);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
