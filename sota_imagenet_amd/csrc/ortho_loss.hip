// ortho_loss.hip — the two parameter-only terms the reference appends to its criterion, over the flat fp32 parameter array (gfx950):
// OrthoLoss, type 1 (sota_imagenet/callbacks.py:126-156, appended by OrthoLossClb, :191-203) and NormLoss (:206-221, NormLossClb :224-229).
//
// OrthoLoss.  mat { RowRecord run; int64 g0; int64 t0 }   32 bytes: a conv weight as run.count = O rows of run.len = K contiguous elements from
//   element run.off (rows.h; any alignment: the stem's rows are 147 long), O <= K; its Gram matrix is gram[g0 .. g0 + O*O), its tiles are
//   tiles[t0 .. t0 + nt (nt + 1) / 2), nt = ceil(O / T), T = MI355_OL_TILE, tile (ti, tj <= ti) at t0 + ti (ti + 1) / 2 + tj.
//   tile { int32 mat; int32 ti | tj << 16; int32 item0; int32 n_slabs }   16 bytes: a T x T tile on or below the diagonal and its n_slabs =
//   ceil(K / MI355_OL_KSLAB) consecutive work items;  item { int32 tile; int32 slab }   8 bytes.
//   G = W W^T - I,  F = |G|_F,  loss += F where F / O > min_norm,  dF/dW = (2 / F) G W  (G is symmetric; 0 where F == 0):
//   ol_gram_kernel     one workgroup per item: the T x T products of rows ti*T.. with rows tj*T.. over the item's K slab, v_mfma_f32_32x32x2_f32
//                      (exact fp32, a k-ordered fmaf chain; four waves, one 32 x 32 quarter each), staged through LDS 32 columns at a time with
//                      scalar loads (a row starts at any element), zeros beyond O and beyond the slab; the partial tile goes to partial[item].
//   ol_finish_kernel   one workgroup per tile: G = (the slab partials added in slab order, fp32) - I, written at (r, c) and, off the diagonal,
//                      mirrored at (c, r); the tile's sum of G^2 in double (fixed tree) -> tile_ss[tile].  A tile one of whose items does not
//                      name it (that item's workgroup wrote no partial) is skipped: tile_ss = 0, G untouched.
//   ol_stats_kernel    ONE workgroup: per matrix, in tile order, ss = sum (diagonal tile ? 1 : 2) tile_ss;  F = (float)sqrt(ss);  ratio = F / (float)O;
//                      gate = ratio > min_norm;  coef = gate && F > 0 ? 2 / F : 0;  stats[4m ..] = { F, ratio, gate, coef };  then thread 0:
//                      loss = (float) sum_m gate F in double, in matrix order.
//   ol_grad_kernel     one workgroup per (matrix, row tile, tile of T columns of K): acc = sum_j G[r, j] W[j, c], j ascending, the same MFMA, the
//                      whole reduction over O inside the workgroup;  dw[r, c] = (accumulate ? dw[r, c] : 0) + (s * coef) * acc, s read from the
//                      device.  A matrix with coef == 0 is left alone (accumulate) or zeroed.
// NormLoss.  items: RowRecord runs of whole rows of one tensor;  tensor { int64 item0; int32 n_items; int32 rows }   16 bytes, item0 ascending.
//   nl_fwd_kernel      one workgroup per item: n_r = sqrt(sum x^2) in double — rows of at most 16 elements one thread each, longer rows one wave
//                      each (piece_sweep, group_sum<64>) —, part[item] = sum_r (1 - n_r)^2 (block_sum<256>).
//   nl_total_kernel    ONE workgroup: tensor_loss[k] = (its items' parts in item order) / rows;  loss = (float) sum_k in tensor order.
//   nl_bwd_kernel      one workgroup per item, n_r again:  dw = (accumulate ? dw : 0) + (float)(s (2 / rows) (n_r - 1) / n_r) * w, 0 where n_r == 0.
// -ffp-contract=off: every operation is rounded on its own.  No floating-point atomics, no flags, no workgroup waits on another: what crosses
// workgroups is left in the scratch by one launch and taken by ONE owner in the next launch on the same stream.  Two runs agree bit for bit.
// A record that does not lie inside its arrays, or does not agree with the records it points to, is skipped before anything is accessed through
// it (its statistics are 0); elements outside the matrices / rows are neither read nor written.
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "rows.h"

namespace mi355 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kT = MI355_OL_TILE;
constexpr int kSlab = MI355_OL_KSLAB;
constexpr int kKc = 32;  // columns staged per step
static_assert(kT == 64, "four waves, one 32 x 32 MFMA quarter each");
static_assert(kSlab % kKc == 0, "a slab is a whole number of staged steps");
constexpr int kMaxRows = 32768;  // O*O and the tile numbers fit an int

struct OrthoMat {
  RowRecord run;  // count = O rows of len = K elements
  long long g0;   // gram[g0 .. g0 + O*O)
  long long t0;   // first tile
};
struct OrthoTile {
  int mat;
  int tij;  // ti | tj << 16
  int item0, n_slabs;
};
struct OrthoItem {
  int tile, slab;
};
struct OrthoGradItem {
  int mat, ti, tc, pad;
};
static_assert(sizeof(OrthoMat) == 32 && sizeof(OrthoTile) == 16 && sizeof(OrthoItem) == 8 && sizeof(OrthoGradItem) == 16, "table records");

struct OlDims {
  size_t n, n_gram, n_mats, n_tiles, n_items;
};

__device__ __forceinline__ int ol_nt(int rows) { return (rows + kT - 1) / kT; }

__device__ __forceinline__ bool ol_mat_ok(const OrthoMat& q, const OlDims& d) {
  if (!rows_ok(q.run.off, q.run.len, q.run.count, d.n) || q.run.count > q.run.len || q.run.count > kMaxRows) return false;
  const size_t oo = (size_t)q.run.count * (size_t)q.run.count;
  const size_t nt = (size_t)ol_nt(q.run.count), tiles = nt * (nt + 1) / 2;
  return q.g0 >= 0 && oo <= d.n_gram && (size_t)q.g0 <= d.n_gram - oo && q.t0 >= 0 && tiles <= d.n_tiles && (size_t)q.t0 <= d.n_tiles - tiles;
}

// tile `idx` of the table: a sound matrix, its own place among that matrix's tiles, and its items inside the item table
__device__ __forceinline__ bool ol_tile_ok(const OrthoTile& tl, size_t idx, const OlDims& d, const OrthoMat* __restrict__ mats, OrthoMat& q, int& ti,
                                           int& tj) {
  if (tl.mat < 0 || (size_t)tl.mat >= d.n_mats) return false;
  q = mats[tl.mat];
  if (!ol_mat_ok(q, d)) return false;
  ti = tl.tij & 0xffff, tj = (tl.tij >> 16) & 0xffff;
  const int nt = ol_nt(q.run.count);
  if (ti >= nt || tj > ti || (size_t)q.t0 + (size_t)(ti * (ti + 1) / 2 + tj) != idx) return false;
  return tl.item0 >= 0 && tl.n_slabs == (q.run.len + kSlab - 1) / kSlab && (size_t)tl.item0 + (size_t)tl.n_slabs <= d.n_items;
}

// the C/D map of v_mfma_f32_32x32x2_f32: register `reg` of lane `lane` is (row, lane & 31) of the 32 x 32 result
__device__ __forceinline__ int mfma_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__global__ __launch_bounds__(256) void ol_gram_kernel(const float* __restrict__ w, float* __restrict__ partial, OlDims d,
                                                      const OrthoMat* __restrict__ mats, const OrthoTile* __restrict__ tiles,
                                                      const OrthoItem* __restrict__ items) {
  __shared__ float sa[kT][kKc + 1], sb[kT][kKc + 1];
  const OrthoItem it = items[blockIdx.x];
  if (it.tile < 0 || (size_t)it.tile >= d.n_tiles) return;  // (every test here is the same for all threads)
  const OrthoTile tl = tiles[it.tile];
  OrthoMat q;
  int ti, tj;
  if (!ol_tile_ok(tl, (size_t)it.tile, d, mats, q, ti, tj)) return;
  if (it.slab < 0 || it.slab >= tl.n_slabs || (size_t)tl.item0 + (size_t)it.slab != blockIdx.x) return;
  const int O = q.run.count, K = q.run.len;
  const int k_begin = it.slab * kSlab, k_end = min(K, k_begin + kSlab);
  const float* base = w + q.run.off;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  const int lc = t & (kKc - 1), lr = t / kKc;  // the thread's column and first row of a staged step
  f32x16 acc = {0};
  for (int k0 = k_begin; k0 < k_end; k0 += kKc) {
    const int k = k0 + lc;
#pragma unroll
    for (int p = 0; p < kT / (256 / kKc); ++p) {
      const int r = lr + p * (256 / kKc);
      const int ga = ti * kT + r, gb = tj * kT + r;
      sa[r][lc] = (ga < O && k < k_end) ? base[(size_t)ga * K + k] : 0.f;
      sb[r][lc] = (gb < O && k < k_end) ? base[(size_t)gb * K + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kKc; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sa[wr * 32 + (lane & 31)][kk + (lane >> 5)], sb[wc * 32 + (lane & 31)][kk + (lane >> 5)], acc, 0, 0, 0);
    __syncthreads();
  }
  float* out = partial + (size_t)blockIdx.x * (kT * kT);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) out[(wr * 32 + mfma_row(reg, lane)) * kT + wc * 32 + (lane & 31)] = acc[reg];
}

__global__ __launch_bounds__(256) void ol_finish_kernel(const float* __restrict__ partial, float* __restrict__ gram, double* __restrict__ tile_ss,
                                                        OlDims d, const OrthoMat* __restrict__ mats, const OrthoTile* __restrict__ tiles,
                                                        const OrthoItem* __restrict__ items) {
  __shared__ double sh[256];
  const OrthoTile tl = tiles[blockIdx.x];
  OrthoMat q;
  int ti = 0, tj = 0;
  bool ok = ol_tile_ok(tl, (size_t)blockIdx.x, d, mats, q, ti, tj);
  if (ok)  // every slab's item names this tile and that slab — what ol_gram_kernel asked before it wrote the partial (the same for all threads)
    for (int j = 0; j < tl.n_slabs; ++j) {
      const OrthoItem it = items[(size_t)tl.item0 + j];
      ok = ok && it.tile == (int)blockIdx.x && it.slab == j;
    }
  double acc = 0.0;
  if (ok) {
    const int O = q.run.count;
    const float* p = partial + (size_t)tl.item0 * (kT * kT);
    float* G = gram + q.g0;
    for (int e = threadIdx.x; e < kT * kT; e += 256) {
      const int gr = ti * kT + (e / kT), gc = tj * kT + (e % kT);
      if (gr >= O || gc >= O) continue;
      float s = p[e];
      for (int j = 1; j < tl.n_slabs; ++j) s += p[(size_t)j * (kT * kT) + e];
      const float g = s - (gr == gc ? 1.f : 0.f);
      G[(size_t)gr * O + gc] = g;
      if (ti != tj) G[(size_t)gc * O + gr] = g;
      acc += (double)g * (double)g;
    }
  }
  const double tot = block_sum<256>(acc, sh);
  if (threadIdx.x == 0) tile_ss[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void ol_stats_kernel(const double* __restrict__ tile_ss, float* stats, float* __restrict__ loss, OlDims d,
                                                       const OrthoMat* __restrict__ mats, float min_norm) {
  for (size_t m = threadIdx.x; m < d.n_mats; m += 256) {
    const OrthoMat q = mats[m];
    float F = 0.f, ratio = 0.f, gate = 0.f, coef = 0.f;
    if (ol_mat_ok(q, d)) {
      const int nt = ol_nt(q.run.count);
      const double* ts = tile_ss + q.t0;
      double ss = 0.0;
      for (int ti = 0; ti < nt; ++ti)
        for (int tj = 0; tj <= ti; ++tj) ss += (ti == tj ? 1.0 : 2.0) * ts[ti * (ti + 1) / 2 + tj];
      F = (float)sqrt(ss);
      ratio = F / (float)q.run.count;
      if (ratio > min_norm) gate = 1.f, coef = F > 0.f ? 2.f / F : 0.f;
    }
    stats[4 * m] = F, stats[4 * m + 1] = ratio, stats[4 * m + 2] = gate, stats[4 * m + 3] = coef;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (size_t m = 0; m < d.n_mats; ++m)
      if (stats[4 * m + 2] != 0.f) tot += (double)stats[4 * m];
    *loss = (float)tot;
  }
}

__global__ __launch_bounds__(256) void ol_grad_kernel(const float* __restrict__ w, float* __restrict__ dw, const float* __restrict__ gram,
                                                      const float* __restrict__ stats, const float* __restrict__ s, OlDims d,
                                                      const OrthoMat* __restrict__ mats, const OrthoGradItem* __restrict__ gitems, int accumulate) {
  __shared__ float sg[kT][kKc + 1], sw[kKc][kT];
  const OrthoGradItem it = gitems[blockIdx.x];
  if (it.mat < 0 || (size_t)it.mat >= d.n_mats) return;  // (every test here is the same for all threads)
  const OrthoMat q = mats[it.mat];
  if (!ol_mat_ok(q, d)) return;
  const int O = q.run.count, K = q.run.len;
  if (it.ti < 0 || it.ti >= ol_nt(O) || it.tc < 0 || it.tc >= (K + kT - 1) / kT) return;
  const float coef = stats[4 * (size_t)it.mat + 3];
  if (coef == 0.f && accumulate) return;
  const float sc = s[0] * coef;
  const float* base = w + q.run.off;
  const float* G = gram + q.g0;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
  f32x16 acc = {0};
  if (coef != 0.f) {
    const int gl = t & (kKc - 1), gr0 = t / kKc;  // G: the thread's column j and first row of a staged step
    const int wl = t & (kT - 1), wr0 = t / kT;    // W: its column c and first row j
    const int c = it.tc * kT + wl;
    for (int j0 = 0; j0 < O; j0 += kKc) {
#pragma unroll
      for (int p = 0; p < kT / (256 / kKc); ++p) {
        const int r = gr0 + p * (256 / kKc), gr = it.ti * kT + r, j = j0 + gl;
        sg[r][gl] = (gr < O && j < O) ? G[(size_t)gr * O + j] : 0.f;
      }
#pragma unroll
      for (int p = 0; p < kKc / (256 / kT); ++p) {
        const int jj = wr0 + p * (256 / kT), j = j0 + jj;
        sw[jj][wl] = (j < O && c < K) ? base[(size_t)j * K + c] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < kKc; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sg[wr * 32 + (lane & 31)][kk + (lane >> 5)], sw[kk + (lane >> 5)][wc * 32 + (lane & 31)], acc, 0, 0, 0);
      __syncthreads();
    }
  }
  const int c = it.tc * kT + wc * 32 + (lane & 31);
  if (c >= K) return;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int gr = it.ti * kT + wr * 32 + mfma_row(reg, lane);
    if (gr >= O) continue;
    float* o = dw + q.run.off + (size_t)gr * K + c;
    const float add = coef != 0.f ? sc * acc[reg] : 0.f;
    *o = (accumulate ? *o : 0.f) + add;
  }
}

// ---- NormLoss -----------------------------------------------------------------------------------------------------------------------------------
constexpr int kThreadRowMax = 16;  // rows up to this length take one thread each (BatchNorm weights: one element), longer rows one wave each

struct NlTensor {
  long long item0;  // its items are items[item0 .. item0 + n_items); item0 ascends with the index
  int n_items;
  int rows;  // R of the mean
};
static_assert(sizeof(NlTensor) == 16, "table records are 16 bytes");

__device__ __forceinline__ bool nl_tensor_ok(const NlTensor& tn, size_t n_items) {
  return tn.item0 >= 0 && tn.n_items >= 1 && tn.rows >= 1 && (size_t)tn.item0 <= n_items && (size_t)tn.n_items <= n_items - (size_t)tn.item0;
}

// the rows of one item, each with its norm in double: short(r, n_r) runs in the one thread that owns row r, wave(r, n_r, active, l) in every lane
// of the wave that owns it.  Every thread of the workgroup passes the same barriers.
template <typename Short, typename Wave>
__device__ __forceinline__ void nl_rows(const float* __restrict__ w, const RowRecord& it, double* sh, Short short_row, Wave wave_row) {
  const int t = threadIdx.x, L = it.len;
  if (L <= kThreadRowMax) {
    for (int r = t; r < it.count; r += 256) {
      const float* x = w + it.off + (long long)r * L;
      double ss = 0.0;
      for (int i = 0; i < L; ++i) ss += (double)x[i] * (double)x[i];
      short_row(r, sqrt(ss));
    }
    return;
  }
  const int l = t & 63, wave = t >> 6;
  for (int r0 = 0; r0 < it.count; r0 += 4) {  // (the same trip count for every thread)
    const int r = r0 + wave;
    const bool active = r < it.count;
    const UnitPiece row = {it.off + (active ? (long long)r * L : 0), L, 0};
    double ss = 0.0;
    if (active) piece_sweep<64>(row, l, [&](float& v) { ss += (double)v * (double)v; }, rd(w + row.off));
    const double tot = group_sum<64>(ss, sh);
    __syncthreads();  // the next round writes sh
    wave_row(row, sqrt(tot), active, l);
  }
}

__global__ __launch_bounds__(256) void nl_fwd_kernel(const float* __restrict__ w, size_t n, double* __restrict__ part, const RowRecord* __restrict__ items) {
  __shared__ double sha[256], shb[256];
  const RowRecord it = items[blockIdx.x];
  double acc = 0.0;
  if (rows_ok(it.off, it.len, it.count, n))  // (the same for every thread)
    nl_rows(
        w, it, sha, [&](int, double nr) { acc += (1.0 - nr) * (1.0 - nr); },
        [&](const UnitPiece&, double nr, bool active, int l) {
          if (active && l == 0) acc += (1.0 - nr) * (1.0 - nr);
        });
  const double tot = block_sum<256>(acc, shb);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void nl_total_kernel(const double* __restrict__ part, double* tensor_loss, float* __restrict__ loss, size_t n_items,
                                                       const NlTensor* __restrict__ tensors, size_t n_tensors) {
  for (size_t k = threadIdx.x; k < n_tensors; k += 256) {
    const NlTensor tn = tensors[k];
    double sum = 0.0;
    if (nl_tensor_ok(tn, n_items)) {
      for (int i = 0; i < tn.n_items; ++i) sum += part[tn.item0 + i];
      sum /= (double)tn.rows;
    }
    tensor_loss[k] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (size_t k = 0; k < n_tensors; ++k) tot += tensor_loss[k];
    *loss = (float)tot;
  }
}

__global__ __launch_bounds__(256) void nl_bwd_kernel(const float* __restrict__ w, float* __restrict__ dw, size_t n, const float* __restrict__ s,
                                                     const RowRecord* __restrict__ items, size_t n_items, const NlTensor* __restrict__ tensors,
                                                     size_t n_tensors, int accumulate) {
  __shared__ double sha[256];
  const RowRecord it = items[blockIdx.x];
  if (!rows_ok(it.off, it.len, it.count, n)) return;  // (the same for every thread)
  size_t lo = 0, hi = n_tensors;
  while (hi - lo > 1) {
    const size_t mid = (lo + hi) >> 1;
    if (tensors[mid].item0 <= (long long)blockIdx.x) lo = mid;
    else hi = mid;
  }
  const NlTensor tn = tensors[lo];
  if (!nl_tensor_ok(tn, n_items) || (long long)blockIdx.x < tn.item0 || (long long)blockIdx.x - tn.item0 >= tn.n_items) return;
  const double s2r = (double)s[0] * (2.0 / (double)tn.rows);
  const bool acc_on = accumulate != 0;
  const auto coef = [&](double nr) { return nr > 0.0 ? (float)(s2r * ((nr - 1.0) / nr)) : 0.f; };
  nl_rows(
      w, it, sha,
      [&](int r, double nr) {
        const float cf = coef(nr);
        const long long o = it.off + (long long)r * it.len;
        for (int i = 0; i < it.len; ++i) dw[o + i] = (acc_on ? dw[o + i] : 0.f) + cf * w[o + i];
      },
      [&](const UnitPiece& row, double nr, bool active, int l) {
        const float cf = coef(nr);
        if (active) piece_sweep<64>(row, l, [&](float& wi, float& di) { di = (acc_on ? di : 0.f) + cf * wi; }, rd(w + row.off), upd_when(dw + row.off, acc_on));
      });
}

bool aligned4(const void* q) { return (uintptr_t)q % 4 == 0; }
bool aligned8(const void* q) { return (uintptr_t)q % 8 == 0; }

}  // namespace

extern "C" size_t mi355_ortho_loss_partial_floats(size_t n_items) { return n_items * (size_t)(kT * kT); }
extern "C" size_t mi355_ortho_loss_stats_floats(size_t n_mats) { return 4 * n_mats; }

extern "C" int mi355_ortho_loss_fwd(const float* w, size_t n, float* gram, size_t n_gram, float* partial, double* tile_ss, float* stats, float* loss,
                                    const void* mats, size_t n_mats, const void* tiles, size_t n_tiles, const void* items, size_t n_items,
                                    float min_norm, void* stream) {
  MI355_ARG(w && gram && partial && tile_ss && stats && loss && mats && tiles && items, "ortho_loss_fwd: null pointer");
  MI355_ARG(aligned16(w) && aligned16(gram) && aligned16(partial) && aligned16(mats) && aligned16(tiles) && aligned8(items) && aligned8(tile_ss) &&
                aligned16(stats) && aligned4(loss),
            "ortho_loss_fwd: misaligned pointer (16 bytes for the arrays, the matrix and tile tables and stats[], 8 for items[] and tile_ss[], 4 for loss)");
  MI355_ARG(n >= 1 && n_gram >= 1 && n_mats >= 1 && n_mats <= 65535 && n_tiles >= 1 && n_tiles <= kLwMaxGrid && n_items >= 1 && n_items <= kLwMaxGrid,
            "ortho_loss_fwd: n=%zu, n_gram=%zu, n_mats=%zu, n_tiles=%zu, n_items=%zu out of range", n, n_gram, n_mats, n_tiles, n_items);
  MI355_ARG(min_norm == min_norm, "ortho_loss_fwd: min_norm is NaN");
  const OlDims d{n, n_gram, n_mats, n_tiles, n_items};
  hipStream_t st = (hipStream_t)stream;
  const OrthoMat* mt = (const OrthoMat*)mats;
  const OrthoTile* tl = (const OrthoTile*)tiles;
  hipLaunchKernelGGL(ol_gram_kernel, dim3((unsigned)n_items), dim3(256), 0, st, w, partial, d, mt, tl, (const OrthoItem*)items);
  hipLaunchKernelGGL(ol_finish_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, partial, gram, tile_ss, d, mt, tl, (const OrthoItem*)items);
  hipLaunchKernelGGL(ol_stats_kernel, dim3(1), dim3(256), 0, st, tile_ss, stats, loss, d, mt, min_norm);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_ortho_loss_bwd(const float* w, float* dw, size_t n, const float* gram, size_t n_gram, const float* stats, const float* s,
                                    const void* mats, size_t n_mats, size_t n_tiles, const void* gitems, size_t n_gitems, int accumulate,
                                    void* stream) {
  MI355_ARG(w && dw && gram && stats && s && mats && gitems, "ortho_loss_bwd: null pointer");
  MI355_ARG(aligned16(w) && aligned16(dw) && aligned16(gram) && aligned16(mats) && aligned16(gitems) && aligned16(stats) && aligned4(s),
            "ortho_loss_bwd: misaligned pointer (16 bytes for the arrays, the tables and stats[], 4 for s)");
  MI355_ARG(w != dw, "ortho_loss_bwd: dw must not be the array w is read from");
  MI355_ARG(n >= 1 && n_gram >= 1 && n_mats >= 1 && n_mats <= 65535 && n_tiles >= 1 && n_tiles <= kLwMaxGrid && n_gitems >= 1 && n_gitems <= kLwMaxGrid,
            "ortho_loss_bwd: n=%zu, n_gram=%zu, n_mats=%zu, n_tiles=%zu, n_gitems=%zu out of range", n, n_gram, n_mats, n_tiles, n_gitems);
  const OlDims d{n, n_gram, n_mats, n_tiles, 0};
  hipLaunchKernelGGL(ol_grad_kernel, dim3((unsigned)n_gitems), dim3(256), 0, (hipStream_t)stream, w, dw, gram, stats, s, d, (const OrthoMat*)mats,
                     (const OrthoGradItem*)gitems, accumulate);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_norm_loss_fwd(const float* w, size_t n, double* part, double* tensor_loss, float* loss, const void* items, size_t n_items,
                                   const void* tensors, size_t n_tensors, void* stream) {
  MI355_ARG(w && part && tensor_loss && loss && items && tensors, "norm_loss_fwd: null pointer");
  MI355_ARG(aligned16(w) && aligned16(items) && aligned16(tensors) && aligned8(part) && aligned8(tensor_loss) && aligned4(loss),
            "norm_loss_fwd: misaligned pointer (16 bytes for the array and the tables, 8 for part[] and tensor_loss[], 4 for loss)");
  MI355_ARG(n >= 1 && n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1 && n_tensors <= 65535, "norm_loss_fwd: n=%zu, n_items=%zu, n_tensors=%zu out of range",
            n, n_items, n_tensors);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(nl_fwd_kernel, dim3((unsigned)n_items), dim3(256), 0, st, w, n, part, (const RowRecord*)items);
  hipLaunchKernelGGL(nl_total_kernel, dim3(1), dim3(256), 0, st, part, tensor_loss, loss, n_items, (const NlTensor*)tensors, n_tensors);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_norm_loss_bwd(const float* w, float* dw, size_t n, const float* s, const void* items, size_t n_items, const void* tensors,
                                   size_t n_tensors, int accumulate, void* stream) {
  MI355_ARG(w && dw && s && items && tensors, "norm_loss_bwd: null pointer");
  MI355_ARG(aligned16(w) && aligned16(dw) && aligned16(items) && aligned16(tensors) && aligned4(s),
            "norm_loss_bwd: misaligned pointer (16 bytes for the arrays and the tables, 4 for s)");
  MI355_ARG(w != dw, "norm_loss_bwd: dw must not be the array w is read from");
  MI355_ARG(n >= 1 && n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1 && n_tensors <= 65535, "norm_loss_bwd: n=%zu, n_items=%zu, n_tensors=%zu out of range",
            n, n_items, n_tensors);
  hipLaunchKernelGGL(nl_bwd_kernel, dim3((unsigned)n_items), dim3(256), 0, (hipStream_t)stream, w, dw, n, s, (const RowRecord*)items, n_items,
                     (const NlTensor*)tensors, n_tensors, accumulate);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
