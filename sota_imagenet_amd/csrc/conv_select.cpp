// conv_select.cpp — which kernel a convolution launch goes to.  Host code only: the one search per launch (select_bf16; launch_igemm_fp8 has two candidates),
// the questions the executors ask of it before they build a launch (igemm_*_legal), and the switch that launches what was found.
// The thresholds are the ends of A/B measurements; their comments are the record of why each is what it is.
#include <cstdio>

#include "conv_kernels.h"

namespace mi355 {

namespace {

constexpr int BKB = 128;  // bytes of K per slab of the implicit-GEMM kernels (= one LDS row)

int max_taps(const IgemmArgs& a, int nclass) {
  int m = 0;
  for (int ci = 0; ci < nclass; ++ci) m = a.cls[ci].ntaps > m ? a.cls[ci].ntaps : m;
  return m;
}

// Which bf16 launches go to the 8-wave ping-pong kernel, and with which tile.  MI355_IGEMM8 in the environment:
//   "0" never;  "<BM>x<BN>[k][f]" (e.g. 256x256, 224x128kf) forces that tile wherever it is legal (k: channel chunks
//   outer, taps inner; f: the fat-phase form);  unset: the measured rule below.
bool choose_igemm8(const IgemmArgs& a, int nclass, ConvPick* p) {
  const char* env = knobs().has_igemm8 ? knobs().igemm8 : nullptr;
  if (env && env[0] == '0') return false;
  if (env && env[0]) {
    int m = 0, n = 0;
    char k1 = 0, k2 = 0;
    if (sscanf(env, "%dx%d%c%c", &m, &n, &k1, &k2) >= 2 && (m == 256 || m == 224) && (n == 256 || n == 128) && igemm8_legal(a, nclass, n)) {
      p->bm = m; p->bn = n; p->korder = k1 == 'k' || k2 == 'k'; p->fat = k1 == 'f' || k2 == 'f';
      return true;
    }
    return false;
  }
  // Measured per layer shape at batch 256 (tools/conv8_check.py, same-process A/B against the 4-wave tiles):
  //  - >= 256 output columns and a reduction of >= 256: the 224 x 256 tile wins on every layer-3/4 shape as long as its
  //    tile count still covers most of the 256 CUs (it is bound by fragment reads + LDS-DMA issue, not by MFMAs, and a
  //    224-row tile has 1/8 fewer A reads than a 256-row one; 224 divides the 49 * 2^k * N pixel counts);
  //  - the 512-column layer-4 3x3 (98 tiles of 256 x 256, 112 of 224 x 256): 256 x 128 fat phases, 196 tiles.
  const int mt = max_taps(a, nclass);
  const long K = (long)mt * a.Ck;
  const long M = (long)a.N * a.Hsub * a.Wsub;
  //  - NOT the output-heavy launches: one workgroup per CU runs its epilogue with the matrix pipe idle, so a short
  //    reduction under a long epilogue (conv1's dgrad: K = 256 / 512 into 1024 / 2048 columns, + shortcut addend + the
  //    BN-backward sums) loses 10-65 us per launch against two independent 4-wave workgroups per CU, and so does a
  //    multi-round launch of short tap classes (the stride-2 3x3 dgrad of layer 3) — measured in the executor,
  //    profiles/r02a_conv_per_layer_bf16_serial_{old,rule}.txt.
  const bool heavy_epilogue = (a.addend != nullptr && K < 1024);
  // k order of a multi-tap launch: channel chunks outer, taps inner — the 9 taps of a 64-channel chunk re-read the same
  // A rows back to back, so they are served from the XCD's L2 instead of being fetched again from beyond it (layer-4 3x3:
  // 373 -> see 77 MB per launch for 25.7 MB of activations, profiles/r02c_pmc_per_conv_launch_bf16_serial.txt; same speed)
  const int ko = (mt > 1 && a.Ck > 64) ? 1 : 0;
  if (a.Ncols % 256 == 0 && K >= 256 && !heavy_epilogue && igemm8_legal(a, nclass, 256)) {
    const long tiles = ((M + 223) / 224) * nclass * (a.Ncols / 256);
    const int cus = device_cus();  // thresholds measured on 256 CUs, kept as fractions of the chip (0.7 of a round; two rounds)
    if (tiles * 10 >= 7L * cus && !(nclass > 1 && tiles > 2L * cus && mt > 1)) {
      p->bm = 224; p->bn = 256; p->korder = ko; p->fat = 0;
      return true;
    }
  }
  if (a.Ncols % 128 == 0 && K >= 4096 && igemm8_legal(a, nclass, 128)) {
    const long tiles = ((M + 255) / 256) * nclass * (a.Ncols / 128);
    if (tiles * 10 >= 7L * device_cus() && tiles <= device_cus()) {
      p->bm = 256; p->bn = 128; p->korder = ko; p->fat = 1;
      return true;
    }
  }
  return false;
}

// The generated kernel of a bf16 launch, if one serves it — the head of the order below, and all the igemm_*_legal questions need.
// (A forced implicit-GEMM tile, MI355_IGEMM8 / MI355_IGEMM_BIG, disables every generated family: gen_kernels.cpp dconv_enabled().)
bool select_generated(const IgemmArgs& a, int nclass, ConvPick* p) {
  return dconv_pick(a, nclass, 0, p) || po_pick(a, nclass, p) || pw_pick(a, nclass, p) || pk_pick(a, nclass, p);
}

// THE ORDER for a bf16 launch: dconv, po, pw, pk, stem-direct, the 8-wave kernel, 256 x 256, 256 x 128, then 128 x 128 / 128 x 64.
// (launch_igemm refuses a half-resolution addend that got past po.)
ConvPick select_bf16(const IgemmArgs& a, int nclass, bool wide) {
  ConvPick p;
  if (select_generated(a, nclass, &p)) return p;
  // the stem as a direct convolution out of raw input rows (stem_direct.hip; MI355_STEM_DIRECT=0: the row-pair implicit GEMM)
  if (knobs().stem_direct && stem_direct_legal(a, nclass)) {
    p.family = CONV_STEM;
    return p;
  }
  if (choose_igemm8(a, nclass, &p)) {
    p.family = CONV_IGEMM8;
    return p;
  }
  // 256 x 256 tiles (bf16 only: fp32 MFMAs are slow enough that the LDS port is not the limit).  Measured per layer
  // shape at batch 256 (tools/one_conv.py): they win when the 256 single-workgroup CUs are still mostly filled
  // (>= 192 tiles) and the reduction is long enough to amortise the larger epilogue (K >= 256); they lose on the
  // HBM-bound layer-1/2 shapes and when layer 4's 98 row tiles leave most CUs idle.
  const int big_mode = knobs().has_igemm_big ? knobs().igemm_big : -1;  // MI355_IGEMM_BIG: 0 never / 1 wherever N % 256 == 0 (tests, A/B); unset: the rule
  const long items256 = (long)cdiv(a.N * a.Hsub * a.Wsub, 256) * nclass * (a.Ncols / 256);
  const int mt = max_taps(a, nclass);
  // (not with the BN-backward sums: that epilogue needs more registers than the 256 x 256 tile leaves)
  const int cus = device_cus();
  const bool big = a.Ncols % 256 == 0 && (big_mode < 0 ? (items256 * 4 >= 3L * cus && mt * a.Ck >= 256 && !a.bn_y) : big_mode == 1);
  // 256 x 128, 8 waves, 3-stage ring: per CU and k-step 8 % faster than two 128 x 128 workgroups (the slab wait drops
  // from ~700 to ~200 cycles), but a partial round costs it a full one where the 2-workgroup form speeds up when a CU
  // holds a single workgroup — so only where all its tiles fit into one round, and the reduction is long
  const long items3 = (long)cdiv(a.N * a.Hsub * a.Wsub, 256) * nclass * (a.Ncols / 128);
  const bool tall = a.Ncols % 128 == 0 &&
                    (big_mode < 0 ? ((items3 <= cus && items3 * 2 >= cus && mt * a.Ck >= 512) || (items3 <= 2L * cus && mt == 1 && a.Ck >= 1024)) : big_mode == 3);
  p.bm = big || tall ? 256 : 128;
  p.bn = big ? 256 : (tall || wide ? 128 : 64);  // 256 x 256, 256 x 128, 128 x 128, 128 x 64
  return p;
}

// the three questions, asked of a pick (a ConvPick that no search filled is a CONV_TILE one): no other kernel than these families' has
// the epilogue / operand path in question
bool leaky_sums_args(int dtype, const IgemmArgs& a) { return dtype == MI355_BF16 && a.bn_y && a.stat_partial && a.bn_slope == 0.01f && !knobs().error[0]; }
bool takes_leaky_sums(const ConvPick& p) { return p.family == CONV_DCONV || p.family == CONV_PO || p.family == CONV_PK; }
bool takes_bn_in(const ConvPick& p) { return p.family == CONV_DCONV || p.family == CONV_PO; }  // conv2 <- bn1, conv3 <- bn2
bool takes_sub2(const ConvPick& p) { return p.family == CONV_PO; }

}  // namespace

bool igemm_leaky_sums_legal(int dtype, const IgemmArgs& a, int nclass) {
  ConvPick p;
  return leaky_sums_args(dtype, a) && select_generated(a, nclass, &p) && takes_leaky_sums(p);
}

bool igemm_sub2_legal(int dtype, const IgemmArgs& a, int nclass) {
  ConvPick p;
  return dtype == MI355_BF16 && a.addend_sub2 && select_generated(a, nclass, &p) && takes_sub2(p);
}

bool igemm_bn_in_legal(int dtype, const IgemmArgs& a, int nclass) {
  ConvPick p;
  return dtype == MI355_BF16 && a.bn_in != nullptr && select_generated(a, nclass, &p) && takes_bn_in(p);
}

int launch_igemm(int dtype, const IgemmArgs& a, int nclass, hipStream_t stream, int* stat_rows) {
  const int bk = BKB / (int)dtype_size(dtype);
  MI355_ARG(a.in && a.wt && a.out, "igemm: null pointer");
  MI355_ARG(a.Ck % bk == 0, "igemm: Ck=%d not a multiple of %d", a.Ck, bk);
  MI355_ARG(a.Ncols % 64 == 0, "igemm: Ncols=%d not a multiple of 64", a.Ncols);
  MI355_ARG(nclass >= 1 && nclass <= 4, "igemm: nclass=%d", nclass);
  MI355_ARG(((size_t)a.pix_stride * dtype_size(dtype)) % 8 == 0, "igemm: pixel stride not 8-byte aligned");
  MI355_ARG(a.N > 0 && a.Hsub > 0 && a.Wsub > 0, "igemm: empty problem");
  MI355_ARG(!knobs().error[0], "%s", knobs().error);
  // BN = 128 unless that leaves most of the 256 CUs without a tile (the FC layer: 256 rows): then 64-wide tiles double
  // the workgroups
  const long tiles128 = (long)cdiv(a.N * a.Hsub * a.Wsub, 128) * nclass * (a.Ncols / 128);
  const bool wide = (a.Ncols % 128 == 0) && tiles128 * 2 >= device_cus();
  MI355_ARG(dtype == MI355_BF16 || !a.addend_sub2, "igemm: a half-resolution addend needs the generated pointwise kernel (igemm_sub2_legal)");
  ConvPick p;  // fp32: the 128-row tiles
  p.bm = 128;
  p.bn = wide ? 128 : 64;
  if (dtype == MI355_BF16) p = select_bf16(a, nclass, wide);
  MI355_ARG(a.bn_slope == 0.f || (leaky_sums_args(dtype, a) && takes_leaky_sums(p)), "igemm: BN-backward sums under a leaky mask need a generated kernel with that epilogue and slope 0.01 (igemm_leaky_sums_legal)");
  MI355_ARG(a.bn_in == nullptr || takes_bn_in(p), "igemm: the input's BatchNorm in the operand path needs a generated kernel with that form (igemm_bn_in_legal)");
  if (dtype != MI355_F32 && dtype != MI355_BF16) {
    set_error("igemm: bad dtype %d", dtype);
    return MI355_E_ARG;
  }
  MI355_ARG(!a.addend_sub2 || p.family == CONV_DCONV || p.family == CONV_PO, "igemm: a half-resolution addend needs the generated pointwise kernel (igemm_sub2_legal)");
  switch (p.family) {
    case CONV_STEM: return launch_stem_direct(a, stream, stat_rows);
    case CONV_IGEMM8: return launch_igemm8(a, nclass, p.bm, p.bn, p.korder, p.fat, stream, stat_rows);
    case CONV_TILE: return launch_igemm_tile(dtype, a, nclass, p.bm, p.bn, stream, stat_rows);
    default: return launch_gen(p, a, nclass, 1.f, stream, stat_rows);
  }
}

// ---- e4m3 operands (fp8.hip holds the quantiser and the C entry points) ------------------------------------------------------------------
bool igemm_fp8_legal(const IgemmArgs& a, int nclass) { return igemm8_fp8_legal(a, nclass, 128); }

int launch_igemm_fp8(const IgemmArgs& a, int nclass, float oscale, hipStream_t stream, int* stat_rows) {
  // the stride-1 3x3 launches of layers 2 - 4: the generated direct kernel on the K = 128 MFMA (asm/dconv_gen.py Cfg.fp8)
  ConvPick p;
  if (dconv_pick(a, nclass, 1, &p)) return launch_gen(p, a, nclass, oscale, stream, stat_rows);
  // the wide tile when it alone fills most of the 256 CUs (same threshold as the bf16 rule, choose_igemm8)
  const long long M = (long long)a.N * a.Hsub * a.Wsub;
  const bool wide8 = a.Ncols % 256 == 0 && ((M + 223) / 224) * nclass * (a.Ncols / 256) * 10 >= 7LL * device_cus();
  MI355_ARG(wide8 || a.Ncols % 128 == 0, "conv fp8: %d output columns (a multiple of 128 is needed)", a.Ncols);
  const int bm = wide8 ? 224 : 256, bn = wide8 ? 256 : 128;
  return launch_igemm8_fp8(a, nclass, bm, bn, max_taps(a, nclass) > 1 ? 1 : 0, oscale, stream, stat_rows);
}

}  // namespace mi355
