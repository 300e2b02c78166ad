// conv_kernels.h — what the conv source files call in one another: every kernel family's legality test and launcher, and the value
// conv_select.cpp passes from its one search per launch to the launch.  (What the executors call — launch_igemm, launch_igemm_fp8,
// the igemm_*_legal questions, plan_wgrad / launch_wgrad — is in common.h.)
#pragma once
#include "common.h"

namespace mi355 {

// the kernel family a conv launch goes to, in the order conv_select.cpp tries them
enum ConvFamily {
  CONV_DCONV,   // generated direct 3x3 kernels (asm/dconv_gen.py): stride 1, and the stride-2 data gradient by output-parity classes
  CONV_PO,      // generated output-heavy pointwise kernels with resident weights (asm/po_gen.py): K <= 512 -> 4K columns, shortcut addend, BN-backward sums
  CONV_PW,      // generated persistent pointwise kernels (asm/pw_gen.py): output-heavy 1x1 forward
  CONV_PK,      // generated long-reduction pointwise kernels (asm/pk_gen.py): K = 1024 / 2048 -> 256-column tiles
  CONV_STEM,    // stem_direct.hip: the stem as a direct convolution
  CONV_IGEMM8,  // conv_igemm8.hip: the 8-wave ping-pong kernel
  CONV_TILE,    // conv_igemm.hip: the 4-wave / 256 x 128 implicit-GEMM tiles
};

struct PoPlan {  // launch plan of a po kernel (gen_kernels.cpp plan_po)
  unsigned T = 0, nct = 0, tpg = 0, G = 0, grid = 0, lognct = 0;
};
// the decision for one launch: found once (conv_select.cpp), launched once
struct ConvPick {
  ConvFamily family = CONV_TILE;
  int vi = -1;                 // generated families: index into the family's variant table ...
  hipFunction_t fn = nullptr;  // ... its function on the current device ...
  PoPlan po;                   // ... and, for po, its plan
  int bm = 0, bn = 0, korder = 0, fat = 0;  // CONV_IGEMM8 / CONV_TILE: the tile; igemm8 only: k order and the fat-phase form
};

// ---- gen_kernels.cpp: *_pick is true, with `p` filled, when the family serves this launch on the current device under the knobs
// (MI355_DCONV, MI355_PO, ...) and its measured per-shape rule; p is untouched otherwise.  dconv fp8 = 1: e4m3 operands.
bool dconv_pick(const IgemmArgs& a, int nclass, int fp8, ConvPick* p);
bool po_pick(const IgemmArgs& a, int nclass, ConvPick* p);
bool pw_pick(const IgemmArgs& a, int nclass, ConvPick* p);
bool pk_pick(const IgemmArgs& a, int nclass, ConvPick* p);
// launches what a *_pick found for the same (a, nclass); oscale: e4m3 dconv only
int launch_gen(const ConvPick& p, const IgemmArgs& a, int nclass, float oscale, hipStream_t stream, int* stat_rows);
int wg3_plan(int dtype, const WgradArgs& a);  // split count of the generated weight-gradient kernels (wg, wg1); 0: the launch is not served by one
int launch_wg3(const WgradArgs& a, int splits, hipStream_t stream);
// ---- stem_direct.hip
bool stem_direct_legal(const IgemmArgs& a, int nclass);
int launch_stem_direct(const IgemmArgs& a, hipStream_t stream, int* stat_rows);
// ---- conv_igemm8.hip: bf16 and e4m3 entry points
bool igemm8_legal(const IgemmArgs& a, int nclass, int bn);
int launch_igemm8(const IgemmArgs& a, int nclass, int bm, int bn, int korder, int fat, hipStream_t stream, int* stat_rows);
bool igemm8_fp8_legal(const IgemmArgs& a, int nclass, int bn);
int launch_igemm8_fp8(const IgemmArgs& a, int nclass, int bm, int bn, int korder, float oscale, hipStream_t stream, int* stat_rows);
// ---- conv_igemm.hip: the instantiated tiles — fp32 128 x 128 | 128 x 64; bf16 those, 256 x 256 and 256 x 128 (8 waves, 3-stage ring)
int launch_igemm_tile(int dtype, const IgemmArgs& a, int nclass, int bm, int bn, hipStream_t stream, int* stat_rows);
// ---- host helpers of the launchers
void lds_opt_in(const void* fn, size_t lds);  // conv_api.cpp: > 64 KiB of dynamic LDS needs an opt-in per kernel symbol (once)
// q / d = mulhi(q, magic32(d)) while q * d < 2^32
static inline unsigned magic32(unsigned d) { return (unsigned)((1ull << 32) / d + 1); }

}  // namespace mi355
