"""The stem tail per op: mi355_bn_relu_maxpool (csrc/misc.hip: one operator in three kernels) and mi355_stem_bwd (csrc/bn.hip: the executor's
backward_stem sequence on the pooled gradient) against the fp64 reference of tests/stem_tail_common.py, whose comparison functions these tests assert
through (tests/test_stem_tail_host.py shows them refusing a wrong tie rule, an edge window that is not voided and misplaced ReLU bits).

What the executor-level tests cannot see and these do: the argmax codes and the ReLU bit bytes themselves; the one-thread-per-window kernel (it runs
only at an odd pooled height or width); the per-pixel gradient dx; border rows and columns, the image boundary behind which the backward's "read
anyway" loads land, ties, and every trip count of the reduce's pipelined loop.

EXACT TIER  dyadic data (stem_tail_common.exact_*_data): a = y * scale + shift is exact in fp32 and in bf16, so p, idx and bits must equal the
  reference bit for bit, under the rule (form 0) and under every legal forced form, and mi355_maxpool_fwd on the reference's stored activation must give
  the same p and idx.  Backward: every term of both sums is a multiple of 1/32 and the reference shows sum |terms| per channel below 2^24 units, so any
  fp32 summation order is exact: dgamma / dbeta equal the fp64 sums exactly, overwritten and accumulated (beta_acc = 1) onto integers — one dropped or
  doubled pixel breaks equality.  Codes and bits: the forward's own, and drawn FREELY (codes 0 .. 8 anywhere, so border windows name taps outside the
  image and every (pixel, window) pair is taken) — with the forward's codes a window off the edge can never name a pixel, so only the free arm
  sees whether it is voided.
RANDOM TIER  continuous data, mixed-sign scales.
  forward value   |p - ref| <= u |ref|, u = 2^-7 (bf16) / 2^-23 (fp32): the kernel's a is ONE fp32 fma, the reference's an fp64 product and sum rounded
                  to fp32 — at most one fp32 ulp apart.  bf16: that can flip one rounding to bf16, and a bf16 ulp is at most 2^-7 of the value.  fp32: a
                  is stored as it is, no further rounding, and an fp32 ulp is at most 2^-23 of the value.
  forward code    names an in-image tap whose reference stored value matches p within the same bound
  forward bits    equal a_ref > 0 except where |a_ref| <= 2^-20 (|y scale| + |shift|); at most 0.1 % of the elements may be excepted — at the seed used the
                  reference excepts none (checked on the CPU by the host file)
  backward sums   |dgamma - ref| <= 1e-5 sum |g xhat|, |dbeta - ref| <= 1e-5 sum |g| per channel: a thread's fp32 chain is at most ~24 adds before the
                  fp64 finalize, worst case ~2e-6 of sum |terms|; the bound is five times that.
                  Largest measured on an MI355X: see test_backward_random.
  backward dx     fp32: normalised max error < 1e-4 (the bar of test_bn_train_fwd_bwd).  bf16: per element |dx - ref| <= 2^-8 |ref| + 1e-4 max |ref| — one
                  RNE rounding (2^-9) with a factor 2, plus the fp32 bar.
NaN inputs and positive fp32 values below 2^-134 are out of scope (the forms differ there by documented design, include/mi355rn.h); the data stay away
from both."""
import pytest
import torch

import stem_tail_common as S

pytestmark = pytest.mark.gpu

C = S.C
CASES = [(s, d) for d in S.DTYPES for s in S.SHAPES]


def _id(shape, dtype):
    return f"{'x'.join(map(str, shape))}-{'f32' if dtype == torch.float32 else 'bf16'}"


IDS = [_id(s, d) for s, d in CASES]
BWD_RANDOM = [(s, d, codes) for s, d in CASES for codes in ("forward", "free")] + [(S.LARGE[d], d, "forward") for d in S.DTYPES]
BWD_EXACT = [(s, d, codes) for s, d in CASES for codes in ("forward", "free")]


def _forward_forms(dev, ops, data, ref, shape, dtype, check):
    """form 0 and every legal forced form through `check`; the forms the shape or dtype does not allow are refused"""
    y, scale, shift = (t.to(dev) for t in data)
    legal = S.legal_forms(shape, dtype)
    out = {}
    for form in [0] + legal:
        p, idx, bits = ops.bn_relu_maxpool(y, scale, shift, form=form)
        torch.cuda.synchronize()
        out[form] = check(p, idx, bits, ref, dtype, what=f"form {form}")
        print(f"{_id(shape, dtype)} form {form}: {out[form]}")
    for form in sorted({1, 2, 3} - set(legal)):
        with pytest.raises(RuntimeError, match="bn_relu_maxpool: form"):
            ops.bn_relu_maxpool(y, scale, shift, form=form)
    for form in (-1, 4):
        with pytest.raises(RuntimeError, match="outside 0..3"):
            ops.bn_relu_maxpool(y, scale, shift, form=form)
    return out


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_forward_exact(dev, shape, dtype):
    from sota_imagenet_amd import ops

    ref = S.exact_fwd_ref(shape, dtype)
    _forward_forms(dev, ops, S.exact_fwd_data(shape, dtype), ref, shape, dtype, S.check_fwd_exact)
    # the stand-alone pool on the activation the unfused path would have stored
    p, idx = ops.maxpool_fwd(ref.stored.to(dtype).to(dev))
    S.check_fwd_exact(p, idx, S.pack_bits(ref.bits, dtype), ref, dtype, what="maxpool_fwd")


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_forward_random(dev, shape, dtype):
    from sota_imagenet_amd import ops

    ref = S.random_fwd_ref(shape, dtype)
    _forward_forms(dev, ops, S.random_fwd_data(shape, dtype), ref, shape, dtype, S.check_fwd_random)


def _bwd_inputs(shape, dtype, codes, tier):
    fwd_ref, fwd_data, bwd_data = ((S.exact_fwd_ref, S.exact_fwd_data, S.exact_bwd_data) if tier == "exact" else
                                   (S.random_fwd_ref, S.random_fwd_data, S.random_bwd_data))
    y = fwd_data(shape, dtype)[0]
    if codes == "forward":
        f = fwd_ref(shape, dtype)
        idx, bits = f.idx, f.bits
    else:
        idx, bits = S.free_codes(shape)
    return (y, idx, bits) + tuple(bwd_data(shape, dtype))


@pytest.mark.parametrize("shape,dtype,codes", BWD_EXACT, ids=[f"{_id(s, d)}-{c}" for s, d, c in BWD_EXACT])
def test_backward_exact(dev, shape, dtype, codes):
    from sota_imagenet_amd import ops

    y, idx, bits, dp, gamma, mean, invstd = _bwd_inputs(shape, dtype, codes, "exact")
    ref = S.exact_bwd_ref(shape, dtype) if codes == "forward" else S.ref_bwd(dp, idx, bits, y, gamma, mean, invstd, dtype)
    assert S.sums_are_exact(ref)
    args = [t.to(dev) for t in (dp, idx, S.pack_bits(bits, dtype), y, gamma, mean, invstd)]
    dx, dg, db = ops.stem_bwd(*args)
    torch.cuda.synchronize()
    S.check_sums_exact(dg, db, ref, what="beta_acc 0")
    print(f"{_id(shape, dtype)}-{codes}: dx {S.check_dx(dx, ref, dtype)}")
    g = torch.Generator().manual_seed(9)
    pre_g = torch.randint(-S.EXACT_PREFILL, S.EXACT_PREFILL + 1, (C,), generator=g).float()
    pre_b = torch.randint(-S.EXACT_PREFILL, S.EXACT_PREFILL + 1, (C,), generator=g).float()
    acc_g, acc_b = pre_g.to(dev), pre_b.to(dev)
    dx2, dg2, db2 = ops.stem_bwd(*args, dgamma=acc_g, dbeta=acc_b, beta_acc=1.0)
    torch.cuda.synchronize()
    assert dg2 is acc_g and db2 is acc_b
    S.check_sums_exact(acc_g, acc_b, ref, pre_g, pre_b, what="beta_acc 1")
    assert torch.equal(dx2, dx)


@pytest.mark.parametrize("shape,dtype,codes", BWD_RANDOM, ids=[f"{_id(s, d)}-{c}" for s, d, c in BWD_RANDOM])
def test_backward_random(dev, shape, dtype, codes):
    """Largest |sum - ref| / sum |terms| measured on an MI355X over all cases: dgamma 1.23e-07 (2x4x6 fp32, the forward's codes), dbeta 7.64e-08
    (3x6x10 fp32); the two large cases 1.9e-09 and 1.2e-09.  The bound is 1e-5."""
    from sota_imagenet_amd import ops

    y, idx, bits, dp, gamma, mean, invstd = _bwd_inputs(shape, dtype, codes, "random")
    ref = S.ref_bwd(dp, idx, bits, y, gamma, mean, invstd, dtype)
    dx, dg, db = ops.stem_bwd(*[t.to(dev) for t in (dp, idx, S.pack_bits(bits, dtype), y, gamma, mean, invstd)])
    torch.cuda.synchronize()
    dg, db, dx = dg.cpu(), db.cpu(), dx.cpu()
    rg, rb = S.sums_ratios(dg, db, ref)
    print(f"{_id(shape, dtype)}-{codes}: dgamma {rg:.3g} of sum |g xhat|, dbeta {rb:.3g} of sum |g|")
    S.check_sums_random(dg, db, ref)
    print(f"{_id(shape, dtype)}-{codes}: dx {S.check_dx(dx, ref, dtype)}")
