"""The BatchNorm kernels of csrc/bn.hip, per op, on the GPU: the forms the executors launch (mi355_bn_apply, mi355_bn_bwd_bits: bit masks, the second
normalised branch, the masked write-back, in-place operation, partial rows in place of the reduce pass), every reduce layout at ragged M, every
finalize form from synthetic partial rows, |mean| >> std through the pivot, constant channels and M = 1, and the inference form.

The assertions are the verify_* functions of tests/bn_common.py — fp64 references, exact data that must come back bit for bit, random data under bounds
derived there — the same that tests/test_bn_host.py runs over an fp32 restatement of the kernels, with errors planted to show that they can fail."""
import pytest
import torch

import bn_common as B

pytestmark = pytest.mark.gpu
ids = lambda c: "-".join(str(v).replace("torch.", "") for v in (c if isinstance(c, tuple) else (c,)))  # noqa: E731


class GpuBackend:
    """the three operations through ops.py; host tensors in, host tensors out"""

    def __init__(self, dev):
        self.dev = dev
        self.last = None

    def up(self, t):
        return None if t is None else t.to(self.dev).contiguous()

    def fwd_train(self, d, momentum, partial=None, relu=1):
        from sota_imagenet_amd import ops

        rm, rv = self.up(d.rm.clone()), self.up(d.rv.clone())
        out, sm, si = ops.bn_fwd_train(self.up(d.x), self.up(d.gamma), self.up(d.beta), rm, rv, None, relu, momentum=momentum, stats=self.up(partial))
        return tuple(t.cpu() for t in (out, sm, si, rm, rv))

    def apply(self, x, scale, shift, relu, want_bits, **addend):
        from sota_imagenet_amd import ops

        out, bits = ops.bn_apply(self.up(x), self.up(scale), self.up(shift), relu=relu, want_bits=want_bits, **{k: self.up(v) for k, v in addend.items()})
        return out.cpu(), None if bits is None else bits.cpu()

    def bwd(self, d, relu, dz_out=False, beta_acc=0.0, alias="none", partial=None):
        from sota_imagenet_amd import ops

        g = self.up(d.g.clone())
        dz = None if not dz_out else g if alias == "dz" else torch.empty_like(g)
        dx = g if alias == "dx" else None
        bits = self.up(B.pack(d.bits, d.x.dtype)) if relu else None
        dx, dg, db = ops.bn_bwd_bits(g, bits, self.up(d.x), self.up(d.gamma), self.up(d.mean), self.up(d.invstd), relu=relu, dx=dx, dz_out=dz,
                                     dgamma=self.up(d.dgamma0.clone()), dbeta=self.up(d.dbeta0.clone()), beta_acc=beta_acc, partial=self.up(partial))
        self.last = (dx.cpu(), None if dz is None else dz.cpu(), dg.cpu(), db.cpu())
        return self.last


@pytest.fixture(scope="module")
def be(dev):
    return GpuBackend(dev)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    i = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(i), b.contiguous().view(i))


@pytest.mark.parametrize("case", B.REDUCE_CASES, ids=ids)
def test_reduce_layouts_and_ragged_rows(be, case):
    """forward statistics and the bit-mask backward through every (threads per row, row lanes, channel workgroups) layout of both dtypes, at M = 1, 2, 5,
    one short of and one past a workgroup's first round, and 777"""
    dt, C, M = case
    for tier in ("exact", "random"):
        B.verify_stats(be, dt, C, M, tier)
        B.verify_bwd(be, dt, C, M, tier, 1)


@pytest.mark.parametrize("case", B.THRESHOLD_CASES, ids=ids)
def test_row_count_thresholds_through_the_real_reduce(be, case):
    """127 / 128 partial rows (the finalize form flips), 128 rows at 64 channels, and the 512-row cap, where a thread walks a ninth row"""
    dt, C, M = case
    for tier in ("exact", "random"):
        B.verify_stats(be, dt, C, M, tier, momentum=0.25)
        B.verify_bwd(be, dt, C, M, tier, 1)


@pytest.mark.parametrize("case", B.SYNTH_CASES, ids=ids)
def test_finalize_forms_from_synthetic_rows(be, case):
    """every finalize form, forward (mi355_bn_fwd_train_partial) and backward (the partial argument of mi355_bn_bwd_bits), one pass of its slices and
    more: the rows are an uneven exact partition of the true sums with empty rows, so the result cannot depend on the form and must be bit-equal"""
    C, nblk = case
    for dt in B.DTYPES:
        B.verify_stats(be, dt, C, B.SYNTH_M, "exact", partial_nblk=nblk)
        fig = B.verify_bwd(be, dt, C, B.SYNTH_M, "exact", 1, partial_nblk=nblk)
        assert fig.get("dx_exact")


def test_offset_data(be):
    """|mean| >> std: the pivot path under the bound with the factor ((pivot - mean)^2 + var) / var, the plain-sum rows under theirs with (mean^2 + var) /
    var; the measured loss of the latter is printed beside the CPU's record of it"""
    for name in B.OFFSET_CASES:
        piv, plain = B.verify_offset(be, name, "pivot"), B.verify_offset(be, name, "plain")
        print(f"{name}: relative error of invstd, pivot path {piv:.3g}, plain-sum rows {plain:.3g} (restatement: {B.PLAIN_SUM_LOSS_MEASURED[name]:.3g})")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
def test_constant_channel_and_single_row(be, dtype):
    for M in (1, B.CONST_M):
        for momentum in (0.1, 0.25):
            B.verify_constant(be, dtype, M, momentum)


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
@pytest.mark.parametrize("shape", B.APPLY_SHAPES, ids=ids)
def test_apply_forms(be, dtype, shape):
    """mi355_bn_apply: {none, residual, second branch} x {no activation, ReLU, ReLU + bits, leaky, leaky + bits}, the legal ones; exact data with zeros and
    negative zeros (bit clear, upper nibble of an fp32 byte zero), random data outside the at-zero band"""
    M, C = shape
    for ad, relu, bits in B.APPLY_FORMS:
        for tier in ("exact", "random"):
            B.verify_apply(be, dtype, M, C, tier, ad, relu, bits)


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
def test_bwd_forms_and_aliasing(be, dtype):
    """mi355_bn_bwd_bits: relu {0, 1, 2} x masked write-back x accumulation onto a prefill x aliasing; an aliased run (dx == g, dz_out == g) returns the
    bits of the unaliased one"""
    for tier in ("exact", "random"):
        base = {}
        for relu, dz, acc, alias in B.BWD_FORMS:
            B.verify_bwd(be, dtype, B.BWD_C, B.BWD_M, tier, relu, dz, acc, alias)
            if alias == "none":
                base[relu, dz, acc] = be.last
            else:
                for name, a, b in zip(("dx", "dz", "dgamma", "dbeta"), be.last, base[relu, dz, acc]):
                    assert _same_bits(a, b), f"{tier} relu={relu} dz_out={dz} beta_acc={acc}: {name} of the run aliased on {alias} differs"


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
@pytest.mark.parametrize("relu", [1, 2])
def test_bwd_on_the_bits_apply_returned(be, dev, dtype, relu):
    """teacher-forced on the mask mi355_bn_apply wrote for the same tensor; and mi355_bn_bwd, which takes its mask from the stored activation, returns the
    same bits of dx / dgamma / dbeta as the bit-mask form"""
    from sota_imagenet_amd import ops

    M, C = 777, 256
    a = B.random_apply_data(M, C, dtype)
    out, packed = be.apply(a.x, a.scale, a.shift, relu, True)
    bits = B.unpack(packed, dtype)
    B.verify_bwd(be, dtype, C, M, "random", relu, bits=bits)
    d = B.random_bwd_data(M, C, dtype)
    up = be.up
    for acc in (0.0, 1.0):   # onto a prefill too: overwritten, resp. accumulated, by both alike
        pre = lambda: {"dgamma": up(d.dgamma0.clone()), "dbeta": up(d.dbeta0.clone()), "beta_acc": acc}  # noqa: E731
        dx, dg, db = ops.bn_bwd_bits(up(d.g), up(packed), up(d.x), up(d.gamma), up(d.mean), up(d.invstd), relu=relu, **pre())
        dx1, dg1, db1, _ = ops.bn_bwd(up(d.g), up(out), up(d.x), up(d.gamma), up(d.mean), up(d.invstd), relu, **pre())
        for name, p, q in (("dx", dx, dx1), ("dgamma", dg, dg1), ("dbeta", db, db1)):
            assert _same_bits(p.cpu(), q.cpu()), f"{name} (beta_acc {acc}): the stored-activation form differs from the bit-mask form"


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
def test_bwd_write_back_forces_the_reduce_and_ignores_the_spare_bits(be, dtype):
    """the rows of a fused data-gradient epilogue come without the masked gradient: with dz_out the call must run its own reduce, as bn_backward of the
    executor does, whatever rows it was handed; and an fp32 mask byte's upper four bits are nobody's: set, they change nothing"""
    from sota_imagenet_amd import ops

    M, C = B.BWD_M, B.BWD_C
    d = B.exact_bwd_data(M, C, dtype)
    want = be.bwd(d, 1, dz_out=True)
    junk = torch.full((5, 2, C), 3.0)
    for name, a, b in zip(("dx", "dz", "dgamma", "dbeta"), be.bwd(d, 1, dz_out=True, partial=junk), want):
        assert _same_bits(a, b), f"{name}: rows handed in beside dz_out were used"
    if dtype == torch.float32:
        up = be.up
        packed = B.pack(d.bits, dtype)
        got = [ops.bn_bwd_bits(up(d.g), up(p), up(d.x), up(d.gamma), up(d.mean), up(d.invstd), relu=1) for p in (packed, packed | 0xF0)]
        for name, a, b in zip(("dx", "dgamma", "dbeta"), *got):
            assert _same_bits(a.cpu(), b.cpu()), f"{name}: the upper nibble of an fp32 mask byte was read"


# inference coefficients in fp32: rv + eps (half an ulp, a quarter after the root), sqrtf (1 ulp), the division (2.5 ulp): under 4 ulp = 8 U32 of scale;
# shift = beta - rm * scale: scale's error times |rm|, one rounding of the product, one of the difference
EVAL_SCALE_OPS = 8


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
@pytest.mark.parametrize("shape", [(37, 512), (5, 4096)], ids=ids)
def test_eval_form(dev, dtype, shape):
    """mi355_bn_fwd_eval with a residual, relu 0 / 1 / 2"""
    from sota_imagenet_amd import ops

    M, C = shape
    a, s = B.random_apply_data(M, C, dtype), B.random_stats_data(M, C, dtype)
    eps = float(torch.tensor(B.EPS, dtype=torch.float32))
    scale = s.gamma.double() / torch.sqrt(s.rv.double() + eps)
    shift = s.beta.double() - s.rm.double() * scale
    dsc = EVAL_SCALE_OPS * B.U32 * scale.abs()
    dsh = dsc * s.rm.double().abs() + B.U32 * (s.rm.double() * scale).abs() + B.U32 * shift.abs()
    up = lambda t: t.to(dev)  # noqa: E731
    for relu in (0, 1, 2):
        for res in (None, a.residual):
            ref = B.ref_apply(a.x, scale, shift, residual=res, relu=relu)
            out = ops.bn_fwd_eval(up(a.x), up(s.gamma), up(s.beta), up(s.rm), up(s.rv), None if res is None else up(res), relu)
            B.check_apply_random(out.cpu(), None, ref, dtype, f"eval {dtype} {shape} relu={relu} residual={res is not None}", a.x, dsc, dsh)
