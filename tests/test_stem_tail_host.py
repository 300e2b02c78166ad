"""The reference of tests/stem_tail_common.py pinned on the CPU, and its comparisons shown to bite.

  * ref_fwd against torch's own max_pool2d(return_indices=True) on the rounded activation, on data where most windows hold their maximum more than once;
  * ref_bwd, on ref_fwd's own codes and bits, against fp64 autograd through BatchNorm (batch statistics, handed to ref_bwd as the given mean / invstd),
    ReLU and the max pool, and against oracle/resnet50_bwd_ref.py's maxpool_bwd + bn_bwd;
  * pool_scatter against the kernels' formulation (csrc/bn.hip PoolGather: a 2 x 2 block of pixels gathers from its four windows), on free codes;
  * three planted errors — the last maximum instead of the first, an edge window not voided, ReLU bits taken from the neighbouring pixel — each fed to
    the comparison functions tests/test_stem_tail_gpu.py asserts through, which must refuse them and must pass the reference's own output."""
import pytest
import torch
import torch.nn.functional as F

import stem_tail_common as S
from oracle import resnet50_bwd_ref as O

C = S.C
CASES = [(s, d) for d in S.DTYPES for s in S.SHAPES]
IDS = [f"{'x'.join(map(str, s))}-{'f32' if d == torch.float32 else 'bf16'}" for s, d in CASES]


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def torch_codes(stored):
    """torch's max pool on NHWC `stored`: (maximum, window code of the index torch returns)"""
    N, H, W, _ = stored.shape
    v, flat = F.max_pool2d(_nchw(stored), 3, 2, 1, return_indices=True)
    oh = torch.arange(H // 2).view(1, 1, -1, 1)
    ow = torch.arange(W // 2).view(1, 1, 1, -1)
    kh, kw = flat // W - (2 * oh - 1), flat % W - (2 * ow - 1)
    assert ((kh >= 0) & (kh <= 2) & (kw >= 0) & (kw <= 2)).all()
    return _nhwc(v), _nhwc(kh * 3 + kw).to(torch.uint8)


def as_kernel_fwd(f, dtype):
    """a reference forward in the kernels' output types"""
    return f.p.to(dtype), f.idx, S.pack_bits(f.bits, dtype)


def as_kernel_bwd(b, dtype):
    return b.dx.to(dtype), b.dgamma.float(), b.dbeta.float()


# ---- the reference itself -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_ref_fwd_is_torch_max_pool_on_the_rounded_activation(shape, dtype):
    y, scale, shift = S.exact_fwd_data(shape, dtype)
    f = S.exact_fwd_ref(shape, dtype)
    a0 = torch.relu(y.double() * scale.double() + shift.double()).to(dtype)  # exact on these grids
    assert torch.equal(a0.double(), f.stored)
    v, code = torch_codes(a0.double())
    assert torch.equal(v, f.p) and torch.equal(code, f.idx)
    assert torch.equal(f.bits, a0 > 0)
    # the data discriminate: every code occurs, more than one window in ten holds its maximum twice or more, clipped windows and signed zeros exist
    assert sorted(set(f.idx.flatten().tolist())) == list(range(9))
    ties = sum((S.tap_values(f.stored, torch.full_like(f.idx, k), float("-inf")) == f.p).to(torch.int64) for k in range(9))
    assert (ties >= 2).double().mean() > 0.1
    zeros = (f.p == 0).double().mean().item()
    assert 0.05 < zeros < 0.25, zeros
    assert ((f.a == 0) & ~torch.signbit(f.a)).any()
    if f.a.numel() >= 2 * 8 * 12 * C:  # (-0 needs a zero of y under a -0 shift: the smaller shapes have too few)
        assert ((f.a == 0) & torch.signbit(f.a)).any()


def test_ref_fwd_on_continuous_data_and_the_seed_of_the_random_tier():
    for shape, dtype in CASES:
        y, scale, shift = S.random_fwd_data(shape, dtype)
        f = S.random_fwd_ref(shape, dtype)
        v, code = torch_codes(f.stored)
        assert torch.equal(v, f.p) and torch.equal(code, f.idx)
        assert (scale < 0).any() and (scale > 0).any()
        share = S.bits_excluded(f).double().mean().item()
        assert share <= S.BITS_EXCLUDED_MAX, (shape, dtype, share)
        assert f.a.abs().min() > 2.0 ** -100  # nowhere near the subnormal range


def test_bits_round_trip_through_the_kernels_bytes():
    for dtype in S.DTYPES:
        bits = torch.rand((2, 4, 6, C), generator=torch.Generator().manual_seed(3)) < 0.5
        packed = S.pack_bits(bits, dtype)
        assert packed.shape == (2, 4, 6, C // S.vec(dtype)) and packed.dtype == torch.uint8
        assert torch.equal(S.unpack_bits(packed, dtype), bits)
        one = torch.zeros((1, 2, 2, C), dtype=torch.bool)
        one[0, 1, 0, S.vec(dtype) + 2] = True  # channel V + 2: byte 1, bit 2
        assert S.pack_bits(one, dtype)[0, 1, 0].tolist() == [0, 4] + [0] * (C // S.vec(dtype) - 2)


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ref_bwd_is_autograd_through_bn_relu_pool(shape):
    """fp64 autograd; the activation is rounded to fp32 straight-through so that the pool sees the reference's own values (and ties); dp is dyadic, so the
    reference's rounding of the pool gradient is exact"""
    dtype = torch.float32
    N, H, W = shape
    y = S.random_fwd_data(shape, dtype)[0].double().requires_grad_(True)
    gamma, beta = S.random_bwd_data(shape, dtype)[1].double().requires_grad_(True), S.random_fwd_data(shape, dtype)[2].double().requires_grad_(True)
    dp = S.exact_bwd_data(shape, dtype)[0]
    y2 = y.reshape(-1, C)
    mean, invstd = y2.mean(0), (y2.var(0, unbiased=False) + O.EPS).rsqrt()
    scale = gamma * invstd
    shift = beta - mean * scale
    a = y * scale + shift
    a = a + (a.float().double() - a).detach()
    out = _nhwc(F.max_pool2d(_nchw(torch.relu(a)), 3, 2, 1))
    out.backward(dp.double())
    f = S.ref_fwd(y.detach(), scale.detach(), shift.detach(), dtype)
    assert torch.equal(f.p, out.detach())
    b = S.ref_bwd(dp, f.idx, f.bits, y.detach(), gamma.detach(), mean.detach(), invstd.detach(), dtype)
    for got, ref in ((b.dx, y.grad), (b.dgamma, gamma.grad), (b.dbeta, beta.grad)):
        assert (got - ref).abs().max() <= 1e-11 * ref.abs().max(), (got - ref).abs().max() / ref.abs().max()


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_ref_bwd_is_the_oracles_stem_backward(shape, dtype):
    y = S.exact_fwd_data(shape, dtype)[0].double()
    f = S.exact_fwd_ref(shape, dtype)
    dp, gamma = S.exact_bwd_data(shape, dtype)[:2]
    g = O.relu_mask(O.maxpool_bwd(f.stored, dp.double()), f.stored)
    dy, dg, db = O.bn_bwd(y, gamma.double(), g)
    mean, invstd, _ = O.bn_stats(y.reshape(-1, C))
    b = S.ref_bwd(dp, f.idx, f.bits, y, gamma, mean, invstd, dtype)
    assert torch.equal(b.g, g)
    for got, ref in ((b.dx, dy), (b.dgamma, dg), (b.dbeta, db)):
        assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
    assert torch.equal(b.abs_g, g.abs().sum((0, 1, 2)))


def gather(dp, idx, shape, void=True):
    """The kernels' form of the pool backward: block t = (n, a, b) of 2 x 2 pixels reads the windows t, t + 1, t + Wo, t + Wo + 1 of the FLATTENED pooled
    tensors (off the right edge that is the next row, off the bottom the next image, behind the tensor zeros), voids the codes of a window off the edge,
    and pixel (r, c) adds the windows (dr <= r, dc <= c) whose code is its position in them."""
    N, H, W, Cc = shape
    Ho, Wo = H // 2, W // 2
    T = N * Ho * Wo
    d = torch.cat([dp.float().reshape(T, Cc), torch.zeros(Wo + 1, Cc)])
    i = torch.cat([idx.reshape(T, Cc), torch.zeros(Wo + 1, Cc, dtype=torch.uint8)])
    a = torch.arange(Ho).view(1, Ho, 1, 1)
    b = torch.arange(Wo).view(1, 1, Wo, 1)
    g = torch.zeros(shape, dtype=torch.float32)
    for r in range(2):
        for c in range(2):
            acc = torch.zeros((N, Ho, Wo, Cc), dtype=torch.float32)
            for dr in range(r + 1):
                for dc in range(c + 1):
                    off = dr * Wo + dc
                    dw, iw = d[off:off + T].view(N, Ho, Wo, Cc), i[off:off + T].view(N, Ho, Wo, Cc)
                    ok = (a + dr < Ho) & (b + dc < Wo) if void else torch.tensor(True)
                    pos = (r + 1 - 2 * dr) * 3 + (c + 1 - 2 * dc)
                    acc = acc + torch.where((iw == pos) & ok, dw, torch.zeros_like(dw))
            g[:, r::2, c::2] = acc
    return g


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_scatter_is_the_kernels_gather(shape):
    N, H, W = shape
    dp = S.random_bwd_data(shape, torch.float32)[0]
    for idx in (S.free_codes(shape)[0], S.exact_fwd_ref(shape, torch.float32).idx):
        assert torch.equal(S.pool_scatter(dp, idx, (N, H, W, C)), gather(dp, idx, (N, H, W, C)))
    # with the forward's own codes a window off the edge never names a pixel (its row -1 / column -1 taps lie outside the image): only free codes
    # show a window that is not voided
    idx = S.exact_fwd_ref(shape, torch.float32).idx
    assert torch.equal(gather(dp, idx, (N, H, W, C), void=False), gather(dp, idx, (N, H, W, C)))


# ---- the comparisons ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_the_references_own_output_passes_every_comparison(shape, dtype):
    f = S.exact_fwd_ref(shape, dtype)
    S.check_fwd_exact(*as_kernel_fwd(f, dtype), f, dtype)
    b = S.exact_bwd_ref(shape, dtype)
    assert S.sums_are_exact(b)
    S.check_sums_exact(*as_kernel_bwd(b, dtype)[1:], b)
    S.check_dx(b.dx.to(dtype), b, dtype)
    f = S.random_fwd_ref(shape, dtype)
    assert S.check_fwd_random(*as_kernel_fwd(f, dtype), f, dtype)["excluded"] <= S.BITS_EXCLUDED_MAX
    y = S.random_fwd_data(shape, dtype)[0]
    dp, gamma, mean, invstd = S.random_bwd_data(shape, dtype)
    b = S.ref_bwd(dp, f.idx, f.bits, y, gamma, mean, invstd, dtype)
    dx, dg, db = as_kernel_bwd(b, dtype)
    S.check_sums_random(dg, db, b)
    S.check_dx(dx, b, dtype)


def last_maximum_codes(stored):
    """the planted tie rule: `>=` in the scan, so the LAST maximum wins"""
    N, H, W, Cc = stored.shape
    xp = S._padded(stored, float("-inf"))
    best = torch.full((N, H // 2, W // 2, Cc), float("-inf"), dtype=torch.float64)
    code = torch.full(best.shape, 255, dtype=torch.uint8)
    for k in range(9):
        t = S._tap(xp, k, H, W)
        better = (t >= best) & (t > float("-inf"))
        best = torch.where(better, t, best)
        code = torch.where(better, torch.full_like(code, k), code)
    return code


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_planted_last_maximum_tie_rule_is_caught(shape, dtype):
    f = S.exact_fwd_ref(shape, dtype)
    wrong = last_maximum_codes(f.stored)
    assert torch.equal(S.tap_values(f.stored, wrong), f.p)  # still a maximum of every window: only the tie rule differs
    p, _, bits = as_kernel_fwd(f, dtype)
    with pytest.raises(AssertionError, match="codes differ"):
        S.check_fwd_exact(p, wrong, bits, f, dtype)
    # and a backward that routes by that rule, against the reference on the forward's codes: tied taps hold the same activation, hence the same y and
    # x_hat, so the sums cannot see where the gradient went — the per-pixel dx does
    y = S.exact_fwd_data(shape, dtype)[0]
    dp, gamma, mean, invstd = S.exact_bwd_data(shape, dtype)
    b = S.exact_bwd_ref(shape, dtype)
    planted = S.ref_bwd(dp, wrong, f.bits, y, gamma, mean, invstd, dtype)
    with pytest.raises(AssertionError, match="dx"):
        S.check_dx(planted.dx.to(dtype), b, dtype)


def bwd_from_g(g32, bits, y, gamma, mean, invstd, dtype):
    """the rest of the backward behind a planted pool gradient (fp32, before rounding and masking), in the kernels' output types"""
    v = lambda t: t.double().view(1, 1, 1, -1)  # noqa: E731
    M = y.shape[0] * y.shape[1] * y.shape[2]
    g = torch.where(bits, g32.to(dtype).double(), torch.zeros((), dtype=torch.float64))
    xhat = (y.double() - v(mean)) * v(invstd)
    dbeta, dgamma = g.sum((0, 1, 2)), (g * xhat).sum((0, 1, 2))
    dx = v(gamma) * v(invstd) * (g - v(dbeta) / M - xhat * v(dgamma) / M)
    return dx.to(dtype), dgamma.float(), dbeta.float()


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_planted_unvoided_edge_window_is_caught(shape, dtype):
    """free codes, as the GPU test's `free` arm draws them: a window read off the right or the bottom edge then names pixels of this block"""
    N, H, W = shape
    idx, bits = S.free_codes(shape)
    # exact tier
    y = S.exact_fwd_data(shape, dtype)[0]
    dp, gamma, mean, invstd = S.exact_bwd_data(shape, dtype)
    b = S.ref_bwd(dp, idx, bits, y, gamma, mean, invstd, dtype)
    assert S.sums_are_exact(b)
    good = bwd_from_g(gather(dp, idx, (N, H, W, C)), bits, y, gamma, mean, invstd, dtype)
    S.check_sums_exact(good[1], good[2], b)
    S.check_dx(good[0], b, dtype)
    dx, dg, db = bwd_from_g(gather(dp, idx, (N, H, W, C), void=False), bits, y, gamma, mean, invstd, dtype)
    with pytest.raises(AssertionError, match="differs"):
        S.check_sums_exact(dg, db, b)
    with pytest.raises(AssertionError, match="dx"):
        S.check_dx(dx, b, dtype)
    # random tier
    y = S.random_fwd_data(shape, dtype)[0]
    dp, gamma, mean, invstd = S.random_bwd_data(shape, dtype)
    b = S.ref_bwd(dp, idx, bits, y, gamma, mean, invstd, dtype)
    dx, dg, db = bwd_from_g(gather(dp, idx, (N, H, W, C), void=False), bits, y, gamma, mean, invstd, dtype)
    with pytest.raises(AssertionError, match="dx"):
        S.check_dx(dx, b, dtype)
    if shape != (5, 16, 24):  # (a few stray border pixels among 1920 per channel can stay inside 1e-5 of sum |terms|: there dx is what catches it)
        with pytest.raises(AssertionError, match="off by"):
            S.check_sums_random(dg, db, b)


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_planted_bits_of_the_neighbouring_pixel_are_caught(shape, dtype):
    for tier, fwd_ref, fwd_data, bwd_data in (("exact", S.exact_fwd_ref, S.exact_fwd_data, S.exact_bwd_data),
                                              ("random", S.random_fwd_ref, S.random_fwd_data, S.random_bwd_data)):
        f = fwd_ref(shape, dtype)
        p, idx, _ = as_kernel_fwd(f, dtype)
        wrong = torch.roll(f.bits, 1, dims=2)  # the bit of pixel (h, w - 1)
        with pytest.raises(AssertionError, match="bit"):
            (S.check_fwd_exact if tier == "exact" else S.check_fwd_random)(p, idx, S.pack_bits(wrong, dtype), f, dtype)
        y = fwd_data(shape, dtype)[0]
        dp, gamma, mean, invstd = bwd_data(shape, dtype)
        b = S.ref_bwd(dp, f.idx, f.bits, y, gamma, mean, invstd, dtype)
        planted = S.ref_bwd(dp, f.idx, wrong, y, gamma, mean, invstd, dtype)
        dx, dg, db = as_kernel_bwd(planted, dtype)
        with pytest.raises(AssertionError):
            S.check_sums_exact(dg, db, b) if tier == "exact" else S.check_sums_random(dg, db, b)
        with pytest.raises(AssertionError, match="dx"):
            S.check_dx(dx, b, dtype)
