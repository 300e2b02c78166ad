"""What tests/test_stem_tail_host.py, tests/test_stem_tail_gpu.py and test_maxpool of tests/test_ops_gpu.py share: a plain fp64 reference of the stem
tail of the ResNet-50 executor — BatchNorm + ReLU + max pool 3x3 / stride 2 / pad 1 fused on the raw conv output (csrc/misc.hip, the three
bn_relu_maxpool kernels behind mi355_bn_relu_maxpool) and its backward from the pooled gradient (csrc/bn.hip, stem_bwd_reduce / stem_bwd_apply behind
mi355_stem_bwd) — the shapes, the data, and the COMPARISONS: the GPU file asserts through the functions below and the host file plants errors
into the reference's own outputs and shows that the same functions catch them.

Tensors are NHWC.  The window scan is nine strided-slice passes over a padded copy (no unfold: the largest case has 21 M elements).
A window code is kh * 3 + kw, the tap (2 oh - 1 + kh, 2 ow - 1 + kw).  The ReLU bits travel as booleans here; pack_bits / unpack_bits convert
to the kernels' bytes ([N][H][W][C / V], V = 16 bytes of elements, bit e of byte v = channel v * V + e)."""
import functools
from typing import NamedTuple

import torch

DTYPES = [torch.float32, torch.bfloat16]
C = 64

# (N, H, W) at full resolution
SHAPES = [
    (1, 4, 4),     # one 2 x 2 pooled block: every window touches a border; most threads of the backward reduce have no block
    (2, 4, 6),     # odd pooled width: the rule picks form 1, forms 2 and 3 are refused
    (3, 6, 10),    # odd pooled height and width
    (2, 8, 12),    # interior blocks, edges and an image boundary (where the "window off the edge is read anyway" loads land)
    (5, 16, 24),   # 480 pooled pixels: threads of the backward reduce get 1 .. 4 blocks — both breaks of the pipelined loop
]
# backward, random tier only: the reduce runs 16 (fp32) / 32 (bf16) block slots per workgroup, four blocks per slot, under a cap of 512 workgroups —
# met at 32 768 resp. 65 536 pooled pixels.  These sizes are just over it (49 152 and 81 920), so a thread takes 6 resp. 5 blocks, and the apply pass
# goes past one grid stride
LARGE = {torch.float32: (3, 256, 256), torch.bfloat16: (5, 256, 256)}

# rel. size of one unit in the last place: the bound of a value that went through one rounding flip (module docstring of the GPU test)
ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7}


def vec(dtype):
    """elements per 16-byte vector"""
    return 16 // torch.empty((), dtype=dtype).element_size()


def odd_pooled(shape):
    """the pooled height or width is odd: only form 1 exists"""
    _, H, W = shape
    return (H // 2) % 2 == 1 or (W // 2) % 2 == 1


def legal_forms(shape, dtype):
    if odd_pooled(shape):
        return [1]
    return [1, 2, 3] if dtype == torch.bfloat16 else [1, 2]


# ---- bits <-> bytes -----------------------------------------------------------------------------------------------------------------------
def pack_bits(bits, dtype):
    """bool [N,H,W,C] -> uint8 [N,H,W,C/V]"""
    V = vec(dtype)
    N, H, W, Cc = bits.shape
    w = (2 ** torch.arange(V, dtype=torch.int64)).view(1, 1, 1, 1, V)
    return (bits.view(N, H, W, Cc // V, V).to(torch.int64) * w).sum(-1).to(torch.uint8)


def unpack_bits(packed, dtype):
    """uint8 [N,H,W,C/V] -> bool [N,H,W,C]"""
    V = vec(dtype)
    N, H, W, cv = packed.shape
    sh = torch.arange(V, dtype=torch.int64).view(1, 1, 1, 1, V)
    return ((packed.to(torch.int64).unsqueeze(-1) >> sh) & 1).bool().view(N, H, W, cv * V)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _padded(x, fill):
    N, H, W, Cc = x.shape
    out = torch.full((N, H + 2, W + 2, Cc), fill, dtype=x.dtype)
    out[:, 1:-1, 1:-1] = x
    return out


def _tap(xp, k, H, W):
    """tap k = kh * 3 + kw of every window, [N,H/2,W/2,C], from the padded tensor"""
    kh, kw = divmod(k, 3)
    return xp[:, kh:kh + H:2, kw:kw + W:2]


def pool_codes(x):
    """3x3 / stride 2 / pad 1 max pool of finite x [N,H,W,C] (H, W even): (window maximum, code of the FIRST maximum in row-major scan order among the
    in-image taps, uint8)"""
    N, H, W, Cc = x.shape
    xp = _padded(x.double(), float("-inf"))
    best = torch.full((N, H // 2, W // 2, Cc), float("-inf"), dtype=torch.float64)
    code = torch.full(best.shape, 255, dtype=torch.uint8)
    for k in range(9):  # scan order; an out-of-image tap is -inf and never beats anything, every window has an in-image tap
        t = _tap(xp, k, H, W)
        better = t > best
        best = torch.where(better, t, best)
        code = torch.where(better, torch.full_like(code, k), code)
    return best, code


def tap_values(x, idx, fill=float("nan")):
    """x at the tap every code names, [N,H/2,W/2,C]; `fill` where the code names a tap outside the image (or is no code at all)"""
    N, H, W, Cc = x.shape
    xp = _padded(x.double(), fill)
    out = torch.full((N, H // 2, W // 2, Cc), fill, dtype=torch.float64)
    for k in range(9):
        out = torch.where(idx == k, _tap(xp, k, H, W), out)
    return out


class Fwd(NamedTuple):
    p: torch.Tensor       # pooled value, fp64 holding a value of dtype
    idx: torch.Tensor     # uint8 window code
    bits: torch.Tensor    # bool, a > 0
    stored: torch.Tensor  # relu(a) as the unfused path would store it: fp64 holding a value of dtype
    a: torch.Tensor       # y * scale + shift, fp64
    mag: torch.Tensor     # |y * scale| + |shift|, fp64: what a's rounding errors scale with


def ref_fwd(y, scale, shift, dtype):
    yd, sc, sh = y.double(), scale.double().view(1, 1, 1, -1), shift.double().view(1, 1, 1, -1)
    prod = yd * sc
    a = prod + sh
    bits = a > 0
    stored = torch.where(bits, a, torch.zeros_like(a)).float().to(dtype).double()  # ReLU, one rounding to fp32 (the kernel's fma), one to dtype
    p, idx = pool_codes(stored)
    return Fwd(p, idx, bits, stored, a, prod.abs() + sh.abs())


class Bwd(NamedTuple):
    dx: torch.Tensor      # fp64 [N,H,W,C]
    dgamma: torch.Tensor  # fp64 [C]
    dbeta: torch.Tensor
    abs_g: torch.Tensor   # sum |g|, sum |g * xhat| per channel: what the sums' rounding errors scale with
    abs_gx: torch.Tensor
    g: torch.Tensor       # the masked pool gradient, fp64 holding a value of dtype


def pool_scatter(dp, idx, shape):
    """the max pool's backward under the GIVEN codes: a pixel's fp32 sum, in (oh, ow) order, of the dp whose code names it.  fp32 [N,H,W,C]"""
    N, H, W, Cc = shape
    gp = torch.zeros((N, H + 2, W + 2, Cc), dtype=torch.float32)
    d = dp.float()
    zero = torch.zeros_like(d)
    for k in range(8, -1, -1):  # ascending (oh, ow) at a fixed pixel is descending (kh, kw); one window per pixel and pass
        kh, kw = divmod(k, 3)
        gp[:, kh:kh + H:2, kw:kw + W:2] += torch.where(idx == k, d, zero)
    return gp[:, 1:-1, 1:-1].contiguous()


def ref_bwd(dp, idx, bits, y, gamma, mean, invstd, dtype):
    """teacher-forced on idx (uint8) and bits (bool)"""
    shape = tuple(y.shape)
    M = shape[0] * shape[1] * shape[2]
    v = lambda t: t.double().view(1, 1, 1, -1)  # noqa: E731
    g = pool_scatter(dp, idx, shape).to(dtype).double()
    g = torch.where(bits, g, torch.zeros_like(g))
    xhat = (y.double() - v(mean)) * v(invstd)
    gx = g * xhat
    dbeta, dgamma = g.sum((0, 1, 2)), gx.sum((0, 1, 2))
    dx = v(gamma) * v(invstd) * (g - v(dbeta) / M - xhat * v(dgamma) / M)
    return Bwd(dx, dgamma, dbeta, g.abs().sum((0, 1, 2)), gx.abs().sum((0, 1, 2)), g)


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(shape, seed, lo, hi, step):
    """k * step for integer k in lo .. hi, fp32"""
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float() * step


EXACT_SCALES = (0.5, 1.0, 2.0, -1.0, 0.25, -0.5)


@functools.lru_cache(maxsize=None)
def exact_fwd_data(shape, dtype):
    """dyadic grids: y on k/4 in [-3, 3], scale per channel from EXACT_SCALES, shift on k/2 in [-2, 2] — a = y * scale + shift is a multiple of 1/16 below
    8 in magnitude, exact in fp32 and in bf16: zeros, negative zeros, plateaus and all-negative windows everywhere.  (y in dtype, scale, shift)"""
    N, H, W = shape
    y = _grid((N, H, W, C), 101, -12, 12, 0.25)
    scale = torch.tensor(EXACT_SCALES)[torch.randint(0, len(EXACT_SCALES), (C,), generator=_gen(102))]
    shift = _grid((C,), 103, -4, 4, 0.5)
    # a sum is -0 only when both addends are: half of the zeros of y and every other zero of shift carry the sign
    minus0 = torch.tensor(-0.0)
    y = torch.where((y == 0) & (torch.rand(y.shape, generator=_gen(104)) < 0.5), minus0, y)
    shift = torch.where((shift == 0) & (torch.arange(C) % 2 == 1), minus0, shift)
    return y.to(dtype), scale, shift


@functools.lru_cache(maxsize=None)
def exact_fwd_ref(shape, dtype):
    return ref_fwd(*exact_fwd_data(shape, dtype), dtype)


EXACT_UNIT = 1.0 / 32   # every term of the exact backward's sums is a multiple of it
EXACT_PREFILL = 8       # |prefilled dgamma / dbeta| of the beta_acc = 1 run, integers


@functools.lru_cache(maxsize=None)
def exact_bwd_data(shape, dtype):
    """dp on k/4 in [-2, 2], mean on k/2 in [-1, 1], invstd from {0.5, 1, 2}, gamma from {0.5, 1, -2}: g (at most four dp) is a multiple of 1/4 below 8,
    xhat = (y - mean) * invstd a multiple of 1/8, every term of both sums a multiple of EXACT_UNIT.  (dp in dtype, gamma, mean, invstd)"""
    N, H, W = shape
    dp = _grid((N, H // 2, W // 2, C), 111, -8, 8, 0.25).to(dtype)
    gamma = torch.tensor([0.5, 1.0, -2.0])[torch.randint(0, 3, (C,), generator=_gen(112))]
    mean = _grid((C,), 113, -2, 2, 0.5)
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=_gen(114))]
    return dp, gamma, mean, invstd


@functools.lru_cache(maxsize=None)
def exact_bwd_ref(shape, dtype):
    """the reference backward on the reference forward's own codes and bits"""
    f = exact_fwd_ref(shape, dtype)
    y = exact_fwd_data(shape, dtype)[0]
    dp, gamma, mean, invstd = exact_bwd_data(shape, dtype)
    return ref_bwd(dp, f.idx, f.bits, y, gamma, mean, invstd, dtype)


def sums_are_exact(b):
    """any fp32 summation order reproduces the exact backward's sums: sum |terms| (+ the prefill of the accumulating run), in units, stays below 2^24"""
    worst = max(b.abs_g.max().item(), b.abs_gx.max().item()) + EXACT_PREFILL
    return worst / EXACT_UNIT < 2.0 ** 24


RANDOM_SEED = 7


@functools.lru_cache(maxsize=None)
def random_fwd_data(shape, dtype, seed=RANDOM_SEED):
    """continuous data, mixed-sign scales of magnitude 0.5 .. 1.5, shift in (-0.5, 0.5): about half of the activations are clipped.  Magnitudes stay far above
    the subnormal range (positive values below 2^-134 are the documented bit difference of form 3) and there is no NaN."""
    N, H, W = shape
    y = torch.randn((N, H, W, C), generator=_gen(seed)).to(dtype)
    u = torch.rand((C,), generator=_gen(seed + 1))
    sign = torch.where(torch.rand((C,), generator=_gen(seed + 2)) < 0.35, -1.0, 1.0)
    scale = (0.5 + u) * sign
    shift = torch.rand((C,), generator=_gen(seed + 3)) - 0.5
    return y, scale, shift


@functools.lru_cache(maxsize=None)
def random_fwd_ref(shape, dtype, seed=RANDOM_SEED):
    return ref_fwd(*random_fwd_data(shape, dtype, seed), dtype)


@functools.lru_cache(maxsize=None)
def random_bwd_data(shape, dtype, seed=RANDOM_SEED):
    """(dp in dtype, gamma mixed sign, mean, invstd): statistics near those of y ~ N(0, 1), not exactly them (the op takes them as given)"""
    N, H, W = shape
    dp = torch.randn((N, H // 2, W // 2, C), generator=_gen(seed + 10)).to(dtype)
    gamma = torch.randn((C,), generator=_gen(seed + 11)) + 0.5
    mean = 0.2 * torch.randn((C,), generator=_gen(seed + 12))
    invstd = 0.7 + 0.6 * torch.rand((C,), generator=_gen(seed + 13))
    return dp, gamma, mean, invstd


@functools.lru_cache(maxsize=None)
def free_codes(shape, seed=5):
    """codes 0 .. 8 and bits drawn freely, for a teacher-forced backward: border windows name taps outside the image (which no pixel takes) and every
    (pixel, window) pair occurs.  With a forward's own codes a window off the edge can never name a pixel — its row -1 / column -1 taps lie outside
    the image — so only such codes show whether the backward voids it."""
    N, H, W = shape
    idx = torch.randint(0, 9, (N, H // 2, W // 2, C), generator=_gen(seed)).to(torch.uint8)
    bits = torch.rand((N, H, W, C), generator=_gen(seed + 1)) < 0.7
    return idx, bits


# ---- comparisons (each returns the figures it asserted on) --------------------------------------------------------------------------------
def _bitpattern(t, dtype):
    t = t.detach().cpu()
    assert t.dtype == dtype, (t.dtype, dtype)
    return t.contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16)


def _where(bad):
    return [tuple(i) for i in bad.nonzero()[:4].tolist()]


def check_fwd_exact(p, idx, bits, ref, dtype, what=""):
    """p (dtype), idx (uint8) and the packed bits of a forward equal the reference bit for bit"""
    idx, bits = idx.detach().cpu(), bits.detach().cpu()
    bad = _bitpattern(p, dtype) != _bitpattern(ref.p.to(dtype), dtype)
    assert not bad.any(), f"{what}: {int(bad.sum())} pooled values differ, first at {_where(bad)}"
    bad = idx != ref.idx
    assert not bad.any(), f"{what}: {int(bad.sum())} codes differ, first at {_where(bad)}: got {idx[bad][:4].tolist()}, reference {ref.idx[bad][:4].tolist()}"
    bad = bits != pack_bits(ref.bits, dtype)
    assert not bad.any(), f"{what}: {int(bad.sum())} bit bytes differ, first at {_where(bad)}"


BITS_SLACK = 2.0 ** -20        # a is "at zero" where |a| <= BITS_SLACK * (|y * scale| + |shift|): its sign is the fp32 fma's business
BITS_EXCLUDED_MAX = 1e-3       # share of elements that may be at zero


def bits_excluded(ref):
    """elements whose bit the random tier does not compare"""
    return ref.a.abs() <= BITS_SLACK * ref.mag


def check_fwd_random(p, idx, bits, ref, dtype, what=""):
    """value within one flipped rounding of the reference, code naming an in-image tap that holds that value, bits equal a > 0 away from zero"""
    u = ULP[dtype]
    p, idx = p.detach().cpu().double(), idx.detach().cpu()
    assert torch.isfinite(p).all(), what
    bad = (p - ref.p).abs() > u * ref.p.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} pooled values off by more than {u:.3g} of the reference, first at {_where(bad)}"
    named = tap_values(ref.stored, idx)
    bad = torch.isnan(named)
    assert not bad.any(), f"{what}: {int(bad.sum())} codes name no in-image tap, first at {_where(bad)}: {idx[bad][:4].tolist()}"
    bad = (named - p).abs() > u * named.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())} codes name a tap that does not hold the pooled value, first at {_where(bad)}"
    skip = bits_excluded(ref)
    share = skip.double().mean().item()
    assert share <= BITS_EXCLUDED_MAX, f"{what}: {share:.2%} of the elements are at zero"
    bad = (unpack_bits(bits.detach().cpu(), dtype) != ref.bits) & ~skip
    assert not bad.any(), f"{what}: {int(bad.sum())} ReLU bits differ from a > 0, first at {_where(bad)}"
    return {"excluded": share}


def check_sums_exact(dgamma, dbeta, ref, prefill_g=None, prefill_b=None, what=""):
    """dgamma / dbeta equal the fp64 sums (plus what they were accumulated onto) exactly"""
    eg = ref.dgamma + (prefill_g.double() if prefill_g is not None else 0.0)
    eb = ref.dbeta + (prefill_b.double() if prefill_b is not None else 0.0)
    dg, db = dgamma.detach().cpu().double(), dbeta.detach().cpu().double()
    bad = dg != eg
    assert not bad.any(), f"{what}: dgamma differs in channels {_where(bad)}: got {dg[bad][:4].tolist()}, reference {eg[bad][:4].tolist()}"
    bad = db != eb
    assert not bad.any(), f"{what}: dbeta differs in channels {_where(bad)}: got {db[bad][:4].tolist()}, reference {eb[bad][:4].tolist()}"


SUMS_TOL = 1e-5   # of sum |terms|: a thread's fp32 chain is at most ~24 adds before the fp64 finalize, worst case ~2e-6; five times that


def sums_ratios(dgamma, dbeta, ref):
    """largest |sum - ref| / sum |terms| over the channels, for dgamma and dbeta (a channel without terms must be 0: any other value is inf)"""
    dg, db = dgamma.detach().cpu().double(), dbeta.detach().cpu().double()
    rg = ((dg - ref.dgamma).abs() / ref.abs_gx.clamp_min(1e-300)).max().item()
    rb = ((db - ref.dbeta).abs() / ref.abs_g.clamp_min(1e-300)).max().item()
    return rg, rb


def check_sums_random(dgamma, dbeta, ref, what=""):
    assert torch.isfinite(dgamma).all() and torch.isfinite(dbeta).all(), what
    rg, rb = sums_ratios(dgamma, dbeta, ref)
    assert rg <= SUMS_TOL and rb <= SUMS_TOL, f"{what}: dgamma off by {rg:.3g} of sum |g xhat|, dbeta by {rb:.3g} of sum |g| (bound {SUMS_TOL:g})"
    return {"dgamma": rg, "dbeta": rb}


DX_NERR_F32 = 1e-4   # the bar test_bn_train_fwd_bwd uses


def check_dx(dx, ref, dtype, what=""):
    """fp32: normalised max error.  bf16: per element, one RNE rounding (2^-9) with a factor 2, plus the fp32 bar on the tensor's scale"""
    d = dx.detach().cpu().double()
    assert d.shape == ref.dx.shape and torch.isfinite(d).all(), what
    err = (d - ref.dx).abs()
    top = ref.dx.abs().max().clamp_min(1e-300)
    if dtype == torch.float32:
        n = (err.max() / top).item()
        assert n < DX_NERR_F32, f"{what}: dx normalised max error {n:.3g}"
        return {"nerr": n}
    bound = 2.0 ** -8 * ref.dx.abs() + DX_NERR_F32 * top
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} dx elements out of bound, first at {_where(bad)}, worst ratio {(err / bound).max().item():.3g}"
    return {"worst_ratio": (err / bound).max().item()}
