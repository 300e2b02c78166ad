"""What tests/test_bn_host.py and tests/test_bn_gpu.py share: the BatchNorm kernels of csrc/bn.hip, per op.

Three things live here.

1. A plain fp64 REFERENCE of the three operations the executors launch: the training statistics (mean, biased variance, invstd, scale / shift, running
   statistics with the unbiased variance), the apply pass in every addend and activation form with its ReLU bits, and the backward (dz, dgamma, dbeta, dx),
   teacher-forced on the mean / invstd / bits it is given.

2. An fp32 RESTATEMENT of the same passes in the kernels' order (rs_*): a thread's row walk, the wave shuffle or the LDS rows, the block partial, the
   fp64 finalize in slice-then-tree order, the fma of the apply, the rounding to the dtype.  reduce_layout / fin_form / elementwise_blocks restate
   reduce_grid / fin_one_channel / elementwise_blocks of bn.hip.  Every rs_* function takes `plant`, a set of names of errors to commit on purpose
   (test_bn_host.py shows that each breaks a check).  The restatement rounds every product (the compiler may contract `s2 += d * d` into one fma, which
   drops a rounding: the bounds count the rounding).

3. DATA and COMPARISONS.  Exact data: dyadic grids on which every fp32 operation of every pass is exact whatever the summation order, so the GPU must
   return the fp64 reference bit for bit (what passes through 1 / sqrt — invstd, scale, shift and what follows — is held to one fp32 ulp of the fp64 value
   instead; equality is of values: the kernels write -0.0 where ReLU clips a negative value without a bit mask, the reference +0.0).  Random data: every
   bound is derived next to its constant and is checked on the CPU against the restatement by test_bn_host.py; none comes from a GPU's output.

Tensors are [M][C] (NHWC with the pixels flattened).  Bits travel as booleans here; pack / unpack convert to the kernels' bytes ([M][C / V], V = 16 bytes of
elements, bit e of byte v = channel v * V + e)."""
import functools
import math
from typing import NamedTuple

import torch

from stem_tail_common import BITS_EXCLUDED_MAX, BITS_SLACK, DTYPES, pack_bits as _pack4, unpack_bits as _unpack4, vec  # noqa: F401

U32 = 2.0 ** -24                # unit roundoff of fp32: one rounding changes a value by at most U32 of its magnitude
HALF = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}   # the rounding of an fp32 value to the dtype, relative (bf16: 8 significant bits, round to nearest)
SLOPE = float(torch.tensor(0.01, dtype=torch.float32))   # the leaky ReLU's slope as the kernels hold it
EPS = 1e-5
MAXBLK, FIN_WIDE_ROWS = 512, 4096


def cdiv(a, b):
    return (a + b - 1) // b


def pack(bits, dtype):
    """bool [M,C] -> uint8 [M,C/V]"""
    M, C = bits.shape
    return _pack4(bits.view(1, 1, M, C), dtype).view(M, C // vec(dtype))


def unpack(packed, dtype):
    """uint8 [M,C/V] -> bool [M,C]"""
    M, cv = packed.shape
    return _unpack4(packed.view(1, 1, M, cv), dtype).view(M, cv * vec(dtype))


# ---- launch geometry, restated ------------------------------------------------------------------------------------------------------------
class Layout(NamedTuple):
    V: int
    tpr: int        # threads per row of a workgroup (channel vectors it covers)
    rpp: int        # row lanes of a workgroup
    gy: int         # workgroups across the channels
    nblk: int       # partial rows written
    chain: int      # rows a thread walks at most: the length of its fp32 chain
    lane_adds: int  # fp32 adds between a thread's sum and the block partial


def reduce_layout(dtype, M, C):
    """reduce_grid of bn.hip"""
    V = vec(dtype)
    tpr_full = C // V
    tpr = min(tpr_full, 256)
    rpp = 256 // tpr
    gy = tpr_full // tpr
    nblk = max(1, min(cdiv(M, rpp * 8), MAXBLK // gy))
    lane_adds = int(math.log2(64 // tpr)) + 4 if tpr < 64 else rpp   # shuffle levels + the four waves' LDS rows | one LDS row per lane
    return Layout(V, tpr, rpp, gy, nblk, cdiv(M, nblk * rpp), lane_adds)


FIN_FORMS = {"four": (4, 256), "one": (1, 256), "wide": (1, 1024)}   # name -> (channels per workgroup, threads)


def fin_form(C, nblk):
    """fin_one_channel + FIN_WIDE_ROWS of bn.hip (rule 2, the only one built)"""
    if (C <= 128 and nblk > 512) or (C <= 512 and nblk >= 128):
        return "wide" if nblk > FIN_WIDE_ROWS else "one"
    return "four"


def fin_slices(form):
    cpw, bt = FIN_FORMS[form]
    return bt // cpw


def elementwise_blocks(nvec, plant=()):
    b = cdiv(nvec, 4 * 256)
    if "stale_c0" in plant:   # the stride is no longer a multiple of the channel vectors, and a thread keeps the constants of its first vector
        return b
    b = max(4, min(b, 65536))
    return cdiv(b, 4) * 4


# ---- fp64 reference -----------------------------------------------------------------------------------------------------------------------
class Stats(NamedTuple):
    mean: torch.Tensor      # fp64 [C]
    var: torch.Tensor       # biased
    invstd: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    rm: torch.Tensor        # running statistics after the update
    rv: torch.Tensor


def ref_stats(x, gamma, beta, rm, rv, momentum, eps=EPS):
    xd = x.double()
    M = xd.shape[0]
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    unb = var * M / (M - 1) if M > 1 else var
    mom = float(torch.tensor(momentum, dtype=torch.float32))
    return Stats(mean, var, invstd, scale, shift, (1 - mom) * rm.double() + mom * mean, (1 - mom) * rv.double() + mom * unb)


class Apply(NamedTuple):
    out: torch.Tensor    # act(a), fp64, before the rounding to the dtype
    bits: torch.Tensor   # bool, a > 0
    a: torch.Tensor      # the sum before the activation
    mag: torch.Tensor    # sum of the magnitudes of everything added: what the fp32 roundings scale with


def ref_apply(x, scale, shift, residual=None, x2=None, scale2=None, shift2=None, relu=1):
    p = x.double() * scale.double()
    a, mag = p + shift.double(), p.abs() + shift.double().abs()
    if residual is not None:
        a, mag = a + residual.double(), mag + residual.double().abs()
    if x2 is not None:
        p2 = x2.double() * scale2.double()
        a, mag = a + p2 + shift2.double(), mag + p2.abs() + shift2.double().abs()
    bits = a > 0
    out = a if relu == 0 else torch.where(bits, a, a * (SLOPE if relu == 2 else 0.0))
    return Apply(out, bits, a, mag)


class Bwd(NamedTuple):
    dz: torch.Tensor       # fp64 [M,C]: the masked gradient
    dx: torch.Tensor
    dgamma: torch.Tensor   # fp64 [C], without any prefill
    dbeta: torch.Tensor
    abs_g: torch.Tensor    # sum |dz|, sum |dz * xhat| per channel
    abs_gx: torch.Tensor
    xhat: torch.Tensor
    k0: torch.Tensor       # gamma * invstd


def ref_bwd(g, bits, x, gamma, mean, invstd, relu):
    """bits: bool [M,C] or None (relu 0)"""
    gd = g.double()
    M = gd.shape[0]
    dz = gd if relu == 0 else torch.where(bits, gd, gd * (SLOPE if relu == 2 else 0.0))
    xhat = (x.double() - mean.double()) * invstd.double()
    gx = dz * xhat
    dbeta, dgamma = dz.sum(0), gx.sum(0)
    k0 = gamma.double() * invstd.double()
    dx = k0 * (dz - dbeta / M - xhat * dgamma / M)
    return Bwd(dz, dx, dgamma, dbeta, dz.abs().sum(0), gx.abs().sum(0), xhat, k0)


# ---- fp32 restatement in the kernels' order -----------------------------------------------------------------------------------------------
def _grid(t, lay, M):
    """[M,C] -> [chain][nblk][rpp][C]: row m = (it * nblk + b) * rpp + r is the it-th row of lane r of workgroup b; zero past M"""
    C = t.shape[1]
    pad = lay.chain * lay.nblk * lay.rpp - M
    return torch.cat([t, t.new_zeros(pad, C)]).view(lay.chain, lay.nblk, lay.rpp, C)


def _lanes(s, lay):
    """a workgroup's lane sums [nblk][rpp][C] -> its partial row [nblk][C]"""
    nblk, _, C = s.shape
    if lay.tpr < 64:   # lanes that share a wavefront: xor butterfly, then the four waves' rows in order
        w = 64 // lay.tpr
        s = s.view(nblk, 4, w, C)
        off = 1
        while off < w:
            s = s + s[:, :, torch.arange(w) ^ off]
            off <<= 1
        rows = s[:, :, 0]
    else:
        rows = s
    a = torch.zeros(nblk, C)
    for rr in range(rows.shape[1]):
        a = a + rows[:, rr]
    return a


def rs_reduce(lay, x, dz=None, mean=None, invstd=None, plant=()):
    """bn_reduce_kernel.  MODE 0 (dz None): (partial rows [nblk,2,C] of sum (x - pivot), sum (x - pivot)^2, pivot);
    MODE 1: (rows of sum dz, sum dz * xhat, None)"""
    M, C = x.shape
    xf = x.float()
    valid = _grid(torch.ones(M, 1), lay, M) > 0
    zero = torch.zeros(())
    if dz is None:
        pivot = torch.zeros(C) if "no_pivot" in plant else xf[0].clone()
        d = torch.where(valid, _grid(xf, lay, M) - pivot, zero)
        t1, t2 = d, d * d
    else:
        pivot = None
        xh = (_grid(xf, lay, M) - mean) * invstd
        t1 = _grid(dz.float(), lay, M)
        t2 = torch.where(valid, t1 * xh, zero)
    if "row_twice" in plant:   # the last lane of a workgroup also takes the first row of the next one
        for t in (t1, t2):
            t[:, :-1, lay.rpp - 1] = t[:, :-1, lay.rpp - 1] + t[:, 1:, 0]
    s1 = torch.zeros(lay.nblk, lay.rpp, C)
    s2 = torch.zeros(lay.nblk, lay.rpp, C)
    for it in range(lay.chain):   # a thread's chain
        s1 = s1 + t1[it]
        s2 = s2 + t2[it]
    return torch.stack([_lanes(s1, lay), _lanes(s2, lay)], 1), pivot


def rs_fin_sums(partial, form, plant=()):
    """bn_finalize_kernel's sums: slice sl adds rows sl, sl + SL, ... in order (eight per pass), then a halving tree over the slices.  fp64 [2][C]"""
    nblk = partial.shape[0]
    SL = fin_slices(form)
    p = partial.double()
    passes = 1 if "skip_rows" in plant else cdiv(nblk, SL * 8)
    acc = torch.zeros((SL,) + tuple(p.shape[1:]), dtype=torch.float64)
    for k in range(0, min(nblk, passes * SL * 8), SL):
        n = min(SL, nblk - k)
        acc[:n] = acc[:n] + p[k:k + n]
    s = SL // 2
    while s > 0:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0]


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def rs_stats_finalize(sums, pivot, M, gamma, beta, rm, rv, momentum, eps=EPS, plant=()):
    """MODE 0 of bn_finalize_kernel from its fp64 sums: (save_mean, save_invstd, scale, shift, running_mean, running_var), fp32"""
    s1, s2 = sums[0], sums[1]
    Md = float(M)
    dm = s1 / Md
    mean = (pivot.double() if pivot is not None else 0.0) + dm
    var = (s2 / Md - dm * dm).clamp_min(0.0)
    invstd = (1.0 / torch.sqrt(var + _f32(eps).double())).float()
    meanf = mean.float()
    sc = gamma * invstd
    shift = beta - meanf * sc
    if "biased_running_var" in plant:
        unb = var
    elif M > 1 or "no_m1_guard" in plant:
        unb = var * Md / torch.tensor(Md - 1.0, dtype=torch.float64)
    else:
        unb = var
    mom = _f32(momentum)
    keep = _f32(1.0) - mom
    return meanf, invstd, sc, shift, keep * rm + mom * meanf, keep * rv + mom * unb.float()


def rs_bwd_finalize(sums, M, gamma, invstd, dgamma0, dbeta0, beta_acc, plant=()):
    """MODE 1: (dgamma, dbeta, coef [3][C] = gamma * invstd, mean dz, mean dz * xhat), fp32"""
    s1, s2 = sums[0], sums[1]
    acc = 0.0 if "no_beta_acc" in plant else beta_acc
    dbeta = (_f32(acc) * dbeta0 if acc != 0.0 else torch.zeros_like(gamma)) + s1.float()
    dgamma = (_f32(acc) * dgamma0 if acc != 0.0 else torch.zeros_like(gamma)) + s2.float()
    return dgamma, dbeta, torch.stack([gamma * invstd, (s1 / float(M)).float(), (s2 / float(M)).float()])


def _fma(a, b, c):
    """fmaf: the fp64 product of two fp32 values is exact; the sum's rounding to fp64 before the one to fp32 matters only at ties of 2^-29 of the result"""
    return (a.double() * b.double() + c.double()).float()


def _thread_channels(M, C, dtype, plant=()):
    """the channel whose constants the elementwise kernels hold for element (m, c): a thread loads them for the vector it starts at and strides on"""
    V = vec(dtype)
    cvecs = C // V
    nvec = M * cvecs
    stride = elementwise_blocks(nvec, plant) * 256
    if stride % cvecs == 0:   # every stride lands on the same channel vector: the element's own channel
        return torch.arange(C)
    i = torch.arange(nvec)
    cv = (i % stride) % cvecs
    return (cv.view(-1, 1) * V + torch.arange(V)).view(M, C)


def rs_apply(x, scale, shift, residual=None, x2=None, scale2=None, shift2=None, relu=1, plant=()):
    """bn_apply_kernel: (out in x's dtype, bits bool)"""
    M, C = x.shape
    dtype = x.dtype
    ch = _thread_channels(M, C, dtype, plant)
    v = _fma(x.float(), scale[ch], shift[ch])
    if residual is not None:
        v = v + residual.float()
    if x2 is not None:
        v = v + _fma(x2.float(), scale2[ch], shift2[ch])
    bits = v > 0
    if relu != 0:
        v = torch.where(bits, v, v * _f32(SLOPE) if relu == 2 else torch.zeros_like(v))
    if "bit_shift" in plant:   # element e lands on bit e + 1
        bits = torch.roll(bits, 1, dims=1)
    return v.to(dtype), bits


def rs_bwd(g, bits, x, gamma, mean, invstd, relu, dz_out=False, dgamma0=None, dbeta0=None, beta_acc=0.0, partial=None, form=None, plant=()):
    """the sequence of mi355_bn_bwd_bits: (dx in the dtype, dz in the dtype or None, dgamma, dbeta) — reduce (or the given rows), finalize, apply"""
    M, C = x.shape
    dtype = x.dtype
    slope = _f32(SLOPE if relu == 2 else 0.0)
    gf = g.float()

    def masked(t):
        return t if relu == 0 else torch.where(bits, t, t * slope if relu == 2 else torch.zeros_like(t))

    dz = masked(gf)
    if partial is None or dz_out:
        lay = reduce_layout(dtype, M, C)
        partial = rs_reduce(lay, x, dz, mean, invstd, plant)[0]
    nblk = partial.shape[0]
    sums = rs_fin_sums(partial, form or fin_form(C, nblk), plant)
    zeros = torch.zeros(C)
    dgamma, dbeta, coef = rs_bwd_finalize(sums, M, gamma, invstd, zeros if dgamma0 is None else dgamma0, zeros if dbeta0 is None else dbeta0, beta_acc, plant)
    stored = dz.to(dtype) if dz_out else None
    if dz_out:
        src = stored.float()
        if "mask_twice" in plant:
            src = masked(src)
    else:
        src = dz
    ch = _thread_channels(M, C, dtype, plant)
    k0, k1, k2 = coef[0][ch], coef[1][ch], coef[2][ch]
    if "swap_k" in plant:
        k1, k2 = k2, k1
    xh = (x.float() - mean[ch]) * invstd[ch]
    dx = k0 * (src - k1 - xh * k2)
    return dx.to(dtype), stored, dgamma, dbeta


def rs_stats(x, gamma, beta, rm, rv, momentum, partial=None, form=None, plant=()):
    """the statistics of mi355_bn_fwd_train (partial None: the reduce with its pivot) or mi355_bn_fwd_train_partial (plain-sum rows, no pivot)"""
    M, C = x.shape
    pivot = None
    if partial is None:
        partial, pivot = rs_reduce(reduce_layout(x.dtype, M, C), x, plant=plant)
    sums = rs_fin_sums(partial, form or fin_form(C, partial.shape[0]), plant)
    return rs_stats_finalize(sums, pivot, M, gamma, beta, rm, rv, momentum, plant=plant)


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _dyadic(shape, seed, lo, hi, step):
    """k * step for integer k in lo .. hi, fp32"""
    return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float() * step


def _pick(values, n, seed):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=_gen(seed))]


EXACT_PREFILL = 8   # |prefilled dgamma / dbeta| of the beta_acc = 1 runs, integers


class ExactFwd(NamedTuple):
    x: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    rm: torch.Tensor
    rv: torch.Tensor


@functools.lru_cache(maxsize=None)
def exact_stats_data(M, C, dtype):
    """x on k/4 in [-3, 3] ([-2, 2] from 8192 rows on): x - pivot is a multiple of 1/4 below 8, its square a multiple of 1/16 below 64.  gamma a power of
    two with a sign, beta on k/2, running statistics on k/4 (exact under momentum 0.25)"""
    r = 12 if M < 8192 else 8
    x = _dyadic((M, C), 201, -r, r, 0.25).to(dtype)
    return ExactFwd(x, _pick([0.5, 1.0, 2.0, -1.0], C, 202), _dyadic((C,), 203, -4, 4, 0.5), _dyadic((C,), 204, -8, 8, 0.25), _dyadic((C,), 205, 1, 8, 0.25))


def stats_sums_are_exact(x):
    """sum (x - pivot)^2 in units of 1/16, with the pivot that makes it largest, stays below 2^24: any fp32 summation order gives the same sums"""
    xd = x.double()
    worst = ((xd - xd[0]) ** 2).sum(0).max().item() * 16
    worst0 = (xd ** 2).sum(0).max().item() * 16   # the plain sums of the partial-row path
    return max(worst, worst0) < 2.0 ** 24


class ExactApply(NamedTuple):
    x: torch.Tensor
    scale: torch.Tensor
    shift: torch.Tensor
    residual: torch.Tensor
    x2: torch.Tensor
    scale2: torch.Tensor
    shift2: torch.Tensor


@functools.lru_cache(maxsize=None)
def exact_apply_data(M, C, dtype):
    """x, residual, x2 on k/4 in [-3, 3], scales powers of two with signs, shifts on k/2 in [-2, 2]: every sum is a multiple of 1/16 below 16 — exact in fp32
    and in bf16 (8 bits).  Zeros everywhere: x = 0 with shift = 0, and half of those zeros negative (a sum is -0 only when every addend is)"""
    x = _dyadic((M, C), 211, -12, 12, 0.25)
    res = _dyadic((M, C), 212, -12, 12, 0.25)
    x2 = _dyadic((M, C), 213, -12, 12, 0.25)
    scale = _pick([0.5, 1.0, 2.0, -1.0, 0.25, -0.5], C, 214)
    scale2 = _pick([0.5, 1.0, -1.0, 0.25], C, 215)
    shift = _dyadic((C,), 216, -4, 4, 0.5)
    shift2 = _dyadic((C,), 217, -2, 2, 0.5)
    minus0 = torch.tensor(-0.0)
    coin = torch.rand((M, C), generator=_gen(218)) < 0.5
    x = torch.where((x == 0) & coin, minus0, x)
    res = torch.where((res == 0) & coin, minus0, res)
    x2 = torch.where((x2 == 0) & coin, minus0, x2)
    odd = torch.arange(C) % 2 == 1
    shift = torch.where((shift == 0) & odd, minus0, shift)
    shift2 = torch.where((shift2 == 0) & odd, minus0, shift2)
    return ExactApply(x.to(dtype), scale, shift, res.to(dtype), x2.to(dtype), scale2, shift2)


class ExactBwd(NamedTuple):
    g: torch.Tensor
    bits: torch.Tensor   # bool
    x: torch.Tensor
    gamma: torch.Tensor
    mean: torch.Tensor
    invstd: torch.Tensor
    dgamma0: torch.Tensor
    dbeta0: torch.Tensor


EXACT_UNIT = 1.0 / 32   # every term of the exact backward's sums is a multiple of it


@functools.lru_cache(maxsize=None)
def exact_bwd_data(M, C, dtype):
    """g on k/4 in [-2, 2] ([-1, 1] from 8192 rows on), x on k/4 in [-3, 3], mean on k/2 in [-1, 1], invstd from {0.5, 1, 2}, gamma from {0.5, 1, -2}: xhat is
    a multiple of 1/8 below 8, every term of both sums a multiple of EXACT_UNIT below 16.  Integer prefill for the accumulating runs"""
    r = 8 if M < 8192 else 4
    g = _dyadic((M, C), 221, -r, r, 0.25).to(dtype)
    x = _dyadic((M, C), 222, -12, 12, 0.25).to(dtype)
    bits = torch.rand((M, C), generator=_gen(223)) < 0.6
    return ExactBwd(g, bits, x, _pick([0.5, 1.0, -2.0], C, 224), _dyadic((C,), 225, -2, 2, 0.5), _pick([0.5, 1.0, 2.0], C, 226),
                    _dyadic((C,), 227, -EXACT_PREFILL, EXACT_PREFILL, 1.0), _dyadic((C,), 228, -EXACT_PREFILL, EXACT_PREFILL, 1.0))


def bwd_sums_are_exact(ref):
    """sum |terms| plus the prefill, in units, stays below 2^24"""
    return (max(ref.abs_g.max().item(), ref.abs_gx.max().item()) + EXACT_PREFILL) / EXACT_UNIT < 2.0 ** 24


def _is_f32(t):
    return bool((t.float().double() == t).all())


def bwd_dx_is_exact(ref, M):
    """every intermediate of dx = k0 * (dz - k1 - xhat * k2) is an fp32 value, so dx is the same whatever is fused: true on the exact data at small
    powers of two M (a quotient by M enters k1 and k2), not beyond"""
    k1, k2 = ref.dbeta / M, ref.dgamma / M
    t1, t2 = ref.dz - k1, ref.xhat * k2
    return all(_is_f32(t) for t in (k1, k2, t1, t2, t1 - t2, ref.k0 * (t1 - t2)))


@functools.lru_cache(maxsize=None)
def random_stats_data(M, C, dtype, seed=31):
    x = (torch.randn((M, C), generator=_gen(seed)) * 1.2 + 0.3).to(dtype)
    return ExactFwd(x, torch.randn((C,), generator=_gen(seed + 1)) + 1.5, torch.randn((C,), generator=_gen(seed + 2)),
                    torch.randn((C,), generator=_gen(seed + 3)), torch.rand((C,), generator=_gen(seed + 4)) + 0.5)


@functools.lru_cache(maxsize=None)
def random_apply_data(M, C, dtype, seed=41):
    """mixed-sign scales of magnitude 0.5 .. 1.5, shifts in (-0.5, 0.5): about half of the sums are negative; no NaN, nothing near the subnormal range"""
    def sc(s):
        u = torch.rand((C,), generator=_gen(s))
        return (0.5 + u) * torch.where(torch.rand((C,), generator=_gen(s + 1)) < 0.35, -1.0, 1.0)
    t = lambda s: torch.randn((M, C), generator=_gen(s)).to(dtype)  # noqa: E731
    return ExactApply(t(seed), sc(seed + 1), torch.rand((C,), generator=_gen(seed + 3)) - 0.5, t(seed + 4), t(seed + 5), sc(seed + 6),
                      torch.rand((C,), generator=_gen(seed + 8)) - 0.5)


@functools.lru_cache(maxsize=None)
def random_bwd_data(M, C, dtype, seed=51):
    """statistics near those of x ~ N(0.3, 1.2), not exactly them (the op takes them as given); bits drawn freely"""
    g = torch.randn((M, C), generator=_gen(seed)).to(dtype)
    x = (torch.randn((M, C), generator=_gen(seed + 1)) * 1.2 + 0.3).to(dtype)
    bits = torch.rand((M, C), generator=_gen(seed + 2)) < 0.6
    return ExactBwd(g, bits, x, torch.randn((C,), generator=_gen(seed + 3)) + 0.5, 0.3 + 0.2 * torch.randn((C,), generator=_gen(seed + 4)),
                    0.6 + 0.5 * torch.rand((C,), generator=_gen(seed + 5)), torch.randn((C,), generator=_gen(seed + 6)),
                    torch.randn((C,), generator=_gen(seed + 7)))


def partition_rows(terms, nblk, seed=61):
    """synthetic partial rows [nblk][k][C] (fp32) that are an exact partition of the column sums of terms [k][M][C] (dyadic, fp64): the M rows are dealt
    unevenly — a third onto the first rows, a third anywhere, the rest onto the LAST rows (those a finalize pass could forget) — most rows stay empty
    when nblk > M, and pairs of rows carry +d / -d (d a small integer), which cancel in the sum only if both are added"""
    k, M, C = terms.shape
    g = _gen(seed + nblk)
    where = torch.randint(0, nblk, (M,), generator=g)
    third = M // 3
    where[:third] = torch.randint(0, min(nblk, 3), (third,), generator=g)
    where[2 * third:] = nblk - 1 - torch.randint(0, min(nblk, 5), (M - 2 * third,), generator=g)
    rows = torch.zeros((nblk, k, C), dtype=torch.float64)
    rows.index_add_(0, where, terms.permute(1, 0, 2).contiguous())
    if nblk > 1:
        npair = min(nblk // 2, 16)
        a = torch.randint(0, nblk, (npair,), generator=g)
        b = (a + 1 + torch.randint(0, nblk - 1, (npair,), generator=g)) % nblk   # never a itself
        d = torch.randint(-3, 4, (npair, k, C), generator=g).double()
        rows.index_add_(0, a, d)
        rows.index_add_(0, b, -d)
    assert _is_f32(rows) and bool((rows.sum(0) == terms.sum(1)).all())
    return rows.float()


def fwd_terms(x):
    xd = x.double()
    return torch.stack([xd, xd * xd])


def bwd_terms(ref):
    return torch.stack([ref.dz, ref.dz * ref.xhat])


OFFSET_CASES = ["f32_ratio100", "f32_pivot8", "bf16_mean64"]
OFFSET_M, OFFSET_C = 777, 64


@functools.lru_cache(maxsize=None)
def offset_data(name):
    """|mean| >> std.  f32_ratio100: mean 100 std 1;  f32_pivot8: the same with row 0 — the pivot — 8 std above the mean;  bf16_mean64: 64 + k / 2, k in
    0 .. 8, on the bf16 grid of [64, 128) (std about 1.3)"""
    M, C = OFFSET_M, OFFSET_C
    if name == "bf16_mean64":
        x = (64.0 + _dyadic((M, C), 71, 0, 8, 0.5)).to(torch.bfloat16)
    else:
        x = 100.0 + torch.randn((M, C), generator=_gen(72))
        if name == "f32_pivot8":
            x[0] = 108.0
    return ExactFwd(x, torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C))


def plain_rows(x, nblk):
    """what a conv epilogue leaves: fp32 rows of sum x, sum x^2 over nblk groups of consecutive pixels, each row one correctly rounded sum (the epilogue's
    own accumulation error is its kernels' business: tests/test_ops_gpu.py), no pivot"""
    t = fwd_terms(x)
    M = t.shape[1]
    edges = [M * i // nblk for i in range(nblk + 1)]
    return torch.stack([t[:, a:b].sum(1) for a, b in zip(edges[:-1], edges[1:])]).float()


# ---- bounds (each next to its derivation) and comparisons ---------------------------------------------------------------------------------
def sum_bound(lay):
    """|fp32 block sums, finalized in fp64 - exact sum| <= sum_bound * sum |terms|.  A term takes at most three roundings before it is added (x - pivot and
    the square; x - mean, * invstd, * dz), then takes part in at most chain adds of its thread and lane_adds adds of the workgroup, each off by at most U32
    of a partial sum that never exceeds sum |terms|; the fp64 finalize adds 2^-53 per row; the result is rounded to fp32 once (dgamma / dbeta, the
    coefficients); one more unit covers the second-order terms ((1 + U32)^n - 1 - n U32 for n <= 40)."""
    return (lay.chain + lay.lane_adds + 3 + 1 + 1) * U32


ROWS_BOUND = 2 * U32   # given rows, each the correct rounding of its group's sum: U32 of sum |terms| in all, + the rounding of the result


def var_rel_bound(sb, factor):
    """|var - exact| <= 3 sb factor var, with factor = ((pivot - mean)^2 + var) / var (pivot 0 on the plain-sum path): var = S2 / M - (S1 / M)^2 with
    S2 = sum d^2 off by sb * sum d^2 = sb M factor var, and S1 / M off by sb * sum |d| / M <= sb sqrt(factor var) against |S1 / M| = |pivot - mean| <=
    sqrt(factor var): the square moves by at most 2 sb factor var (+ second order, inside the unit sum_bound keeps for it)"""
    return 3.0 * sb * factor


def invstd_rel_bound(var_rel):
    """invstd = (var + eps)^-1/2 moves by half the relative change of var + eps <= that of var, to first order; 1 / (1 - e) bounds the rest for e < 1;
    + one fp32 ulp for the fp64 -> fp32 rounding on both sides"""
    assert (var_rel < 0.5).all() if torch.is_tensor(var_rel) else var_rel < 0.5
    return 0.5 * var_rel / (1.0 - var_rel) + 2 * U32


def _where(bad):
    return [tuple(i) for i in bad.nonzero()[:4].tolist()]


def _d(t):
    return t.detach().cpu().double()


def _assert_within(got, ref, bound, what):
    got = _d(got)
    assert got.shape == ref.shape and torch.isfinite(got).all(), f"{what}: shape or non-finite values"
    err = (got - ref).abs()
    bad = err > bound
    ratio = (err / bound.clamp_min(1e-300)).max().item() if torch.is_tensor(bound) else err.max().item() / max(bound, 1e-300)
    assert not bad.any(), f"{what}: {int(bad.sum())} values out of bound, first at {_where(bad)}, worst {ratio:.3g} of the bound"
    return ratio


def _assert_equal(got, ref, what):
    """equality of values (the sign of a zero aside), no NaN"""
    got = _d(got)
    assert got.shape == ref.shape, what
    bad = ~(got == ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {_where(bad)}: got {got[bad][:4].tolist()}, reference {ref[bad][:4].tolist()}"


def rounded(t, dtype):
    """fp64 -> the dtype (through fp32, as the kernels) -> fp64"""
    return t.float().to(dtype).double()


# running statistics: keep = 1 - momentum, two products and a sum in fp32, each U32 of its magnitude (4 roundings, or 3 fused), on top of what the
# batch statistic itself is off by
RUNNING_OPS = 4


def check_stats(got, ref, data, M, momentum, var_rel, mean_exact, what=""):
    """got: (save_mean, save_invstd, running_mean, running_var) of a training forward.  var_rel: the bound of the relative error of var (var_rel_bound; fp64
    noise on exact data).  mean_exact: the sums are exact and M is a power of two, so save_mean must equal the reference bit for bit; in any case it is
    held to mean_abs_bound"""
    sm, si, rm, rv = got
    check_mean(sm, ref, var_rel, what)
    mom = float(_f32(momentum))
    figures = {}
    if mean_exact:
        _assert_equal(sm, ref.mean.float().double(), f"{what} save_mean")
    ib = invstd_rel_bound(var_rel)
    figures["invstd"] = _assert_within(si, ref.invstd, ib * ref.invstd, f"{what} save_invstd")
    a, b = (1 - mom) * data.rm.double().abs(), mom * ref.mean.abs()
    figures["rm"] = _assert_within(rm, ref.rm, RUNNING_OPS * U32 * (a + b) + mom * mean_abs_bound(ref, var_rel), f"{what} running_mean")
    unb = ref.var * (M / (M - 1.0) if M > 1 else 1.0)
    a, b = (1 - mom) * data.rv.double().abs(), mom * unb
    figures["rv"] = _assert_within(rv, ref.rv, RUNNING_OPS * U32 * (a + b) + mom * unb * (var_rel + 2 * U32) + 1e-300, f"{what} running_var")
    return figures


def mean_abs_bound(ref, var_rel):
    """|save_mean - mean|: pivot + S1 / M with S1 off by sb * sum |d| <= sb M sqrt(factor var) — a third of var_rel * var / sqrt(factor var) and so below
    var_rel * sqrt(var) — then one fp32 rounding (a whole ulp: the reference's own rounding may fall the other way)"""
    return var_rel * torch.sqrt(ref.var) + 2 * U32 * ref.mean.abs()


def check_mean(sm, ref, var_rel, what=""):
    return _assert_within(sm, ref.mean, mean_abs_bound(ref, var_rel) + 1e-300, f"{what} save_mean")


def coef_bounds(ref, data, var_rel):
    """what scale = gamma * invstd and shift = beta - mean * scale may be off by: invstd's bound plus one rounding for scale; for shift the error of
    mean * scale (scale's, the mean's, one rounding of the product) and one rounding of the difference"""
    ib = invstd_rel_bound(var_rel)
    dsc = (ib + U32) * ref.scale.abs()
    dsh = dsc * ref.mean.abs() + mean_abs_bound(ref, var_rel) * ref.scale.abs() + U32 * (ref.mean * ref.scale).abs() + U32 * ref.shift.abs()
    return dsc, dsh


# fma, + residual | + fma of the second branch (2), * slope: at most four roundings, each U32 of at most mag; five with the margin for second order
APPLY_OPS = 5


def apply_bound(ref, dtype, x=None, dsc=None, dsh=None):
    """|out - act(a)| <= one rounding to the dtype of the result (HALF, of the fp32 value: (1 + HALF) carries the fp32 error through it) + the fp32
    roundings; with coefficients that are themselves off by dsc / dsh (the training forward's), |x| dsc + dsh on top"""
    fp32 = APPLY_OPS * U32 * ref.mag
    if dsc is not None:
        fp32 = fp32 + x.double().abs() * dsc + dsh
    return HALF[dtype] * ref.out.abs() + (1 + HALF[dtype]) * fp32


def bits_excluded(ref):
    """elements "at zero": the sign of a is the fp32 fma's business"""
    return ref.a.abs() <= BITS_SLACK * ref.mag


def check_apply_exact(out, bits, ref, dtype, relu=1, what=""):
    """exact data: out equals the reference (rounded to the dtype: it already is a value of it) and the bytes equal the packed a > 0 — which leaves the bit
    of 0 and -0 clear and the upper four bits of an fp32 byte zero.  Under the leaky ReLU the negative side is a * 0.01, not exact: out by its bound there"""
    assert out.dtype == dtype
    if relu == 2:
        _assert_within(out, ref.out, apply_bound(ref, dtype) + 1e-300, f"{what} out")
        _assert_equal(torch.where(ref.bits, _d(out), ref.out), rounded(ref.out, dtype).where(ref.bits, ref.out), f"{what} out, positive side")
    else:
        _assert_equal(out, rounded(ref.out, dtype), f"{what} out")
    if bits is not None:
        b = bits.detach().cpu()
        if dtype == torch.float32:
            assert not (b >> 4).any(), f"{what}: upper nibble of an fp32 mask byte set"
        bad = b != pack(ref.bits, dtype)
        assert not bad.any(), f"{what}: {int(bad.sum())} bit bytes differ, first at {_where(bad)}"


def check_apply_random(out, bits, ref, dtype, what="", x=None, dsc=None, dsh=None, skip=None):
    assert out.dtype == dtype
    fig = {"out": _assert_within(out, ref.out, apply_bound(ref, dtype, x, dsc, dsh) + 1e-300, f"{what} out")}
    if bits is not None:
        skip = bits_excluded(ref) if skip is None else skip
        share = skip.double().mean().item()
        assert share <= BITS_EXCLUDED_MAX, f"{what}: {share:.2%} of the elements are at zero"
        b = bits.detach().cpu()
        if dtype == torch.float32:
            assert not (b >> 4).any(), f"{what}: upper nibble of an fp32 mask byte set"
        bad = (unpack(b, dtype) != ref.bits) & ~skip
        assert not bad.any(), f"{what}: {int(bad.sum())} ReLU bits differ from a > 0, first at {_where(bad)}"
        fig["excluded"] = share
    return fig


def check_sums_exact(dgamma, dbeta, ref, dgamma0=None, dbeta0=None, what=""):
    _assert_equal(dgamma, ref.dgamma + (dgamma0.double() if dgamma0 is not None else 0.0), f"{what} dgamma")
    _assert_equal(dbeta, ref.dbeta + (dbeta0.double() if dbeta0 is not None else 0.0), f"{what} dbeta")


def check_sums_random(dgamma, dbeta, ref, sb, dgamma0=None, dbeta0=None, what=""):
    """sb: sum_bound(layout) or ROWS_BOUND; an accumulating run adds the prefill in fp32: one more rounding of the result"""
    eg = ref.dgamma + (dgamma0.double() if dgamma0 is not None else 0.0)
    eb = ref.dbeta + (dbeta0.double() if dbeta0 is not None else 0.0)
    extra = U32 if dgamma0 is not None else 0.0
    return {"dgamma": _assert_within(dgamma, eg, sb * ref.abs_gx + extra * eg.abs() + 1e-300, f"{what} dgamma"),
            "dbeta": _assert_within(dbeta, eb, sb * ref.abs_g + extra * eb.abs() + 1e-300, f"{what} dbeta")}


# x - mean, * invstd, dz - k1, xhat * k2, the difference, * k0, gamma * invstd, g * slope: eight roundings, each U32 of at most the magnitudes below
DX_OPS = 8


def dx_bound(ref, M, dtype, sb, relu, dz_out):
    """|dx - exact| per element: k0 times (the fp32 roundings, of |dz| + |k1| + |xhat k2|; the sums' error sb * sum |.| / M that k1 and k2 carry, k2's scaled
    by |xhat|; where a leaky dz went through a store in the dtype, its rounding), then the rounding of dx itself"""
    k1, k2 = (ref.dbeta / M).abs(), (ref.dgamma / M).abs()
    inner = DX_OPS * U32 * (ref.dz.abs() + k1 + ref.xhat.abs() * k2) + (sb + U32) * (ref.abs_g / M + ref.xhat.abs() * ref.abs_gx / M)
    if dz_out and relu == 2:
        inner = inner + HALF[dtype] * ref.dz.abs()
    return HALF[dtype] * ref.dx.abs() + (1 + HALF[dtype]) * ref.k0.abs() * inner


def check_dx_exact(dx, ref, dtype, what=""):
    assert dx.dtype == dtype
    _assert_equal(dx, rounded(ref.dx, dtype), f"{what} dx")


def check_dx_random(dx, ref, M, dtype, sb, relu, dz_out=False, what=""):
    assert dx.dtype == dtype
    return {"dx": _assert_within(dx, ref.dx, dx_bound(ref, M, dtype, sb, relu, dz_out) + 1e-300, f"{what} dx")}


def check_dz(dz, ref, dtype, relu, what=""):
    """the stored masked gradient: g itself or 0 (exact), or g * slope rounded once in fp32 and once to the dtype"""
    assert dz.dtype == dtype
    if relu != 2:
        _assert_equal(dz, ref.dz, f"{what} dz")
        return {}
    return {"dz": _assert_within(dz, ref.dz, (HALF[dtype] + (1 + HALF[dtype]) * U32) * ref.dz.abs() + 1e-300, f"{what} dz")}


# ---- case tables ----------------------------------------------------------------------------------------------------------------------------
CHANNELS = [64, 128, 256, 512, 1024, 2048, 4096]


def ragged_ms(dtype, C):
    """M = 1, 2 (the unbiased-variance branch), 5 (below the row lanes of most layouts), one short of / one past a full first workgroup round, 777"""
    rpp = reduce_layout(dtype, 1, C).rpp
    ms = sorted({1, 2, 5, rpp * 8 - 1, rpp * 8 + 1, 777})
    return [m for m in ms if C < 4096 or m <= 33]


REDUCE_CASES = [(dt, C, M) for dt in DTYPES for C in CHANNELS for M in ragged_ms(dt, C)]

# (dtype, C, M): through the real reduce — nblk 127 / 128 (the finalize form flips), nblk 128 at 64 channels, the 512-row cap (a thread's ninth row)
THRESHOLD_CASES = [(torch.float32, 512, 2032), (torch.float32, 512, 2048), (torch.bfloat16, 64, 32768), (torch.bfloat16, 2048, 4100),
                   (torch.float32, 2048, 2100)]

# every finalize form from synthetic partial rows, M = 64 rows of x: (C, nblk)
SYNTH_M = 64
SYNTH_CASES = ([(64, n) for n in (1, 63, 64, 65, 512, 513, 2048, 2049, 4096, 4097, 8193, 14336)] + [(256, n) for n in (127, 128, 600, 1024)]
               + [(1024, n) for n in (512, 513, 1024)])

APPLY_SHAPES = [(5, 64), (777, 256), (33, 4096)]
ADDENDS = ["none", "residual", "x2"]
# (relu, bits)
APPLY_ACTS = [(0, False), (1, False), (1, True), (2, False), (2, True)]


def apply_legal(addend, relu, bits):
    return not (relu == 2 and bits and addend != "none")


APPLY_FORMS = [(ad, relu, bits) for ad in ADDENDS for relu, bits in APPLY_ACTS if apply_legal(ad, relu, bits)]


def apply_args(d, addend):
    """the keyword arguments of ref_apply / rs_apply / ops.bn_apply for one addend form"""
    if addend == "residual":
        return {"residual": d.residual}
    if addend == "x2":
        return {"x2": d.x2, "scale2": d.scale2, "shift2": d.shift2}
    return {}


BWD_M, BWD_C = 64, 128     # the backward's form matrix: M a small power of two (dx exact on exact data), two workgroups of the reduce in bf16
BWD_FORMS = [(relu, dz, acc, alias) for relu in (0, 1, 2) for dz in (False, True) for acc in (0.0, 1.0) for alias in ("none", "dx", "dz")
             if dz or alias != "dz"]

# ---- the tests themselves, over a backend ---------------------------------------------------------------------------------------------------
# A backend runs the three operations on host tensors and returns host tensors: HostBackend below through the restatement (with planted errors),
# the GPU file's through ops.py.  The verify_* functions are the tests' bodies: the same assertions judge both.
class HostBackend:
    def __init__(self, plant=(), form=None):
        self.plant, self.form = set(plant), form

    def fwd_train(self, d, momentum, partial=None, relu=1):
        """(out, save_mean, save_invstd, running_mean, running_var)"""
        sm, si, sc, sh, rm, rv = rs_stats(d.x, d.gamma, d.beta, d.rm, d.rv, momentum, partial, self.form, self.plant)
        return rs_apply(d.x, sc, sh, relu=relu, plant=self.plant)[0], sm, si, rm, rv

    def apply(self, x, scale, shift, relu, want_bits, **addend):
        out, bits = rs_apply(x, scale, shift, relu=relu, plant=self.plant, **addend)
        return out, pack(bits, x.dtype) if want_bits else None

    def bwd(self, d, relu, dz_out=False, beta_acc=0.0, alias="none", partial=None):
        """(dx, dz or None, dgamma, dbeta); dgamma / dbeta start from the prefill of d whatever beta_acc is"""
        return rs_bwd(d.g, d.bits if relu else None, d.x, d.gamma, d.mean, d.invstd, relu, dz_out, d.dgamma0, d.dbeta0, beta_acc, partial, self.form,
                      self.plant)


FP64_NOISE = 1e-12   # relative error of var on exact data: the finalize's own fp64 arithmetic


def _pow2(n):
    return n & (n - 1) == 0


def _factor(pm, var):
    """((pivot - mean)^2 + var) / var; 1 where var is 0 (then every row equals the pivot and the sums are exact zeros)"""
    return torch.where(var > 0, (pm * pm + var) / var.clamp_min(1e-300), torch.ones_like(var))


def verify_stats(be, dtype, C, M, tier, momentum=0.1, partial_nblk=None, data=None, rows=None, what=None):
    """training forward: statistics, running statistics and the activation that follows.  partial_nblk: through synthetic partial rows (exact tier).
    data / rows: given data (and plain-sum rows) instead of the tier's.  Returns the figures it asserted on"""
    what = what or f"{tier} {dtype} C={C} M={M} nblk={partial_nblk}"
    d = data if data is not None else exact_stats_data(M, C, dtype) if tier == "exact" else random_stats_data(M, C, dtype)
    ref = ref_stats(d.x, d.gamma, d.beta, d.rm, d.rv, momentum)
    partial = rows
    if partial_nblk is not None:
        assert tier == "exact"
        partial = partition_rows(fwd_terms(d.x), partial_nblk)
    out, sm, si, rm, rv = be.fwd_train(d, momentum, partial)
    if tier == "exact":
        assert stats_sums_are_exact(d.x), what
        var_rel = torch.full_like(ref.var, FP64_NOISE)
    else:
        sb = ROWS_BOUND if partial is not None else sum_bound(reduce_layout(dtype, M, C))
        pm = ref.mean if partial is not None else d.x[0].double() - ref.mean
        var_rel = var_rel_bound(sb, _factor(pm, ref.var))
    fig = check_stats((sm, si, rm, rv), ref, d, M, momentum, var_rel, tier == "exact" and _pow2(M), what)
    dsc, dsh = coef_bounds(ref, d, var_rel)
    fig.update(check_apply_random(out, None, ref_apply(d.x, ref.scale, ref.shift), dtype, what, d.x, dsc, dsh))
    fig["invstd_rel"] = ((_d(si) - ref.invstd).abs() / ref.invstd).max().item()
    return fig


def verify_apply(be, dtype, M, C, tier, addend, relu, bits):
    what = f"{tier} {dtype} M={M} C={C} {addend} relu={relu} bits={bits}"
    d = exact_apply_data(M, C, dtype) if tier == "exact" else random_apply_data(M, C, dtype)
    kw = apply_args(d, addend)
    ref = ref_apply(d.x, d.scale, d.shift, relu=relu, **kw)
    out, b = be.apply(d.x, d.scale, d.shift, relu, bits, **kw)
    assert (b is not None) == bits
    if tier == "exact":
        check_apply_exact(out, b, ref, dtype, relu, what)
        return {}
    return check_apply_random(out, b, ref, dtype, what)


def verify_bwd(be, dtype, C, M, tier, relu, dz_out=False, beta_acc=0.0, alias="none", partial_nblk=None, bits=None):
    """mi355_bn_bwd_bits.  bits: teacher-force on these (bool) instead of the data's"""
    what = f"{tier} {dtype} C={C} M={M} relu={relu} dz_out={dz_out} beta_acc={beta_acc} alias={alias} nblk={partial_nblk}"
    d = exact_bwd_data(M, C, dtype) if tier == "exact" else random_bwd_data(M, C, dtype)
    if bits is not None:
        d = d._replace(bits=bits)
    ref = ref_bwd(d.g, d.bits if relu else None, d.x, d.gamma, d.mean, d.invstd, relu)
    partial = None
    if partial_nblk is not None:
        assert tier == "exact" and relu != 2
        partial = partition_rows(bwd_terms(ref), partial_nblk)
    dx, dz, dg, db = be.bwd(d, relu, dz_out, beta_acc, alias, partial)
    pre = (d.dgamma0, d.dbeta0) if beta_acc else (None, None)
    sb = ROWS_BOUND if partial is not None and not dz_out else sum_bound(reduce_layout(dtype, M, C))
    fig = {}
    if tier == "exact" and relu != 2:
        assert bwd_sums_are_exact(ref), what
        check_sums_exact(dg, db, ref, *pre, what=what)
        if bwd_dx_is_exact(ref, M):
            check_dx_exact(dx, ref, dtype, what)
            fig["dx_exact"] = True
    else:
        fig.update(check_sums_random(dg, db, ref, sb, *pre, what=what))
    fig.update(check_dx_random(dx, ref, M, dtype, sb, relu, dz_out, what))
    assert (dz is not None) == dz_out
    if dz_out:
        fig.update(check_dz(dz, ref, dtype, relu, what))
    return fig


def verify_offset(be, name, path):
    """|mean| >> std through the pivot path (the reduce) or the plain-sum rows; returns the measured relative error of invstd"""
    d = offset_data(name)
    rows = plain_rows(d.x, 13) if path == "plain" else None
    return verify_stats(be, d.x.dtype, OFFSET_C, OFFSET_M, "random", 0.1, data=d, rows=rows, what=f"{name} {path}")["invstd_rel"]


CONST_M, CONST_C = 37, 64


@functools.lru_cache(maxsize=None)
def constant_data(dtype, M):
    """even channels constant (3.75, -100.5, ... : values of both dtypes), odd channels random"""
    d = random_stats_data(M, CONST_C, dtype, seed=81)
    x = d.x.clone()
    x[:, 0::2] = torch.tensor([3.75, -100.5, 0.0, 1024.0]).repeat(CONST_C // 8).to(dtype)
    return d._replace(x=x)


def verify_constant(be, dtype, M, momentum):
    """var = 0 (constant channels; every channel at M = 1): invstd = 1 / sqrt(eps), everything finite, the output is beta up to the rounding of
    shift = beta - mean * scale — mean * scale rounded (U32), the difference (U32 of |shift| <= |mean scale| + |beta|), the apply's fma (U32 of |out|): in all
    3 U32 |mean scale| + 2 U32 |beta|, then the rounding to the dtype — running_var moves toward 0 by the momentum, and the backward stays finite with
    dgamma = 0 exactly (xhat = 0)"""
    what = f"constant {dtype} M={M} momentum={momentum}"
    d = constant_data(dtype, M)
    const = torch.ones(CONST_C, dtype=torch.bool) if M == 1 else torch.arange(CONST_C) % 2 == 0
    ref = ref_stats(d.x, d.gamma, d.beta, d.rm, d.rv, momentum)
    assert (ref.var[const] == 0).all()
    out, sm, si, rm, rv = be.fwd_train(d, momentum, None, relu=0)
    for name, t in (("out", out), ("save_mean", sm), ("save_invstd", si), ("running_mean", rm), ("running_var", rv)):
        assert torch.isfinite(_d(t)).all(), f"{what}: {name} not finite"
    _assert_equal(sm[const], ref.mean[const], f"{what} save_mean")
    _assert_within(si[const], ref.invstd[const], 2 * U32 * ref.invstd[const], f"{what} save_invstd")
    beta = d.beta.double()
    bound = (3 * U32 * (ref.mean * ref.scale).abs() + 2 * U32 * beta.abs()) * (1 + HALF[dtype]) + HALF[dtype] * beta.abs()
    fig = {"out": _assert_within(out[:, const], beta[const].expand(M, -1), bound[const].expand(M, -1) + 1e-300, f"{what} |out - beta|")}
    mom = float(_f32(momentum))
    keep = (1 - mom) * d.rv.double()
    _assert_within(rv[const], keep[const], RUNNING_OPS * U32 * keep[const], f"{what} running_var")
    g = random_bwd_data(M, CONST_C, dtype)
    bd = g._replace(x=d.x, gamma=d.gamma, mean=_d(sm).float(), invstd=_d(si).float())
    dx, _, dg, db = be.bwd(bd, 1)
    for name, t in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        assert torch.isfinite(_d(t)).all(), f"{what}: {name} not finite"
    _assert_equal(dg[const], torch.zeros(int(const.sum()), dtype=torch.float64), f"{what} dgamma of the constant channels")
    return fig


# measured on the CPU (test_bn_host.py::test_offset_data_bounds prints them): the relative error of invstd on the offset data through the restatement
#   pivot path (mi355_bn_fwd_train):              f32_ratio100 1.5e-7   f32_pivot8 1.9e-6   bf16_mean64 3.8e-8 (the sums are exact: invstd's own rounding)
#   plain-sum rows (mi355_bn_fwd_train_partial):  f32_ratio100 1.9e-4   f32_pivot8 2.2e-4   bf16_mean64 3.8e-8 (13 rows of 60 values: exact in fp32)
# 13 correctly rounded rows lose about mean^2 / var * 2^-24 of var, a thousand times what the pivot path loses, and a tenth of their bound
# invstd_rel_bound(var_rel_bound(ROWS_BOUND, (mean^2 + var) / var)) = 2.0e-3 / 1.9e-3 / 5.0e-4.  They document the path; the bound is
# what is asserted.
PLAIN_SUM_LOSS_MEASURED = {"f32_ratio100": 1.912e-4, "f32_pivot8": 2.230e-4, "bf16_mean64": 3.786e-8}
