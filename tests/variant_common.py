"""What tests/test_variant_ops_host.py and tests/test_variant_ops_gpu.py share: plain fp64 references of the small BResNet-50 variant operators
(csrc/variant.hip behind mi355_blurpool_*, mi355_avgpool2_*, mi355_maxpool3s1_*, mi355_eca_*, mi355_weight_std_*, mi355_residual_act_*,
mi355_keep_scale), the shapes both files walk, and the input data.

The references are tensor code on NHWC tensors, fp64 throughout, one statement per line of the operator's definition; the forward passes and the
backward passes of the max pool, ECA and residual_act are written out, the remaining backward passes go through fp64 autograd.  The host file pins
every one of them to its oracle/ops_ref.py counterpart (fp32, torch's own kernels) and checks that the data discriminate: ties in most max-pool
windows, pooled ECA means of order 1 under an asymmetric filter, exact zeros in front of the activation."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

LEAKY = 0.01
DTYPES = [torch.float32, torch.bfloat16]
# normalised max error, as tests/test_ops_gpu.py and tests/test_variant_gpu.py: fp32 2e-5 (1e-4 where a backward sums many terms), bf16 2e-2
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}
TOL_SUM = {torch.float32: 1e-4, torch.bfloat16: 2e-2}

# 3x3 / stride-1 max pool.  The C-ABI takes the row-walking kernels when W >= 16 and N*H*C/8 >= 16384, the point-wise kernels otherwise; the row
# walk cuts a row into segments of min(W, 112) pixels and unrolls by three.
MAXPOOL_POINT = [(2, 5, 7, 64), (1, 1, 1, 64), (2, 9, 15, 64), (1, 3, 1, 8)]
MAXPOOL_ROWS = [
    (32, 64, 16, 64),    # W % 3 == 1
    (32, 64, 18, 64),    # W % 3 == 0: the unrolled loop alone
    (32, 64, 20, 64),    # W % 3 == 2
    (8, 32, 113, 512),   # a second segment of 1 pixel
    (8, 32, 114, 512),   # ... of 2
    (8, 32, 115, 512),   # ... of 3
    (8, 32, 160, 512),   # the stem map of a 320-px image: 112 + 48
]
# (N, H, W, C, k)
ECA_CASES = [(3, 7, 7, 256, k) for k in (1, 3, 5, 7, 9)] + [
    (2, 1, 1, 64, 9),      # one pixel, the smallest C
    (2, 3, 5, 128, 5),     # fewer pixels than the 32 pixel lanes of the reductions
    (2, 6, 6, 2048, 3),
    (72, 1, 1, 2048, 3),   # N*C = 147456: a second round of the gate backward's walk (128 workgroups x 1024 threads)
    (64, 1, 1, 2048, 3),   # N*C = 131072: exactly one round
]
WEIGHT_STD_SHAPES = [(64, 3, 3, 3), (8, 1, 1, 1), (32, 7, 7, 3), (16, 3, 3, 512)]
WEIGHT_STD_CONST = (4, 3, 3, 16)   # row 1 constant
RESIDUAL_SHAPE = (3, 5, 5, 72)     # HWC/8 = 225 (bf16), HWC/4 = 450 (fp32): no multiple of 256, a workgroup straddles images
RESIDUAL_SCALE = (0.0, 1.25, 1.0)
POOL_SHAPES = [(1, 4, 2, 64), (2, 2, 6, 8), (2, 10, 12, 264)]
# (n, p, seed, counter)
KEEP_CASES = [(1, 0.2, 0, 0), (257, 0.0, 3, 5), (200000, 0.2, 3, 5), (4096, 0.9375, 2 ** 63 + 11, 2 ** 40 + 63)]


def nerr(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def rnd(shape, seed, dtype, scale=1.0):
    """uniform in (-scale, scale), rounded to dtype (and kept in it)"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(dtype)


def ints(shape, seed, lo, hi):
    """integers lo .. hi inclusive, int8: exact in fp32 and bf16"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8)


def tie_data(shape):
    """integers 0 .. 3: nine taps over four values, so most windows hold their maximum more than once"""
    return ints(shape, 21, 0, 3)


def eca_data(case, dtype):
    """x = uniform(-1, 1) + offset[c] with offset uniform in (-2, 2): pooled means of order 1, so the gates leave 0.5 and the filter's direction and the
    zero padding at the two ends of the channel axis show in y; w falls from -0.9 to 0.7 (asymmetric) plus noise.  Returns (x, w, dy): x, dy in dtype."""
    N, H, W, C, k = case
    x = (rnd((N, H, W, C), 31, torch.float32).double() + rnd((C,), 32, torch.float32, 2.0).double()).to(dtype)
    w = (torch.linspace(-0.9, 0.7, k) + rnd((k,), 33, torch.float32, 0.05)).float()
    return x, w, rnd((N, H, W, C), 34, dtype)


def weight_std_data(shape):
    w = rnd(shape, 41, torch.float32, 0.3) + 0.05
    if shape == WEIGHT_STD_CONST:
        w[1] = 0.3
    return w, rnd(shape, 42, torch.float32)


def residual_data(dtype):
    """small integers: with the scales 0, 1.25 and 1 per image (or none) the sum in front of the activation is exactly 0 at many places"""
    b = ints(RESIDUAL_SHAPE, 51, -4, 4).to(dtype)
    s = ints(RESIDUAL_SHAPE, 52, -5, 5).to(dtype)
    return b, s, torch.tensor(RESIDUAL_SCALE), rnd(RESIDUAL_SHAPE, 53, dtype)


# ---- 3x3 / stride-1 max pool ----------------------------------------------------------------------------------------------------
def maxpool3s1_first_max(x, last=False):
    """(y, idx): pad with -inf, visit the nine taps in scan order a*3 + b, take a tap on strict > — the FIRST maximum.  idx is the tap's code, uint8.
    last=True is the other rule (the last maximum: >= among real pixels), for the host file's check that the data tell the two apart."""
    x = x.double()
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    best = torch.full_like(x, float("-inf"))
    code = torch.full(x.shape, 4, dtype=torch.uint8)
    for a in range(3):
        for b in range(3):
            v = xp[:, a:a + H, b:b + W, :]
            take = (v >= best) & (v > float("-inf")) if last else v > best
            best = torch.where(take, v, best)
            code[take] = a * 3 + b
    return best, code


def maxpool3s1_scatter(dy, idx):
    """dx[h][w] = sum over the nine taps (a, b) of dy at the window centred at (h + 1 - a, w + 1 - b), where that window exists and names tap a*3 + b"""
    dy = dy.double()
    N, H, W, C = dy.shape
    dyp = F.pad(dy, (0, 0, 1, 1, 1, 1))
    ip = F.pad(idx, (0, 0, 1, 1, 1, 1), value=255)
    dx = torch.zeros_like(dy)
    for a in range(3):
        for b in range(3):
            sl = (slice(None), slice(2 - a, 2 - a + H), slice(2 - b, 2 - b + W))
            dx += torch.where(ip[sl] == a * 3 + b, dyp[sl], 0.0)
    return dx


@functools.lru_cache(maxsize=1)
def tie_case(shape):
    """(x int8, y fp64, idx uint8) of the tie data at one shape — computed once for the dtypes that share it (0 .. 3 are exact in both)"""
    x = tie_data(shape)
    y, idx = maxpool3s1_first_max(x)
    return x, y, idx


# ---- ECA ------------------------------------------------------------------------------------------------------------------------------
def _taps(v, k):
    """[N][C] -> [k][N][C]: tap j holds v[n][c + j - k//2], zero outside the channel axis"""
    C = v.shape[1]
    vp = F.pad(v, (k // 2, k // 2))
    return torch.stack([vp[:, j:j + C] for j in range(k)])


def eca_gate_ref(pooled, w):
    """gate[n][c] = sigmoid(sum_j w[j] * pooled[n][c + j - k//2]): cross-correlation, zero padding"""
    w = w.double()
    return torch.sigmoid((w.view(-1, 1, 1) * _taps(pooled.double(), w.numel())).sum(0))


def eca_ref(x, w):
    """(y, pooled, gate)"""
    x = x.double()
    pooled = x.mean(dim=(1, 2))
    gate = eca_gate_ref(pooled, w)
    return x * gate[:, None, None, :], pooled, gate


def eca_bwd_ref(dy, x, w):
    """(dx, dw): s = sum_hw dy x; dpre = s g (1 - g); dpool[n][c] = sum_j w[j] dpre[n][c - j + k//2] / HW; dw[j] = sum_nc dpre[n][c] pooled[n][c + j - k//2]"""
    dy, x, w = dy.double(), x.double(), w.double()
    k, hw = w.numel(), x.shape[1] * x.shape[2]
    _, pooled, gate = eca_ref(x, w)
    dpre = (dy * x).sum(dim=(1, 2)) * gate * (1 - gate)
    dw = (dpre * _taps(pooled, k)).sum(dim=(1, 2))
    dpool = (w.flip(0).view(-1, 1, 1) * _taps(dpre, k)).sum(0) / hw
    return dy * gate[:, None, None, :] + dpool[:, None, None, :], dw


# ---- weight standardisation -----------------------------------------------------------------------------------------------------
def weight_std_ref(w, eps=1e-5):
    """(w_hat, invstd [Cout]): per output channel (w - mean) / sqrt(var + eps), biased variance"""
    w = w.double()
    flat = w.reshape(w.shape[0], -1)
    mean = flat.mean(1)
    var = ((flat - mean[:, None]) ** 2).mean(1)
    invstd = 1.0 / torch.sqrt(var + eps)
    return ((flat - mean[:, None]) * invstd[:, None]).reshape(w.shape), invstd


def weight_std_bwd_ref(g, w, eps=1e-5):
    wd = w.double().clone().requires_grad_(True)
    weight_std_ref(wd, eps)[0].backward(g.double())
    return wd.grad


# ---- residual + activation ---------------------------------------------------------------------------------------------------------
def _act(v, act):
    return v if act == 0 else torch.where(v > 0, v, v * (LEAKY if act == 2 else 0.0))


def residual_act_ref(branch, scale_n, shortcut, act):
    v = branch.double()
    if scale_n is not None:
        v = v * scale_n.double().view(-1, 1, 1, 1)
    if shortcut is not None:
        v = v + shortcut.double()
    return _act(v, act)


def residual_act_bwd_ref(dout, out, scale_n, act):
    """(dbranch, dshortcut) from the stored output: slope = out > 0 ? 1 : (0 for ReLU, 0.01 for leaky ReLU), 1 everywhere without activation"""
    dout, out = dout.double(), out.double()
    slope = torch.ones_like(out) if act == 0 else torch.where(out > 0, 1.0, LEAKY if act == 2 else 0.0)
    dz = dout * slope
    return (dz if scale_n is None else dz * scale_n.double().view(-1, 1, 1, 1)), dz


# ---- blur pool, 2x2 average pool ------------------------------------------------------------------------------------------------
def blurpool_ref(x):
    """reflect pad 1, [1, 2, 1] x [1, 2, 1] / 16, stride 2"""
    x = x.double()
    N, H, W, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)
    f = (1.0, 2.0, 1.0)
    y = torch.zeros((N, H // 2, W // 2, C), dtype=torch.float64)
    for a in range(3):
        for b in range(3):
            y = y + f[a] * f[b] / 16.0 * xp[:, a:a + H - 1:2, b:b + W - 1:2, :]
    return y


def avgpool2_ref(x):
    x = x.double()
    N, H, W, C = x.shape
    return x.view(N, H // 2, 2, W // 2, 2, C).mean(dim=(2, 4))


def grad64(fn, x, dy):
    """fp64 autograd: the gradient of fn at x under the upstream gradient dy"""
    xd = x.double().clone().requires_grad_(True)
    fn(xd).backward(dy.double())
    return xd.grad


# ---- drop-connect / dropout stream ----------------------------------------------------------------------------------------------
def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def keep_scale_ref(n, p, seed, counter):
    """float32 [n]: 1 / (1 - p) where u_i >= p, else 0; u_i = (top 24 bits of splitmix64(base + 0x632BE59BD9B4E019 (i + 1)) + 0.5) 2^-24 in float32,
    base = splitmix64(seed ^ splitmix64(counter)), all in uint64 with wrap-around"""
    with np.errstate(over="ignore"):
        seed = np.array([seed % 2 ** 64], dtype=np.uint64)
        counter = np.array([counter % 2 ** 64], dtype=np.uint64)
        base = _splitmix64(seed ^ _splitmix64(counter))
        i = np.arange(1, n + 1, dtype=np.uint64)
        bits = _splitmix64(base + np.uint64(0x632BE59BD9B4E019) * i) >> np.uint64(40)
    u = (bits.astype(np.float32) + np.float32(0.5)).astype(np.float32) * np.float32(2.0 ** -24)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    return np.where(u >= np.float32(p), scale, np.float32(0)).astype(np.float32)
