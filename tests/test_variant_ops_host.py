"""The fp64 references of tests/variant_common.py, on the CPU: each agrees with its oracle/ops_ref.py counterpart (fp32 on torch's own kernels) within
1e-6 normalised error on the shapes tests/test_variant_ops_gpu.py walks, the first-maximum max pool agrees exactly with torch's max_pool2d and its
indices, and the inputs discriminate — conditions on the data, not measurements: a kernel with the wrong tie rule, a reversed ECA filter or no
zero padding at the ends of the channel axis moves the reference by far more than the tolerance the GPU file grants."""
import numpy as np
import pytest
import torch

import variant_common as V
from oracle import ops_ref as R

F = torch.nn.functional


def _tap_codes(flat, H, W):
    """torch's flat argmax indices [N][C][H][W] into the plane -> NHWC tap codes a*3 + b of the window centred at the output pixel"""
    h = torch.arange(H).view(1, 1, H, 1)
    w = torch.arange(W).view(1, 1, 1, W)
    a = flat // W - h + 1
    b = flat % W - w + 1
    assert ((a >= 0) & (a < 3) & (b >= 0) & (b < 3)).all()
    return (a * 3 + b).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shape", V.MAXPOOL_POINT + V.MAXPOOL_ROWS)
def test_first_max_reference_is_torchs_max_pool_and_the_tie_data_discriminate(shape):
    N, H, W, C = shape
    x, y, idx = V.tie_case(shape)
    yt, flat = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 1, 1, return_indices=True)
    assert torch.equal(y.float(), yt.permute(0, 2, 3, 1))
    assert torch.equal(y.float(), R.maxpool3s1(x.float()))
    assert torch.equal(idx, _tap_codes(flat, H, W))
    if H * W < 9:   # (the single-column shapes: windows of at most three pixels; the conditions are about the data of the full windows)
        return
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1), value=float("-inf"))
    at_max = sum((xp[:, a:a + H, b:b + W, :] == y.float()).int() for a in range(3) for b in range(3))
    assert (at_max >= 2).float().mean().item() >= 0.30
    _, idx_last = V.maxpool3s1_first_max(x, last=True)
    assert (idx_last != idx).float().mean().item() >= 0.10


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("shape", V.MAXPOOL_POINT + V.MAXPOOL_ROWS[:3])
def test_scatter_reference_is_torchs_max_pool_backward_where_no_ties_exist(shape, dtype):
    """on tie-free data (a ramp over the pixels under the noise) torch routes every gradient to the one maximum; with ties torch's CPU kernel takes the
    first maximum too, which the index test above pins"""
    N, H, W, C = shape
    x = (V.rnd(shape, 22, torch.float32).double() + torch.arange(H * W).view(1, H, W, 1) * 2.5).float()
    dy = V.rnd(shape, 23, dtype)
    y, idx = V.maxpool3s1_first_max(x)
    (ref,) = R.grads(R.maxpool3s1, [x], dy)
    assert V.nerr(V.maxpool3s1_scatter(dy, idx), ref) < 1e-6
    x, _, idx = V.tie_case(shape)
    (ref,) = R.grads(R.maxpool3s1, [x.float()], dy)
    assert V.nerr(V.maxpool3s1_scatter(dy, idx), ref) < 1e-6


@pytest.mark.parametrize("case", V.ECA_CASES)
def test_eca_reference_and_its_data(case):
    N, H, W, C, k = case
    x, w, dy = V.eca_data(case, torch.float32)
    y, pooled, gate = V.eca_ref(x, w)
    assert V.nerr(y, R.eca(x, w)) < 1e-6
    assert V.nerr(pooled, R.gap(x)) < 1e-6
    dx, dw = V.eca_bwd_ref(dy, x, w)
    dx_o, dw_o = R.grads(R.eca, [x, w], dy)
    assert V.nerr(dx, dx_o) < 1e-6
    # the written-out backward against fp64 autograd of the forward that the oracle has just pinned: the formulas themselves
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    V.eca_ref(xd, wd)[0].backward(dy.double())
    assert V.nerr(dx, xd.grad) < 1e-12 and V.nerr(dw, wd.grad) < 1e-12
    # dw[j] is a sum of n = N*C terms t = dpre * pooled, which the oracle forms and adds in fp32: to first order its own error is at most
    # (8 + log2 n) u sum |t| — eight roundings on the way to a term (the pixel sum apart, which dx above covers), log2 n levels of a pairwise sum.
    # Measured over six seeds: 1e-7 .. 1e-6 of max |dw| at n = 768, 1e-6 .. 7e-6 at n >= 131072, so 1e-6 cannot hold for this one quantity.
    dpre = (dy.double() * x.double()).sum(dim=(1, 2)) * gate * (1 - gate)
    sum_abs = (dpre.abs() * V._taps(pooled, k).abs()).sum(dim=(1, 2)).max().item()
    own = (8 + np.log2(N * C)) * 2.0 ** -24 * sum_abs / dw.abs().max().item()
    assert V.nerr(dw, dw_o) < own, (V.nerr(dw, dw_o), own)
    # the data discriminate
    assert pooled.abs().mean().item() > 0.5
    if k > 1:
        assert V.nerr(V.eca_ref(x, w.flip(0))[0], y) > 0.2, "a reversed filter must show at 10 x the bf16 tolerance"
    cut = pooled.clone()
    cut[:, 0] = 0
    cut[:, C - 1] = 0
    e = k // 2 + 1
    assert (V.eca_gate_ref(cut, w)[:, :e] - gate[:, :e]).abs().max().item() > 1e-2, "the first channels must feel their neighbours"


@pytest.mark.parametrize("shape", V.WEIGHT_STD_SHAPES + [V.WEIGHT_STD_CONST])
def test_weight_std_reference(shape):
    w, g = V.weight_std_data(shape)
    w_hat, invstd = V.weight_std_ref(w)
    assert V.nerr(w_hat, R.weight_std(w)) < 1e-6
    (dw_o,) = R.grads(R.weight_std, [w], g)
    assert V.nerr(V.weight_std_bwd_ref(g, w), dw_o) < 1e-6
    if shape == V.WEIGHT_STD_CONST:
        assert w_hat[1].abs().max().item() == 0 and abs(invstd[1].item() * 1e-5 ** 0.5 - 1) < 1e-12
    if w[0].numel() == 1:
        assert w_hat.abs().max().item() == 0


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("form", ["all", "no_shortcut", "no_scale", "neither"])
def test_residual_act_reference_and_its_zeros(form, act, dtype):
    b, s, scale, dout = V.residual_data(dtype)
    s = None if form in ("no_shortcut", "neither") else s
    scale = None if form in ("no_scale", "neither") else scale
    out = V.residual_act_ref(b, scale, s, act)
    assert V.nerr(out, R.residual_act(b, scale, s, act)) < 1e-6
    assert (out == 0).float().mean().item() > 0.02, "exact zeros in front of the activation"
    db, ds = V.residual_act_bwd_ref(dout, out, scale, act)
    fn = (lambda u, v: R.residual_act(u, scale, v, act)) if s is not None else (lambda u: R.residual_act(u, scale, None, act))
    got = R.grads(fn, [b] if s is None else [b, s], dout)
    assert V.nerr(db, got[0]) < 1e-6
    if s is not None:
        assert V.nerr(ds, got[1]) < 1e-6
    for n, sc in enumerate(V.RESIDUAL_SCALE if scale is not None else ()):
        assert torch.equal(db[n], ds[n] * sc)


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("shape", [(2, 8, 8, 64)] + V.POOL_SHAPES)
def test_pool_references(shape, dtype):
    x = V.rnd(shape, 61, dtype)
    for ref, oracle in ((V.blurpool_ref, R.blurpool), (V.avgpool2_ref, R.avgpool2)):
        y = ref(x)
        assert V.nerr(y, oracle(x)) < 1e-6
        dy = V.rnd(tuple(y.shape), 62, dtype)
        (dx_o,) = R.grads(oracle, [x], dy)
        assert V.nerr(V.grad64(ref, x, dy), dx_o) < 1e-6


def test_keep_scale_reference():
    k = V.keep_scale_ref(200000, 0.2, 3, 5)
    assert k.dtype == np.float32 and np.array_equal(k, V.keep_scale_ref(200000, 0.2, 3, 5))
    assert set(np.unique(k).tolist()) == {0.0, 1.25}
    assert abs((k > 0).mean() - 0.8) < 5e-3
    assert not np.array_equal(k, V.keep_scale_ref(200000, 0.2, 3, 6)) and not np.array_equal(k, V.keep_scale_ref(200000, 0.2, 4, 5))
    assert np.array_equal(V.keep_scale_ref(257, 0.0, 3, 5), np.ones(257, np.float32))
    assert np.array_equal(k[:4096], V.keep_scale_ref(4096, 0.2, 3, 5)), "element i depends on i alone"
    # 64-bit wrap-around: Python integers reduced mod 2^64 give the same stream as the uint64 arithmetic
    M = 2 ** 64 - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    n, p, seed, counter = V.KEEP_CASES[3]
    base = sm(seed ^ sm(counter))
    bits = [sm((base + 0x632BE59BD9B4E019 * (i + 1)) & M) >> 40 for i in range(n)]
    keep = np.array([(b + 0.5) / 2 ** 24 >= p for b in bits])   # (in exact arithmetic: no sample of this case sits where float32's rounding of b + 0.5 decides)
    assert np.array_equal(V.keep_scale_ref(n, p, seed, counter) > 0, keep) and 0 < keep.sum() < n
