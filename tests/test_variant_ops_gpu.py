"""The small kernels of the BResNet-50 variant (csrc/variant.hip) per op against the fp64 references of tests/variant_common.py, at the shapes and on
the data where they can go wrong: the segmented row walk of the 3x3 / stride-1 max pool and its first-maximum rule on data full of ties (values, argmax
codes byte for byte, and the row-walking form bit-equal to the point-wise one), ECA with pooled means of order 1 under an asymmetric filter at every
kernel width, one pixel, and a gate backward that walks more than one round, the accumulate mode of the two weight gradients, the null-pointer forms of
residual_act with exact zeros in front of the activation, single values of the drop-connect stream, and one launch past the grid cap.

Tolerances, normalised max error as in test_ops_gpu.py / test_variant_gpu.py: fp32 2e-5 (1e-4 where a backward sums many terms), bf16 2e-2; inputs are
rounded to the dtype before both paths.  Every comparison prints its figure before it asserts (pytest -s).

Which assertion catches which slip:
  a wrong column at a segment boundary, a short last segment, W % 3 == 0   the `values` / `argmax codes` equalities at W = 113, 114, 115, 160 and 18, and the
                                                                           bit-equality with image 0 alone (point-wise form)
  a last-maximum rule, another scan order in either form                   `argmax codes` (the host file: a last-maximum rule moves over 10 % of them)
  a reversed ECA filter, no zero padding at c = 0 / C - 1                  eca_gate and eca_y (the host file: 0.2 and 1e-2 of difference in the reference)
  a lost second round / a stale partial row of the gate backward           eca_dw and eca_dx at N*C = 147456, 131072 and 128
  beta ignored, or dw read under beta = 0                                  *_beta1 against twice the gradient, *_beta0 on a NaN-filled dw
  a null-pointer form of residual_act, the slope at 0                      the `form` cases, residual_act_slope_at_0, `db2 == db` without the shortcut gradient
  a changed drop-connect stream                                            the mask equality of test_keep_scale_values
  a wrong stride past the grid cap                                         test_grid_stride_second_trip

Largest normalised error seen on an MI355X (fp32 / bf16; the file takes 10 s), a baseline for tightening:
  blurpool fwd 1.0e-7 / 3.5e-3, bwd 4.7e-8 / 3.0e-3; avgpool2 fwd 6.4e-8 / 3.3e-3, bwd 0 / 0; maxpool3s1 bwd 1.5e-7 / 3.3e-3 (values and codes exact)
  eca pooled 1.3e-7 / 1.0e-7, gate 1.2e-7 / 1.3e-7, y 1.4e-7 / 3.2e-3, dx 1.5e-7 / 3.8e-3, dw 4.9e-7 / 3.2e-7 (beta 1 and beta 0 the same)
  weight_std fwd 1.0e-7, invstd 5.4e-8, bwd 1.4e-7 (fp32 only); residual_act fwd 6.0e-10 / 2.0e-5, dbranch 4.8e-8 / 3.1e-3, dshortcut 4.7e-10 / 2.9e-5
  keep_scale: mask equal, kept value equal to float32 1 / (1 - p) in every case"""
import numpy as np
import pytest
import torch

import variant_common as V
from variant_common import TOL, TOL_SUM, nerr

pytestmark = pytest.mark.gpu
NAME = {torch.float32: "fp32", torch.bfloat16: "bf16"}


def close(what, dtype, got, ref, tol):
    e = nerr(got, ref)
    print(f"variant-op {what} {NAME[dtype]} err {e:.3e} tol {tol:.0e}")
    assert e < tol, f"{what} {NAME[dtype]}: {e:.3e} >= {tol:.0e}"


def _maxpool_tie_case(dev, dtype, shape):
    """forward and backward on the tie data against the first-maximum reference; returns the device tensors (x, dy, y, idx, dx)"""
    from sota_imagenet_amd import ops

    x8, y_ref, idx_ref = V.tie_case(shape)
    x = x8.to(dev).to(dtype)
    y, idx = ops.maxpool3s1_fwd(x)
    assert torch.equal(y.cpu().double(), y_ref), "values"
    assert torch.equal(idx.cpu(), idx_ref), "argmax codes: the first maximum in scan order"
    dy = V.rnd(shape, 24, dtype)
    dyd = dy.to(dev)
    dx = ops.maxpool3s1_bwd(dyd, idx)
    close("maxpool3s1_bwd", dtype, dx, V.maxpool3s1_scatter(dy, idx_ref), TOL[dtype])
    return x, dyd, y, idx, dx


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in V.MAXPOOL_POINT for d in V.DTYPES])
def test_maxpool3s1_point_wise_on_ties(dev, shape, dtype):
    N, H, W, C = shape
    assert N * H * C // 8 < 16384 or W < 16
    _maxpool_tie_case(dev, dtype, shape)


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in V.MAXPOOL_ROWS for d in V.DTYPES])
def test_maxpool3s1_row_walk_on_ties_and_bit_equal_to_the_point_wise_form(dev, shape, dtype):
    """the whole batch takes the row-walking kernels (W >= 16, N*H*C/8 >= 16384: the smallest launches that do), image 0 alone the point-wise ones:
    same values, same codes, same gradient, bit for bit"""
    from sota_imagenet_amd import ops

    N, H, W, C = shape
    assert W >= 16 and N * H * C // 8 >= 16384 and H * C // 8 < 16384
    x, dy, y, idx, dx = _maxpool_tie_case(dev, dtype, shape)
    y0, idx0 = ops.maxpool3s1_fwd(x[:1].contiguous())
    assert torch.equal(y0, y[:1]) and torch.equal(idx0, idx[:1])
    assert torch.equal(ops.maxpool3s1_bwd(dy[:1].contiguous(), idx0), dx[:1])


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("case", V.ECA_CASES)
def test_eca(dev, case, dtype):
    from sota_imagenet_amd import ops

    N, H, W, C, k = case
    x, w, dy = V.eca_data(case, dtype)
    y_ref, pooled_ref, gate_ref = V.eca_ref(x, w)
    dx_ref, dw_ref = V.eca_bwd_ref(dy, x, w)
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    y, pooled, gate = ops.eca_fwd(xd, wd)
    close(f"eca_pooled[{N}x{H}x{W}x{C},k{k}]", dtype, pooled, pooled_ref, 2e-5)   # fp32 arrays formed from the already-rounded input: 2e-5 in both dtypes
    close(f"eca_gate[{N}x{H}x{W}x{C},k{k}]", dtype, gate, gate_ref, 2e-5)
    close(f"eca_y[{N}x{H}x{W}x{C},k{k}]", dtype, y, y_ref, TOL[dtype])
    dx, dw = ops.eca_bwd(dyd, xd, wd, pooled, gate)
    close(f"eca_dx[{N}x{H}x{W}x{C},k{k}]", dtype, dx, dx_ref, TOL_SUM[dtype])
    close(f"eca_dw[{N}x{H}x{W}x{C},k{k}]", dtype, dw, dw_ref, TOL_SUM[dtype])
    # accumulate mode: beta = 1 adds to what dw holds, beta = 0 never reads it
    acc = torch.zeros(k, device=dev)
    for _ in range(2):
        _, out = ops.eca_bwd(dyd, xd, wd, pooled, gate, dw=acc, beta=1.0)
        assert out is acc
    close(f"eca_dw_beta1[{N}x{H}x{W}x{C},k{k}]", dtype, acc, 2 * dw_ref, TOL_SUM[dtype])
    nan = torch.full((k,), float("nan"), device=dev)
    ops.eca_bwd(dyd, xd, wd, pooled, gate, dw=nan, beta=0.0)
    close(f"eca_dw_beta0[{N}x{H}x{W}x{C},k{k}]", dtype, nan, dw_ref, TOL_SUM[dtype])
    assert torch.equal(nan, dw)


@pytest.mark.parametrize("shape", V.WEIGHT_STD_SHAPES + [V.WEIGHT_STD_CONST])
def test_weight_std(dev, shape):
    from sota_imagenet_amd import ops

    f32 = torch.float32
    w, g = V.weight_std_data(shape)
    w_hat_ref, invstd_ref = V.weight_std_ref(w)
    dw_ref = V.weight_std_bwd_ref(g, w)
    w_hat, invstd = ops.weight_std_fwd(w.to(dev))
    tag = "x".join(map(str, shape))
    close(f"weight_std_fwd[{tag}]", f32, w_hat, w_hat_ref, 2e-5)
    close(f"weight_std_invstd[{tag}]", f32, invstd, invstd_ref, 2e-5)
    if shape == V.WEIGHT_STD_CONST:   # a constant row: no variance, w_hat = 0 and invstd = 1 / sqrt(eps)
        assert w_hat[1].abs().max().item() == 0.0
        assert abs(invstd[1].item() * 1e-5 ** 0.5 - 1.0) < 2e-5
    gd = g.to(dev)
    dw = ops.weight_std_bwd(gd, w_hat, invstd)
    close(f"weight_std_bwd[{tag}]", f32, dw, dw_ref, 1e-4)
    acc = torch.zeros(shape, device=dev)
    for _ in range(2):
        assert ops.weight_std_bwd(gd, w_hat, invstd, dw=acc, beta=1.0) is acc
    close(f"weight_std_bwd_beta1[{tag}]", f32, acc, 2 * dw_ref, 1e-4)
    nan = torch.full(shape, float("nan"), device=dev)
    ops.weight_std_bwd(gd, w_hat, invstd, dw=nan, beta=0.0)
    close(f"weight_std_bwd_beta0[{tag}]", f32, nan, dw_ref, 1e-4)
    assert torch.equal(nan, dw)


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("form", ["all", "no_shortcut", "no_scale", "neither"])
def test_residual_act_call_forms(dev, form, act, dtype):
    """every null-pointer form of the two entry points, on small integers: exact zeros in front of the activation, where the backward's slope is
    `out > 0 ? 1 : slope` — 0 for ReLU, 0.01 for leaky ReLU"""
    from sota_imagenet_amd import ops

    b, s, scale, dout = V.residual_data(dtype)
    s = None if form in ("no_shortcut", "neither") else s
    scale = None if form in ("no_scale", "neither") else scale
    on = lambda t: None if t is None else t.to(dev)
    out_ref = V.residual_act_ref(b, scale, s, act)
    out = ops.residual_act_fwd(b.to(dev), on(s), on(scale), act)
    close(f"residual_act_fwd[{form},act{act}]", dtype, out, out_ref, TOL[dtype])
    zero = out_ref == 0
    assert zero.any() and torch.equal(out.cpu() == 0, zero)
    stored = out_ref.to(dtype)   # what the forward leaves for the backward, rounded to the dtype before both paths
    db_ref, ds_ref = V.residual_act_bwd_ref(dout, stored, scale, act)
    db, ds = ops.residual_act_bwd(dout.to(dev), stored.to(dev), on(scale), act, want_shortcut=True)
    close(f"residual_act_dbranch[{form},act{act}]", dtype, db, db_ref, TOL[dtype])
    close(f"residual_act_dshortcut[{form},act{act}]", dtype, ds, ds_ref, TOL[dtype])
    close(f"residual_act_slope_at_0[{form},act{act}]", dtype, ds.cpu()[zero], ds_ref[zero], TOL[dtype])
    if act == 1:
        assert ds.cpu()[zero].abs().max().item() == 0.0
    db2, none = ops.residual_act_bwd(dout.to(dev), stored.to(dev), on(scale), act, want_shortcut=False)
    assert none is None and torch.equal(db2, db)


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("shape", V.POOL_SHAPES)
def test_blurpool_and_avgpool2_at_the_small_and_rectangular_shapes(dev, shape, dtype):
    from sota_imagenet_amd import ops

    x = V.rnd(shape, 61, dtype)
    tag = "x".join(map(str, shape))
    for name, fwd, bwd, ref in (("blurpool", ops.blurpool_fwd, ops.blurpool_bwd, V.blurpool_ref), ("avgpool2", ops.avgpool2_fwd, ops.avgpool2_bwd, V.avgpool2_ref)):
        y_ref = ref(x)
        dy = V.rnd(tuple(y_ref.shape), 62, dtype)
        close(f"{name}_fwd[{tag}]", dtype, fwd(x.to(dev)), y_ref, TOL[dtype])
        close(f"{name}_bwd[{tag}]", dtype, bwd(dy.to(dev), shape), V.grad64(ref, x, dy), TOL[dtype])


@pytest.mark.parametrize("n,p,seed,counter", V.KEEP_CASES)
def test_keep_scale_values(dev, n, p, seed, counter):
    """the drop-connect / dropout stream is a pure integer function of (seed, counter, i): the mask equals the numpy restatement element for
    element (a resumed run replays it), the kept value is float32 1 / (1 - p) to 1 ulp"""
    from sota_imagenet_amd import ops

    ref = V.keep_scale_ref(n, p, seed, counter)
    k = ops.keep_scale(n, p, seed, counter, dev).cpu().numpy()
    assert k.shape == ref.shape and np.array_equal(k > 0, ref > 0)
    assert np.all(k[ref == 0] == 0)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    if (ref > 0).any():
        rel = np.abs(k[ref > 0].astype(np.float64) / np.float64(scale) - 1).max()
        print(f"variant-op keep_scale[{n},{p}] fp32 err {rel:.3e} tol 1.2e-07")
        assert rel <= 1.2e-7
    if p == 0.0:
        assert np.all(k == 1.0)


def test_grid_stride_second_trip(dev):
    """the elementwise kernels launch at most 65536 workgroups of 256 threads and loop: dx of the 2x2 average pool's backward at 1 x 4096 x 2064 x 8
    fp32 has 16.9 M vectors, above 65536 * 256 = 16.78 M, so its last vectors come from a second trip of that loop (one macro for all of them).
    Small integers: dx = dy / 4 at the pixel's 2x2 block, exactly."""
    from sota_imagenet_amd import ops

    shape = (1, 4096, 2064, 8)
    assert shape[1] * shape[2] * shape[3] // 4 > 65536 * 256
    dy = V.ints((1, 2048, 1032, 8), 71, -8, 8).float()
    dx = ops.avgpool2_bwd(dy.to(dev), shape).cpu()
    ref = (dy * 0.25).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert dx.shape == ref.shape and torch.equal(dx, ref)
