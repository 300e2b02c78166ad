"""The case table of tests/conv_geometry_common.py, checked on the CPU: the geometry is legal, the oracle's fp32 results are exact (so the GPU
tests compare bit for bit), and the integer data actually tells H from W and dh from dw — a table on which a swap gives the same answer would
pin nothing."""
import pytest
import torch
import torch.nn.functional as F

from conv_geometry_common import CASES, case_id, expected, has_dgrad, operands, out_shape
from oracle import naive_ref as NV
from oracle import ops_ref as R


def _conv64(x, w, dy, s, p):
    """the oracle's call form (oracle/ops_ref.py conv2d_fwd / conv2d_bwd) evaluated in fp64"""
    xn = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wn = w.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.conv2d(xn, wn, stride=s, padding=p)
    y.backward(dy.double().permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1), xn.grad.permute(0, 2, 3, 1), wn.grad.permute(0, 2, 3, 1)


def _tap_conv(x, w, s, p, Ho, Wo, swap_taps=False):
    """y[n, i, j] = sum over taps (kh, kw) of w[:, kh, kw] . x[n, i*s + dh, j*s + dw], zero outside the image, with (dh, dw) = (kh - p, kw - p) —
    or, swap_taps, (kw - p, kh - p): the tap table of a builder that mixes the two offsets"""
    N, H, W, C = x.shape
    Cout, KH, KW, _ = w.shape
    B = max(KH, KW) + p + s * max(Ho, Wo)  # border wide enough for every read
    xp = F.pad(x, (0, 0, B, B, B, B))
    y = torch.zeros(N, Ho, Wo, Cout)
    for kh in range(KH):
        for kw in range(KW):
            dh, dw = (kw - p, kh - p) if swap_taps else (kh - p, kw - p)
            win = xp[:, B + dh: B + dh + s * Ho: s, B + dw: B + dw + s * Wo: s]
            y += win @ w[:, kh, kw].t()
    return y


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_output_extents_are_positive_and_the_oracle_is_exact(case):
    N, H, W, Cin, Cout, KH, KW, s, p = case
    assert Cin % 64 == 0 and Cout % 64 == 0 and 1 <= KH * KW <= 9 and s in (1, 2)   # csrc/conv_api.cpp check_conv
    _, Ho, Wo, _ = out_shape(case)
    assert Ho >= 1 and Wo >= 1
    x, w, dy, add = operands(case)
    assert x.abs().max() <= 2 and w.abs().max() <= 2 and dy.abs().max() <= 2 and add.abs().max() <= 3
    y, dx, dw = expected(case)
    assert tuple(y.shape) == out_shape(case) and dx.shape == x.shape and dw.shape == w.shape
    y64, dx64, dw64 = _conv64(x, w, dy, s, p)
    # exact in fp32: equal to the fp64 evaluation bit for bit, so no summation order can change a value
    assert torch.equal(y.double(), y64) and torch.equal(dx.double(), dx64) and torch.equal(dw.double(), dw64)
    assert max(y.abs().max(), dx.abs().max(), dw.abs().max()) < 2 ** 24
    if has_dgrad(case):
        assert torch.equal((dx + add).double(), dx64 + add.double())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_data_tells_h_from_w_and_dh_from_dw(case):
    N, H, W, Cin, Cout, KH, KW, s, p = case
    x, w, _, _ = operands(case)
    y, _, _ = expected(case)
    _, Ho, Wo, _ = out_shape(case)
    assert torch.equal(_tap_conv(x, w, s, p, Ho, Wo), y)   # the tap form restates the oracle
    # (the 1 x 1 map is its own transpose; a 1x1 / stride 1 / pad 0 convolution maps flat pixel m to flat pixel m whatever the extents are called:
    #  those four rows are in the table for their pixel counts and channel counts, and only the half-resolution addend of 3c can tell H from W there)
    if H != W and (KH, KW, s, p) != (1, 1, 1, 0):
        ys = R.conv2d_fwd(x.reshape(N, W, H, Cin), w, s, p)   # the same memory read with H and W exchanged
        assert ys.numel() != y.numel() or not torch.equal(ys.reshape(-1), y.reshape(-1))
    if KH != KW:
        assert not torch.equal(_tap_conv(x, w, s, p, Ho, Wo, swap_taps=True), y)
        yk = R.conv2d_fwd(x, w.reshape(Cout, KW, KH, Cin), s, p)   # the same weights read with the kernel's two axes exchanged
        assert yk.numel() != y.numel() or not torch.equal(yk.reshape(-1), y.reshape(-1))
    for q in (p - 1, p + 1):  # an off-by-one in the padding shows
        assert not torch.equal(_tap_conv(x, w, s, q, Ho, Wo), y)


NAIVE = [(1, 1, 1, 64, 64, 3, 3, 1, 1), (2, 7, 5, 64, 64, 3, 3, 2, 1), (2, 6, 8, 64, 64, 2, 3, 1, 1), (2, 5, 7, 64, 64, 1, 1, 1, 1)]


@pytest.mark.parametrize("case", NAIVE, ids=case_id)
def test_oracle_against_the_naive_window_scan(case):
    """oracle/naive_ref.py's fp64 loops (the second statement of the convolution, tests/test_oracle_naive.py) at rows where the kernel is not
    square, the padding is not K // 2, the extents are odd under stride 2, or the map is a single pixel: equal, not close"""
    assert case in CASES
    x, w, dy, _ = operands(case)
    s, p = case[7], case[8]
    y, dx, dw = expected(case)
    assert torch.equal(y.double(), torch.from_numpy(NV.conv2d_fwd(x.numpy(), w.numpy(), s, p)))
    ndx, ndw = NV.conv2d_bwd(x.numpy(), w.numpy(), dy.numpy(), s, p)
    assert torch.equal(dx.double(), torch.from_numpy(ndx)) and torch.equal(dw.double(), torch.from_numpy(ndw))
