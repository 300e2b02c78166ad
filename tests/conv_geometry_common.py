"""The case table and the reference of the convolution geometry tests (tests/test_conv_geometry_host.py, tests/test_conv_geometry_gpu.py).

Every other convolution test of the suite runs square maps, square kernels, pad = K // 2 and even extents under stride 2; there a swap of H and W in
one of the library's pixel decodes, a tap table that mixes dh with dw, or an off-by-one that shows only when pad != K // 2 gives the same answer.
The rows below are the small geometries the C ABI accepts (csrc/conv_api.cpp check_conv) where each of these slips changes the result.

Operands are small integers from a seeded CPU generator (x, w, dy in [-2, 2], addends in [-3, 3]): every partial sum is an integer far below 2^24
(the largest magnitude of the whole table is 380), so fp32 sums are exact in any order and the expected values carry no tolerance.  bf16 results
compare against the oracle rounded to bf16 (one rounding of the exact fp32 accumulator, which is what the kernels' epilogues do).
"""
import functools

import torch

from oracle import ops_ref as R

# (N, H, W, Cin, Cout, KH, KW, stride, pad)
CASES = [
    # rectangular, both orientations
    (2, 6, 10, 64, 64, 3, 3, 1, 1),
    (2, 10, 6, 64, 128, 3, 3, 1, 1),
    (5, 5, 13, 64, 256, 3, 3, 1, 1),
    (4, 12, 20, 256, 256, 1, 1, 1, 0),
    # degenerate extents, M far below one row tile
    (1, 1, 1, 64, 64, 3, 3, 1, 1),
    (3, 1, 9, 64, 64, 1, 1, 1, 0),
    (1, 9, 1, 128, 64, 3, 3, 1, 1),
    # stride 2 on odd extents: forward and weight gradient only, the data gradient is refused (build_dgrad_args)
    (2, 7, 5, 64, 64, 3, 3, 2, 1),
    (2, 9, 7, 64, 128, 1, 1, 2, 0),
    # stride 2, even, rectangular; 1x1 and 2x2: output-parity classes of the data gradient without taps
    (2, 8, 12, 128, 64, 3, 3, 2, 1),
    (2, 12, 8, 64, 64, 1, 1, 2, 0),
    (2, 8, 6, 64, 64, 2, 2, 2, 0),
    # pad != K // 2, including outputs larger than the input
    (2, 8, 6, 64, 64, 3, 3, 1, 0),
    (2, 6, 8, 64, 64, 3, 3, 1, 2),
    (2, 8, 10, 64, 64, 3, 3, 2, 0),
    (2, 5, 7, 64, 64, 1, 1, 1, 1),
    # KH != KW
    (2, 6, 9, 64, 64, 1, 3, 1, 1),
    (2, 9, 6, 64, 64, 3, 1, 1, 1),
    (2, 7, 6, 64, 64, 2, 2, 1, 0),
    (1, 5, 11, 64, 64, 1, 7, 1, 3),
    (2, 6, 8, 64, 64, 2, 3, 1, 1),
    # long reduction / wide output on a tiny rectangular map
    (1, 3, 5, 2048, 64, 1, 1, 1, 0),
    (1, 4, 6, 64, 2048, 1, 1, 1, 0),
    # added: a stride-2 1x1 whose data gradient has 128 columns, so that the forced 256 x 128 and 8-wave tiles see three empty parity classes
    (2, 6, 10, 128, 128, 1, 1, 2, 0),
]


def case_id(case):
    N, H, W, Cin, Cout, KH, KW, s, p = case
    return f"{N}x{H}x{W}-c{Cin}-o{Cout}-k{KH}x{KW}-s{s}-p{p}"


def out_dim(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def out_shape(case):
    N, H, W, _, Cout, KH, KW, s, p = case
    return (N, out_dim(H, KH, s, p), out_dim(W, KW, s, p), Cout)


def has_dgrad(case):
    """the data gradient of a stride-2 convolution exists only at even H and W"""
    _, H, W, _, _, _, _, s, _ = case
    return s == 1 or (H % 2 == 0 and W % 2 == 0)


def _ints(gen, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


@functools.lru_cache(maxsize=None)
def operands(case):
    """(x NHWC, w KRSC, dy NHWC, addend NHWC of x's shape) as fp32 CPU tensors of small integers; the same tensors on every call: do not modify"""
    N, H, W, Cin, Cout, KH, KW, _, _ = case
    gen = torch.Generator().manual_seed(1000 + CASES.index(case) if case in CASES else 999)
    x = _ints(gen, -2, 2, (N, H, W, Cin))
    w = _ints(gen, -2, 2, (Cout, KH, KW, Cin))
    dy = _ints(gen, -2, 2, out_shape(case))
    add = _ints(gen, -3, 3, (N, H, W, Cin))
    return x, w, dy, add


@functools.lru_cache(maxsize=None)
def expected(case):
    """(y, dx, dw) of the torch-CPU oracle (oracle/ops_ref.py) for operands(case), fp32; the same tensors on every call: do not modify"""
    x, w, dy, _ = operands(case)
    s, p = case[7], case[8]
    y = R.conv2d_fwd(x, w, s, p)
    dx, dw = R.conv2d_bwd(x, w, dy, s, p)
    return y, dx, dw


def as_dtype(ref, dtype):
    """what a kernel that rounds its exact fp32 accumulator once to `dtype` must store, held as fp32"""
    return ref.to(dtype).float()
