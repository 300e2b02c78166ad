"""The conv entry points of the C ABI on rectangular, odd and off-centre geometry (the table of tests/conv_geometry_common.py), exact on integer
data against the torch-CPU oracle, with every output fenced: the launch writes into a 256-byte aligned view inside a larger NaN-filled tensor,
and afterwards the guards are the same bits, no NaN is left in the view, and the view equals the oracle.

Which kernel served which row (asserted below; "tile" = csrc/conv_igemm.hip igemm<dtype,BM,BN,stages>):
  default rule, fp32        every forward / data gradient: igemm<f32,128,64,2>; weight gradients: wgrad<f32,...> (table WGRAD_TILE)
  default rule, bf16        igemm<bf16,128,64,2>, except the 1x1 / stride 1 / pad 0 rows, which the resident-weight pointwise kernels take
                            (table PO_DEFAULT): 4x12x20 256->256, 3x1x9 64->64, the data gradient of 1x3x5 2048->64, the forward of 1x4x6 64->2048
  forced tiles, bf16        table FORCED: 256 x 256 and 256 x 128 (MI355_IGEMM_BIG=1 / 3) and the 8-wave kernel (MI355_IGEMM8) each served the
                            rectangular rows 5x5x13, 4x12x20, 1x4x6 (forward) and 4x12x20, 1x3x5 (data gradient); with 128 columns the 8-wave
                            224 x 128 / 256 x 128 tiles and the 256 x 128 tile served 2x10x6, 2x9x7 and both stride-2 data gradients
  generated kernels         section c: po (half-resolution, plain and masked addend), pk, pw, wg1 at H != W; dconv / wg3 refuse 7 x 28

Random data (section d), normalised max error max|got - ref| / max|ref| measured on the MI355X (tolerances: fp32 2e-5, bf16 2e-2 as in
tests/test_ops_gpu.py):
  row                          dtype   forward    dgrad      dgrad+addend  wgrad
  2x6x10  64->64  3x3 s1 p1    fp32    1.07e-06   7.32e-07   5.80e-07      0.00e+00
                               bf16    2.65e-03   2.72e-03   2.11e-03      1.20e-07
  2x8x12  128->64 3x3 s2 p1    fp32    1.32e-06   5.04e-07   3.64e-07      0.00e+00
                               bf16    1.97e-03   2.05e-03   2.92e-03      9.72e-08
  2x6x8   64->64  2x3 s1 p1    fp32    7.81e-07   5.31e-07   3.98e-07      0.00e+00
                               bf16    3.31e-03   2.65e-03   2.16e-03      1.46e-07
(the fp32 weight gradient came out bit-identical to the oracle's at these three rows: at most 120 products per element)
"""
import math
import re

import pytest
import torch

from conv_geometry_common import CASES, as_dtype, case_id, expected, has_dgrad, operands, out_dim, out_shape
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
GUARD = 4096  # elements on either side of a fenced view


# ---- fenced outputs ---------------------------------------------------------------------------------------------------------------------
class Fenced:
    """a `shape` view whose first byte is 256-byte aligned, inside one tensor with >= GUARD elements on either side, everything NaN"""

    def __init__(self, shape, dtype, dev):
        n = math.prod(shape)
        es = torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + n + GUARD + 256 // es,), float("nan"), dtype=dtype, device=dev)
        off = GUARD
        off += ((-(self.buf.data_ptr() + off * es)) % 256) // es
        self.off, self.n = off, n
        self.view = self.buf[off:off + n].view(shape)
        assert self.view.data_ptr() % 256 == 0 and off >= GUARD and self.buf.numel() - off - n >= GUARD
        self.snap = None

    def _bits(self):
        return self.buf.view(torch.int32 if self.buf.element_size() == 4 else torch.int16)

    def arm(self):
        torch.cuda.synchronize()
        self.snap = self._bits().clone()
        return self

    def guards_intact(self):
        b = self._bits()
        return torch.equal(b[:self.off], self.snap[:self.off]) and torch.equal(b[self.off + self.n:], self.snap[self.off + self.n:])

    def untouched(self):
        return torch.equal(self._bits(), self.snap)

    def check(self, ref, what):
        """guards the same bits, no NaN in the view, the view equal to ref (fp32 CPU)"""
        torch.cuda.synchronize()
        assert self.guards_intact(), f"{what}: a guard element changed"
        got = self.view.float().cpu()
        assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} output elements were not written"
        assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} of {ref.numel()} elements differ, max |diff| {(got - ref).abs().max().item()}"


# ---- launches through the C ABI, the test owning every buffer -------------------------------------------------------------------------------
def _L():
    from sota_imagenet_amd import native

    return native.lib()


def _ws(case, dtype, dev):
    from sota_imagenet_amd.native import dtype_code

    n = _L().mi355_conv2d_workspace_bytes(dtype_code(dtype), *case)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def fwd(case, x, w, y):
    from sota_imagenet_amd.native import check, cur_stream, dtype_code, ptr

    check(_L().mi355_conv2d_fwd(dtype_code(x.dtype), ptr(x), ptr(w), ptr(y), *case, cur_stream()))


def dgrad(case, dy, w, dx, addend, ws, ws_bytes):
    from sota_imagenet_amd.native import check, cur_stream, dtype_code, ptr

    check(_L().mi355_conv2d_dgrad(dtype_code(dy.dtype), ptr(dy), ptr(w), ptr(dx), ptr(addend), *case, ptr(ws), ws_bytes, cur_stream()))


def wgrad(case, dy, x, dw, beta, ws, ws_bytes):
    from sota_imagenet_amd.native import check, cur_stream, dtype_code, ptr

    check(_L().mi355_conv2d_wgrad(dtype_code(dy.dtype), ptr(dy), ptr(x), ptr(dw), beta, *case, ptr(ws), ws_bytes, cur_stream()))


def last_kernel():
    from sota_imagenet_amd import ops

    return ops.last_conv_kernel()


def _dev_operands(case, dtype, dev):
    return tuple(t.to(dev, dtype).contiguous() for t in operands(case))


# ---- 3a: exact results, outputs fenced ------------------------------------------------------------------------------------------------------
# the 1x1 / stride 1 / pad 0 launches the resident-weight pointwise kernels take under the default rule in bf16: (row, launch) -> kernel
# (launch 0 forward, 1 data gradient, 2 data gradient + addend)
PO_DEFAULT = {
    ((4, 12, 20, 256, 256, 1, 1, 1, 0), 0): "po_k256_b256_s0_a0", ((4, 12, 20, 256, 256, 1, 1, 1, 0), 1): "po_k256_b256_s0_a0",
    ((4, 12, 20, 256, 256, 1, 1, 1, 0), 2): "po_k256_b256_s0_a1",
    ((3, 1, 9, 64, 64, 1, 1, 1, 0), 0): "po_k64_b64_s0_a0", ((3, 1, 9, 64, 64, 1, 1, 1, 0), 1): "po_k64_b64_s0_a0",
    ((3, 1, 9, 64, 64, 1, 1, 1, 0), 2): "po_k64_b64_s0_a1",
    ((1, 3, 5, 2048, 64, 1, 1, 1, 0), 1): "po_k64_b256_s0_a0", ((1, 3, 5, 2048, 64, 1, 1, 1, 0), 2): "po_k64_b256_s0_a1",
    ((1, 4, 6, 64, 2048, 1, 1, 1, 0), 0): "po_k64_b256_s0_a0",
}


def _default_kernel(case, dtype, launch):
    if dtype == torch.bfloat16 and (case, launch) in PO_DEFAULT:
        return PO_DEFAULT[(case, launch)]
    return "igemm<%s,128,64,2>" % ("f32" if dtype == torch.float32 else "bf16")  # every launch here is far below one round of 128-row tiles


def WGRAD_TILE(case, dtype):
    """csrc/conv_wgrad.hip launch_d: 128-channel tiles where the channel count allows, else 64 x 64 with 4 or 3 taps per item"""
    _, _, _, Cin, Cout, KH, KW, _, _ = case
    bm, bn, taps = (128 if Cout % 128 == 0 else 64), (128 if Cin % 128 == 0 else 64), KH * KW
    tpi = 1 if (bm, bn) != (64, 64) else (4 if taps % 4 == 0 else (3 if taps % 3 == 0 else 1))
    return "wgrad<%s,%d,%d,%d>" % ("f32" if dtype == torch.float32 else "bf16", bm, bn, tpi)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_entry_point_is_exact_and_writes_its_output_only(dev, case, dtype):
    N, H, W, Cin, Cout, KH, KW, s, p = case
    x, w, dy, add = _dev_operands(case, dtype, dev)
    y_ref, dx_ref, dw_ref = expected(case)
    add_ref = operands(case)[3]
    ws, ws_bytes = _ws(case, dtype, dev)

    y = Fenced(out_shape(case), dtype, dev).arm()
    fwd(case, x, w, y.view)
    assert last_kernel() == _default_kernel(case, dtype, 0), last_kernel()
    y.check(as_dtype(y_ref, dtype), "forward")

    if has_dgrad(case):
        dx = Fenced((N, H, W, Cin), dtype, dev).arm()
        dgrad(case, dy, w, dx.view, None, ws, ws_bytes)
        assert last_kernel() == _default_kernel(case, dtype, 1), last_kernel()
        dx.check(as_dtype(dx_ref, dtype), "data gradient")
        dxa = Fenced((N, H, W, Cin), dtype, dev).arm()
        dgrad(case, dy, w, dxa.view, add, ws, ws_bytes)
        assert last_kernel() == _default_kernel(case, dtype, 2), last_kernel()
        dxa.check(as_dtype(dx_ref + add_ref, dtype), "data gradient + addend")

    dw = Fenced((Cout, KH, KW, Cin), torch.float32, dev).arm()
    wgrad(case, dy, x, dw.view, 0.0, ws, ws_bytes)   # beta = 0 over NaN: must overwrite, not scale
    assert last_kernel() == WGRAD_TILE(case, dtype), last_kernel()
    dw.check(dw_ref, "weight gradient, beta 0")
    g = torch.Generator().manual_seed(77)
    preset = (2 * torch.randint(-3, 4, tuple(dw_ref.shape), generator=g)).float()   # even integers: half of them is exact
    for beta in (1.0, 0.5):
        dwb = Fenced((Cout, KH, KW, Cin), torch.float32, dev)
        dwb.view.copy_(preset.to(dev))
        dwb.arm()
        wgrad(case, dy, x, dwb.view, beta, ws, ws_bytes)
        dwb.check(dw_ref + beta * preset, f"weight gradient, beta {beta}")


# ---- 3b: every tile family sees the table ---------------------------------------------------------------------------------------------------
KNOBS = [("MI355_IGEMM_BIG", "1"), ("MI355_IGEMM_BIG", "3"), ("MI355_IGEMM8", "224x128"), ("MI355_IGEMM8", "256x256"), ("MI355_IGEMM8", "256x128f")]
T64, T256, T3 = "igemm<bf16,128,64,2>", "igemm<bf16,256,256,2>", "igemm<bf16,256,128,3>"
E224, E256, EFAT = "igemm8<224,128>", "igemm8<256,256>", "igemm8<256,128,fat>"
# the kernel that ran, per knob in the order of KNOBS.  A forced tile that is not legal for a launch falls back to the default rule (T64 here):
# 256-column tiles at 128 columns; the 8-wave kernel at sub-grid rows of one pixel (igemm8_legal: Wsub < 2).
COLS256 = [T256, T3, E224, E256, EFAT]
COLS128 = [T64, T3, E224, T64, EFAT]
FORCED = [
    # (row, launch: 0 forward (columns = Cout) / 1 data gradient (columns = Cin), kernels)
    ((2, 10, 6, 64, 128, 3, 3, 1, 1), 0, COLS128),
    ((5, 5, 13, 64, 256, 3, 3, 1, 1), 0, COLS256),
    ((4, 12, 20, 256, 256, 1, 1, 1, 0), 0, COLS256),
    ((2, 9, 7, 64, 128, 1, 1, 2, 0), 0, COLS128),          # stride 2 on odd extents
    ((1, 4, 6, 64, 2048, 1, 1, 1, 0), 0, COLS256),         # 24 pixels into 8 / 16 column tiles
    ((2, 6, 10, 128, 128, 1, 1, 2, 0), 0, COLS128),
    ((4, 12, 20, 256, 256, 1, 1, 1, 0), 1, COLS256),
    ((1, 9, 1, 128, 64, 3, 3, 1, 1), 1, [T64, T3, T64, T64, T64]),   # one pixel per row: not the 8-wave kernel's
    ((2, 8, 12, 128, 64, 3, 3, 2, 1), 1, COLS128),         # four parity classes of 4, 2, 2, 1 taps
    ((1, 3, 5, 2048, 64, 1, 1, 1, 0), 1, COLS256),
    ((2, 6, 10, 128, 128, 1, 1, 2, 0), 1, COLS128),        # four parity classes, three of them without taps
]


def test_forced_table_covers_every_row_with_128_output_columns():
    assert {c for c, l, _ in FORCED if l == 0} == {c for c in CASES if c[4] % 128 == 0}
    assert {c for c, l, _ in FORCED if l == 1} == {c for c in CASES if c[3] % 128 == 0 and has_dgrad(c)}
    ran = {k for _, _, ks in FORCED for k in ks}
    assert {T64, T256, T3, E224, E256, EFAT} <= ran
    rect = [ks for c, _, ks in FORCED if c[1] != c[2]]
    for fam in (T64, T256, T3, E224, E256, EFAT):   # each family served a rectangular row
        assert any(fam in ks for ks in rect), fam


@pytest.mark.parametrize("knob", range(len(KNOBS)), ids=["%s=%s" % k for k in KNOBS])
@pytest.mark.parametrize("row", FORCED, ids=lambda r: case_id(r[0]) + ("-dgrad" if r[1] else "-fwd"))
def test_forced_tiles_are_exact_on_the_table(dev, row, knob, monkeypatch):
    case, launch, kernels = row
    N, H, W, Cin, Cout, KH, KW, s, p = case
    dtype = torch.bfloat16
    x, w, dy, add = _dev_operands(case, dtype, dev)
    y_ref, dx_ref, _ = expected(case)
    monkeypatch.setenv(*KNOBS[knob])
    if launch == 0:
        y = Fenced(out_shape(case), dtype, dev).arm()
        fwd(case, x, w, y.view)
        assert last_kernel() == kernels[knob], last_kernel()
        y.check(as_dtype(y_ref, dtype), "forward")
    else:
        ws, ws_bytes = _ws(case, dtype, dev)
        dx = Fenced((N, H, W, Cin), dtype, dev).arm()
        dgrad(case, dy, w, dx.view, add, ws, ws_bytes)
        assert last_kernel() == kernels[knob], last_kernel()
        dx.check(as_dtype(dx_ref + operands(case)[3], dtype), "data gradient + addend")


# ---- 3c: the generated pointwise kernels on rectangular maps --------------------------------------------------------------------------------
def _pack_bits(mask):
    """bool [..., C] -> uint8 [..., C / 8]: bit e of byte j = channel 8j + e (tests/test_dconv_gpu.py)"""
    m = mask.reshape(*mask.shape[:-1], -1, 8).to(torch.int32)
    return (m << torch.arange(8, device=mask.device, dtype=torch.int32)).sum(-1).to(torch.uint8)


def _unpack_bits(bits, C):
    return ((bits.reshape(-1, C // 8, 1).to(torch.int32) >> torch.arange(8, device=bits.device, dtype=torch.int32)) & 1).reshape(-1, C)


def _po_dgrad(dev, N, H, W, Cx, Cy, add, sums, seed):
    """conv1's data gradient as the executor launches it (mi355_conv2d_dgrad_bn) on integer data: returns (kernel name, dx, partial rows, the
    fp32 reference of dx rounded to bf16 [pixels, Cx], the fp64 BN-backward sums or None).  add: 0 none, 1 plain, 2 under ReLU bits, 3 the
    half-resolution tensor"""
    from sota_imagenet_amd import ops

    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g)
    dy = ri(-2, 2, (N, H, W, Cy)).to(dev, torch.bfloat16)
    w = ri(-2, 2, (Cy, 1, 1, Cx)).to(dev, torch.bfloat16)
    ad = abits = None
    ref = dy.float().reshape(-1, Cy) @ w.float().reshape(Cy, Cx)
    if add == 3:
        ad = ri(-3, 3, (N, H // 2, W // 2, Cx)).to(dev, torch.bfloat16)
        full = torch.zeros((N, H, W, Cx), device=dev)
        full[:, ::2, ::2] = ad.float()
        ref = ref + full.reshape(-1, Cx)
    elif add:
        ad = ri(-3, 3, (N, H, W, Cx)).to(dev, torch.bfloat16)
        a = ad.float().reshape(-1, Cx)
        if add == 2:
            abits = ri(0, 255, (N, H, W, Cx // 8)).to(dev, torch.uint8)
            a = a * _unpack_bits(abits, Cx)
        ref = ref + a
    ref = ref.to(torch.bfloat16)
    kw, want = {}, None
    if sums:
        y = ri(-3, 3, (N, H, W, Cx)).to(dev, torch.bfloat16)
        ybits = ri(0, 255, (N, H, W, Cx // 8)).to(dev, torch.uint8)
        mean, invstd = (ri(-4, 4, (Cx,)) * 0.25).float().to(dev), (ri(1, 4, (Cx,)) * 0.5).float().to(dev)
        kw = dict(bn_y=y, bn_bits=ybits, bn_mean=mean, bn_invstd=invstd)
        dz = ref.double() * _unpack_bits(ybits, Cx)
        xhat = (y.double().reshape(-1, Cx) - mean.double()) * invstd.double()
        want = (dz.sum(0), (dz * xhat).sum(0))
    dx, part = ops.conv2d_dgrad_bn(dy, w, (N, H, W, Cx), 1, 0, addend=ad, addend_bits=abits, addend_sub2=(add == 3), **kw)
    return ops.last_conv_kernel(), dx, part, ref, want


def _check_po(dx, part, ref, want, Cx):
    assert not torch.isnan(dx.float()).any()
    assert torch.equal(dx.reshape(-1, Cx), ref), f"{int((dx.reshape(-1, Cx) != ref).sum())} elements differ"
    if want is None:
        assert part is None
        return
    assert part is not None and part.shape[1:] == (2, Cx)
    for i in (0, 1):
        assert (part[:, i].double().sum(0) - want[i]).abs().max() <= 1e-6 * max(1.0, want[i].abs().max().item())


@pytest.mark.parametrize("sums", [True, False], ids=["sums", "nosums"])
@pytest.mark.parametrize("N,H,W", [(2, 12, 20), (2, 20, 12), (3, 6, 10), (3, 10, 6)])
def test_po_half_resolution_addend_on_rectangular_maps(dev, N, H, W, sums):
    """the only launch that uses the map's extents (W, H, magic_w, magic_h of the po kernarg): the downsample branch's gradient exists at even rows
    and columns only and comes as the compact [N][H/2][W/2][C] tensor; the reference adds the zero-filled full-size one.  Both orientations;
    480 and 180 pixels are no multiples of the 64-pixel tile"""
    name, dx, part, ref, want = _po_dgrad(dev, N, H, W, 512, 256, 3, sums, 31)
    assert name == "po_k256_b256_s%d_a3" % (2 if sums else 0), name
    _check_po(dx, part, ref, want, 512)


@pytest.mark.parametrize("sums", [True, False], ids=["sums", "nosums"])
@pytest.mark.parametrize("add", [1, 2], ids=["plain", "masked"])
def test_po_plain_and_masked_addend_on_a_rectangular_map(dev, add, sums):
    """3 x 10 x 14 = 420 pixels: six whole 64-pixel tiles and one of 36"""
    name, dx, part, ref, want = _po_dgrad(dev, 3, 10, 14, 512, 128, add, sums, 32)
    assert name == "po_k128_b256_s%d_a%d" % (2 if sums else 0, add), name
    _check_po(dx, part, ref, want, 512)


def _int_fwd(dev, N, H, W, Cin, Cout, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, H, W, Cin), generator=g).float()
    w = torch.randint(-2, 3, (Cout, K, K, Cin), generator=g).float()
    return x, w, R.conv2d_fwd(x, w, 1, K // 2)


def test_pk_and_pw_take_a_rectangular_map_of_whole_tiles(dev, monkeypatch):
    """4 x 7 x 28 = 784 pixels = 4 tiles of 196 (pk) = 7 tiles of 112 (pw): the tile is a run of flat pixels, whatever the map's shape.  The default
    rule gives 256 -> 1024 to the resident-weight kernels (po); MI355_PO=0 leaves it to pw"""
    from sota_imagenet_amd import ops

    x, w, ref = _int_fwd(dev, 4, 7, 28, 1024, 256, 1, 33)
    y = ops.conv2d_fwd(x.to(dev, torch.bfloat16), w.to(dev, torch.bfloat16), 1, 0)
    assert ops.last_conv_kernel() == "pk_k1024_n256_w196_s0", ops.last_conv_kernel()
    assert torch.equal(y.float().cpu(), as_dtype(ref, torch.bfloat16))
    x, w, ref = _int_fwd(dev, 4, 7, 28, 256, 1024, 1, 34)
    y = ops.conv2d_fwd(x.to(dev, torch.bfloat16), w.to(dev, torch.bfloat16), 1, 0)
    assert ops.last_conv_kernel() == "po_k256_b256_s0_a0", ops.last_conv_kernel()
    assert torch.equal(y.float().cpu(), as_dtype(ref, torch.bfloat16))
    monkeypatch.setenv("MI355_PO", "0")
    y = ops.conv2d_fwd(x.to(dev, torch.bfloat16), w.to(dev, torch.bfloat16), 1, 0)
    assert ops.last_conv_kernel() == "pw_k256_n1024_s0", ops.last_conv_kernel()
    assert torch.equal(y.float().cpu(), as_dtype(ref, torch.bfloat16))


@pytest.mark.parametrize("N,H,W,Cin,Cout,kernel", [(3, 5, 9, 64, 256, "wg1_c64_o256"), (3, 9, 5, 512, 128, "wg1_c512_o128")])
def test_generated_pointwise_weight_gradient_on_a_rectangular_map(dev, N, H, W, Cin, Cout, kernel):
    """135 pixels: two 64-pixel tiles and one of 7; accumulation into an existing gradient"""
    from sota_imagenet_amd import ops

    case = (N, H, W, Cin, Cout, 1, 1, 1, 0)
    x, _, dy, _ = _dev_operands(case, torch.bfloat16, dev)
    _, _, dw_ref = expected(case)
    dw = ops.conv2d_wgrad(dy, x, 1, 1, 1, 0)
    assert ops.last_conv_kernel() == kernel, ops.last_conv_kernel()
    assert torch.equal(dw.cpu(), dw_ref)
    assert torch.equal(ops.conv2d_wgrad(dy, x, 1, 1, 1, 0, dw=dw.clone(), beta=1.0).cpu(), 2 * dw_ref)


def test_generated_3x3_kernels_refuse_a_map_of_matching_area_but_other_shape(dev):
    """7 x 28 = 14 x 14 pixels, 256 channels: dconv_l3 / wg3_l3 are built for 14 x 14 rows and must not take it; the result is still exact"""
    from sota_imagenet_amd import ops

    case = (2, 7, 28, 256, 256, 3, 3, 1, 1)
    x, w, dy, _ = _dev_operands(case, torch.bfloat16, dev)
    y_ref, dx_ref, dw_ref = expected(case)
    y = ops.conv2d_fwd(x, w, 1, 1)
    assert not ops.last_conv_kernel().startswith("dconv"), ops.last_conv_kernel()
    assert torch.equal(y.float().cpu(), as_dtype(y_ref, torch.bfloat16))
    dx = ops.conv2d_dgrad(dy, w, (2, 7, 28, 256), 1, 1)
    assert not ops.last_conv_kernel().startswith("dconv"), ops.last_conv_kernel()
    assert torch.equal(dx.float().cpu(), as_dtype(dx_ref, torch.bfloat16))
    dw = ops.conv2d_wgrad(dy, x, 3, 3, 1, 1)
    assert not ops.last_conv_kernel().startswith("wg3"), ops.last_conv_kernel()
    assert torch.equal(dw.cpu(), dw_ref)
    sq = (2, 14, 14, 256, 256, 3, 3, 1, 1)   # the same launches at the square shape do take them: the refusal above is the shape's
    xs, ws_, dys, _ = _dev_operands(sq, torch.bfloat16, dev)
    ops.conv2d_fwd(xs, ws_, 1, 1)
    assert ops.last_conv_kernel() == "dconv_l3_s0", ops.last_conv_kernel()
    ops.conv2d_wgrad(dys, xs, 3, 3, 1, 1)
    assert ops.last_conv_kernel() == "wg3_l3", ops.last_conv_kernel()


# ---- 3d: random data ------------------------------------------------------------------------------------------------------------------------
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}   # tests/test_ops_gpu.py


def _nerr(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def _rnd(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(dtype).float()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [(2, 6, 10, 64, 64, 3, 3, 1, 1), (2, 8, 12, 128, 64, 3, 3, 2, 1), (2, 6, 8, 64, 64, 2, 3, 1, 1)], ids=case_id)
def test_random_data(dev, case, dtype):
    from sota_imagenet_amd import ops

    N, H, W, Cin, Cout, KH, KW, s, p = case
    x, w = _rnd((N, H, W, Cin), 1, dtype), _rnd((Cout, KH, KW, Cin), 2, dtype, 0.1)
    y_ref = R.conv2d_fwd(x, w, s, p)
    dy, add = _rnd(tuple(y_ref.shape), 3, dtype), _rnd((N, H, W, Cin), 4, dtype)
    dx_ref, dw_ref = R.conv2d_bwd(x, w, dy, s, p)
    xd, wd, dyd, addd = (t.to(dev, dtype).contiguous() for t in (x, w, dy, add))
    errs = (_nerr(ops.conv2d_fwd(xd, wd, s, p), y_ref), _nerr(ops.conv2d_dgrad(dyd, wd, (N, H, W, Cin), s, p), dx_ref),
            _nerr(ops.conv2d_dgrad(dyd, wd, (N, H, W, Cin), s, p, addend=addd), dx_ref + add), _nerr(ops.conv2d_wgrad(dyd, xd, KH, KW, s, p), dw_ref))
    print("random data %s %s: fwd %.2e dgrad %.2e dgrad+addend %.2e wgrad %.2e" % ((case_id(case), str(dtype)) + errs))
    assert max(errs) < TOL[dtype], errs


# ---- 4: refusals ----------------------------------------------------------------------------------------------------------------------------
def _zeros(dev, dtype, *shape):
    return torch.zeros(shape, dtype=dtype, device=dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case,msg", [((1, 4, 6, 96, 64, 3, 3, 1, 1), "multiples of 64"), ((1, 6, 8, 64, 64, 2, 5, 1, 1), "kernel 2x5 unsupported"),
                                      ((1, 9, 9, 64, 64, 3, 3, 3, 1), "stride 3 unsupported")],
                         ids=["cin96", "ten-taps", "stride3"])
def test_geometry_outside_the_domain_is_refused_with_a_message(dev, case, msg, dtype):
    N, H, W, Cin, Cout, KH, KW, s, p = case
    x, w = _zeros(dev, dtype, N, H, W, Cin), _zeros(dev, dtype, Cout, KH, KW, Cin)
    dy = _zeros(dev, dtype, *out_shape(case))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    y = Fenced(out_shape(case), dtype, dev).arm()
    with pytest.raises(RuntimeError, match=msg):
        fwd(case, x, w, y.view)
    dx = Fenced((N, H, W, Cin), dtype, dev).arm()
    with pytest.raises(RuntimeError, match=msg):
        dgrad(case, dy, w, dx.view, None, ws, ws.numel())
    dw = Fenced((Cout, KH, KW, Cin), torch.float32, dev).arm()
    with pytest.raises(RuntimeError, match=msg):
        wgrad(case, dy, x, dw.view, 0.0, ws, ws.numel())
    torch.cuda.synchronize()
    assert y.untouched() and dx.untouched() and dw.untouched()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [c for c in CASES if not has_dgrad(c)], ids=case_id)
def test_stride_2_data_gradient_at_odd_extents_is_refused(dev, case, dtype):
    from sota_imagenet_amd import ops

    N, H, W, Cin, Cout, KH, KW, s, p = case
    _, w, dy, _ = _dev_operands(case, dtype, dev)
    ws, ws_bytes = _ws(case, dtype, dev)
    dx = Fenced((N, H, W, Cin), dtype, dev).arm()
    with pytest.raises(RuntimeError, match=f"dgrad: stride=2 with H={H} W={W} unsupported"):
        dgrad(case, dy, w, dx.view, None, ws, ws_bytes)
    torch.cuda.synchronize()
    assert dx.untouched()
    with pytest.raises(RuntimeError, match="dgrad: stride=2"):   # the executor's form of the launch refuses it too
        ops.conv2d_dgrad_bn(dy, w, (N, H, W, Cin), s, p)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_a_workspace_one_byte_too_small_is_refused(dev, dtype):
    """the bound is the real one: one byte less is refused and leaves the output alone, exactly the bound computes the exact result"""
    case = (2, 6, 10, 64, 64, 3, 3, 1, 1)
    N, H, W, Cin, Cout, KH, KW, s, p = case
    x, w, dy, _ = _dev_operands(case, dtype, dev)
    _, dx_ref, dw_ref = expected(case)
    ws, _ = _ws(case, dtype, dev)
    need = Cin * KH * KW * Cout * x.element_size()   # the transposed weights
    dx = Fenced((N, H, W, Cin), dtype, dev).arm()
    with pytest.raises(RuntimeError, match=r"dgrad: workspace too small \(%d < %d\)" % (need - 1, need)):
        dgrad(case, dy, w, dx.view, None, ws, need - 1)
    torch.cuda.synchronize()
    assert dx.untouched()
    dgrad(case, dy, w, dx.view, None, ws, need)
    dx.check(as_dtype(dx_ref, dtype), "data gradient at the bound")

    dw = Fenced((Cout, KH, KW, Cin), torch.float32, dev).arm()
    with pytest.raises(RuntimeError, match="wgrad: workspace too small") as e:
        wgrad(case, dy, x, dw.view, 0.0, ws, 0)
    need = int(re.search(r"\(0 < (\d+)\)", str(e.value)).group(1))   # split count x gradient size x 4: the message states it
    assert need > 0 and need % (Cout * KH * KW * Cin * 4) == 0 and need <= ws.numel()
    with pytest.raises(RuntimeError, match=r"wgrad: workspace too small \(%d < %d\)" % (need - 1, need)):
        wgrad(case, dy, x, dw.view, 0.0, ws, need - 1)
    torch.cuda.synchronize()
    assert dw.untouched()
    wgrad(case, dy, x, dw.view, 0.0, ws, need)
    dw.check(dw_ref, "weight gradient at the bound")
