"""Per-op Python entry points over the C-ABI (include/mi355rn.h) on PyTorch-ROCm tensors.

These are the unit-level handles the parity tests use; the training path goes through the whole-network executor
(sota_imagenet_amd/models.py).  Tensors are NHWC (`[N,H,W,C]`), conv weights KRSC (`[Cout,KH,KW,Cin]`).  Every function enqueues on torch's
current stream and raises RuntimeError on any native failure.

Argument contract.  The library receives raw addresses and a few integers: it cannot know how long a buffer is.  So every wrapper tests what it
is given, in one way and before it allocates or enqueues anything: with _arg each tensor's dtype, contiguity and extent — the extent the header
states for the entry point —, then once with _on_device that all of them are CUDA (ROCm) tensors on ONE device; host-side record tables that must
not overlap go through _check_disjoint.  A ValueError names the wrapper and the argument.  Geometry the kernels do not have (channel multiples,
strides, alignment) stays the library's to refuse (RuntimeError).  Whether the tensors' device is torch's current one is not tested: cur_stream()
is the current device's stream.
"""
import ctypes

import numpy as np
import torch

from . import native
from .native import check, cur_stream, dtype_code, ptr

_F32, _F64, _I32, _I64, _U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
_NHWC = (None, None, None, None)            # any [N, H, W, C]
_ACT = (torch.float32, torch.bfloat16)      # the activation dtypes (MI355_F32, MI355_BF16)
_E4M3 = (torch.float8_e4m3fn, torch.uint8)  # e4m3 operand bytes, as quantize_fp8 returns them or viewed as bytes


def _L():
    return native.lib()


# ---- the argument contract ---------------------------------------------------------------------------------------------------------------------
def _arg(who, names, dtype, shape, *ts, optional=False):
    """ValueError unless every tensor of ts is a contiguous tensor of `dtype` (one dtype or a tuple of allowed ones) and extent `shape`: an int
    n — exactly n elements, any rank; a tuple of int (exactly that extent) and None (any extent >= 1); None — any extent.  optional: a tensor may
    be None.  names: the arguments' names, a constant string with blanks between them that is taken apart only to raise."""
    for t in ts:
        if t is None:
            if optional:
                continue
        elif isinstance(t, torch.Tensor) and (t.dtype == dtype or (dtype.__class__ is tuple and t.dtype in dtype)) and t.is_contiguous():
            if shape is None or (t.numel() == shape if shape.__class__ is int else
                                 t.dim() == len(shape) and all(have >= 1 if want is None else have == want for have, want in zip(t.shape, shape))):
                continue
        if shape is None or shape.__class__ is int:
            extent = "of any shape" if shape is None else f"of {shape} elements"
        else:
            extent = "[" + ", ".join("n" if s is None else str(s) for s in shape) + "]"
        got = f"{t.dtype} {tuple(t.shape)}{'' if t.is_contiguous() else ' (not contiguous)'}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{who}: {_name(names, ts, t)} must be a contiguous {dtype} tensor {extent}, got {got}")


def _name(names, ts, t):
    return names.split()[[k for k, x in enumerate(ts) if x is t][0]]


def _on_device(who, names, *ts):
    """ValueError unless every given tensor (None: an optional one left out) is a CUDA (ROCm) tensor and all live on one device, which is
    returned.  Called after the _arg tests of a wrapper, so that a malformed tensor is named for its form wherever it lives."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{who}: {_name(names, ts, t)} must be a CUDA (ROCm) tensor, got one on {t.device}")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"{who}: {_name(names, ts, t)} lives on {t.device}, the arguments before it on {dev}: all must live on one device")
    return dev


def _flat(who, names, *ts):
    """the flat fp32 arrays of one length that an optimizer step or a family's offsets count from: that length, the first one's"""
    n = ts[0].numel() if isinstance(ts[0], torch.Tensor) else None
    _arg(who, names, _F32, n, *ts)
    return n


def _check_disjoint(what, spans):
    """ValueError if one of the spans [(first element, length)], given in sorted order, begins before the one in front of it ends: two workgroups
    would rewrite the same elements.  what: "<op>: the record" or "<op>: the item", as the message names it"""
    end = None
    for first, length in spans:
        if end is not None and first < end:
            raise ValueError(f"{what} at offset {first} overlaps the one before it (which ends at {end})")
        end = first + length


def _ema_step(stem, names, flat, behind, ema, ema_decay, lead=(), then=(), others=()):
    """the one "plain entry point or its _ema twin" branch: mi355_<stem>(*lead, pointers, n, *behind, stream), or with ema
    mi355_<stem>_ema(*lead, pointers, ema, n, *behind, ema_decay, stream).  flat: the wrapper's fp32 arrays of one length n, p first, tested
    here, and ema like them; then: the tensors whose pointers follow theirs, others: those whose pointers are in `behind`, both tested by the
    wrapper; names: those of flat, then, others, and "ema".  Last, the placement of all."""
    n = _flat(stem, names, *flat)
    _arg(stem, "ema", _F32, n, ema, optional=True)
    _on_device(stem, names, *flat, *then, *others, ema)
    if ema is None:
        check(getattr(_L(), "mi355_" + stem)(*lead, *map(ptr, flat), *map(ptr, then), n, *behind, cur_stream()))
    else:
        check(getattr(_L(), "mi355_" + stem + "_ema")(*lead, *map(ptr, flat), *map(ptr, then), ptr(ema), n, *behind, float(ema_decay), cur_stream()))


# ---- what a call returns or borrows ------------------------------------------------------------------------------------------------------------
def _scratch(nbytes, device):
    """(workspace, its bytes) of one call: the conv, BatchNorm, stem and ECA launchers take theirs from the caller"""
    return torch.empty(nbytes, dtype=_U8, device=device), nbytes


def _half(N, H, W, C):
    """the half-resolution output of the 2x2 / stride-2 ops"""
    return (N, H // 2, W // 2, C)


def _conv_out(N, H, W, Cout, KH, KW, stride, pad):
    return (N, (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1, Cout)


# rows of the statistics scratch: the implicit-GEMM kernels write <= 768, the generated kernels one per pixel tile (3584 for a
# 56 x 56 x 64 conv at batch 256, 14336 for a 112 x 112 x 64 one: two-row tiles); the library takes the kernel the buffer allows (the static
# executors give it their widest layer's)
STATS_ROWS_C128, STATS_ROWS_C256, STATS_ROWS_IGEMM = 16384, 8192, 768  # Cout <= 128, Cout <= 256, wider
DGRAD_BN_ROWS = 4096  # rows of the BN-backward partial sums a data-gradient epilogue may leave


def _stats_partial(rows, C, device):
    return torch.empty(rows * 2 * C, dtype=_F32, device=device), ctypes.c_int(0)


def _stats_rows(partial, nblk, C):
    return partial[: nblk.value * 2 * C].view(nblk.value, 2, C) if nblk.value > 0 else None


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------------
def conv2d_fwd(x, w, stride=1, pad=0, stats=False):
    """stats=True: returns (y, partial) — `partial` = the BN batch-statistics rows the conv epilogue summed over y, an fp32
    tensor [nblk, 2, Cout] (or None where the launch could not carry them) to hand to bn_fwd_train(y, ..., stats=partial):
    an explicit value owned by the caller, valid for exactly this y as long as y is not modified."""
    _arg("conv2d_fwd", "x", _ACT, _NHWC, x)
    N, H, W, Cin = x.shape
    _arg("conv2d_fwd", "w", x.dtype, (None, None, None, Cin), w)
    dev = _on_device("conv2d_fwd", "x w", x, w)
    Cout, KH, KW, _ = w.shape
    y = torch.empty(_conv_out(N, H, W, Cout, KH, KW, stride, pad), dtype=x.dtype, device=dev)
    if not stats:
        check(_L().mi355_conv2d_fwd(dtype_code(x.dtype), ptr(x), ptr(w), ptr(y), N, H, W, Cin, Cout, KH, KW, stride, pad, cur_stream()))
        return y
    partial, nblk = _stats_partial(STATS_ROWS_C128 if Cout <= 128 else (STATS_ROWS_C256 if Cout <= 256 else STATS_ROWS_IGEMM), Cout, dev)
    check(_L().mi355_conv2d_fwd_stats(dtype_code(x.dtype), ptr(x), ptr(w), ptr(y), ptr(partial), partial.numel() * 4, ctypes.byref(nblk), N, H, W, Cin,
                                      Cout, KH, KW, stride, pad, cur_stream()))
    return y, _stats_rows(partial, nblk, Cout)


def conv2d_fwd_bn_in(y_in, scale, shift, w, pad=1):
    """the forward conv with the previous layer's BatchNorm + ReLU in its operand path (mi355_conv2d_fwd_bn_in): returns
    (y, partial, a, a_bits) — y = conv(a, w) with a = relu(y_in * scale + shift) rounded to y_in's dtype, the BN statistics rows of y, and
    the by-products a and its ReLU bits (1 byte per 8 channels) the same launch leaves for the backward pass.  scale, shift: fp32 [Cin]"""
    _arg("conv2d_fwd_bn_in", "y_in", _ACT, _NHWC, y_in)
    N, H, W, Cin = y_in.shape
    _arg("conv2d_fwd_bn_in", "scale shift", _F32, Cin, scale, shift)
    _arg("conv2d_fwd_bn_in", "w", y_in.dtype, (None, None, None, Cin), w)
    dev = _on_device("conv2d_fwd_bn_in", "y_in scale shift w", y_in, scale, shift, w)
    Cout, KH, KW, _ = w.shape
    y = torch.empty((N, H, W, Cout), dtype=y_in.dtype, device=dev)
    a = torch.empty_like(y_in)
    bits = torch.empty((N, H, W, Cin // 8), dtype=_U8, device=dev)
    ss = torch.cat([scale.reshape(-1), shift.reshape(-1)])
    partial, nblk = _stats_partial(STATS_ROWS_C256 if Cout <= 256 else STATS_ROWS_IGEMM, Cout, dev)
    check(_L().mi355_conv2d_fwd_bn_in(dtype_code(y_in.dtype), ptr(y_in), ptr(ss), ptr(w), ptr(y), ptr(a), ptr(bits), ptr(partial), partial.numel() * 4,
                                      ctypes.byref(nblk), N, H, W, Cin, Cout, KH, KW, 1, pad, cur_stream()))
    return y, _stats_rows(partial, nblk, Cout), a, bits


def quantize_fp8(x, scale=1.0):
    """q = saturate_e4m3fn(x * scale) as a torch.float8_e4m3fn tensor of x's shape (x fp32 or bf16, numel % 8 == 0)."""
    _arg("quantize_fp8", "x", _ACT, None, x)
    dev = _on_device("quantize_fp8", "x", x)
    q = torch.empty(x.shape, dtype=_U8, device=dev)
    check(_L().mi355_quantize_fp8(dtype_code(x.dtype), ptr(x), ptr(q), float(scale), x.numel(), cur_stream()))
    return q.view(torch.float8_e4m3fn)


def conv2d_fwd_fp8(xq, wq, stride=1, pad=0, oscale=1.0):
    """bf16 y = conv(xq NHWC e4m3, wq KRSC e4m3) * oscale on the fp8 MFMA path (Cin, Cout multiples of 128)."""
    _arg("conv2d_fwd_fp8", "xq", _E4M3, _NHWC, xq)
    N, H, W, Cin = xq.shape
    _arg("conv2d_fwd_fp8", "wq", _E4M3, (None, None, None, Cin), wq)
    dev = _on_device("conv2d_fwd_fp8", "xq wq", xq, wq)
    Cout, KH, KW, _ = wq.shape
    y = torch.empty(_conv_out(N, H, W, Cout, KH, KW, stride, pad), dtype=torch.bfloat16, device=dev)
    check(_L().mi355_conv2d_fwd_fp8(ptr(xq), ptr(wq), ptr(y), float(oscale), N, H, W, Cin, Cout, KH, KW, stride, pad, cur_stream()))
    return y


def conv2d_dgrad_fp8(dyq, wq, x_shape, stride=1, pad=0, oscale=1.0, wt=None):
    """bf16 dx for the conv above from e4m3 dy and the KRSC e4m3 weights (transposed here to [Cin][KH][KW][Cout], or given so as wt)."""
    N, H, W, Cin = x_shape
    _arg("conv2d_dgrad_fp8", "wq", _E4M3, (None, None, None, Cin), wq)
    Cout, KH, KW, _ = wq.shape
    _arg("conv2d_dgrad_fp8", "dyq", _E4M3, _conv_out(N, H, W, Cout, KH, KW, stride, pad), dyq)
    _arg("conv2d_dgrad_fp8", "wt", _E4M3, (Cin, KH, KW, Cout), wt, optional=True)
    dev = _on_device("conv2d_dgrad_fp8", "dyq wq wt", dyq, wq, wt)
    if wt is None:
        wt = wq.view(_U8).permute(3, 1, 2, 0).contiguous()
    dx = torch.empty((N, H, W, Cin), dtype=torch.bfloat16, device=dev)
    check(_L().mi355_conv2d_dgrad_fp8(ptr(dyq), ptr(wt), ptr(dx), float(oscale), N, H, W, Cin, Cout, KH, KW, stride, pad, cur_stream()))
    return dx


_WGRAD_WS = {}


def conv2d_wgrad_fp8(dyq, xq, KH, KW, stride=1, pad=0, oscale=1.0):
    """fp32 dw [Cout,KH,KW,Cin] = oscale * sum_pixels dyq (x) xq from e4m3 dy (NHWC) and x (NHWC) on the fp8 MFMA path."""
    _arg("conv2d_wgrad_fp8", "xq", _E4M3, _NHWC, xq)
    N, H, W, Cin = xq.shape
    _arg("conv2d_wgrad_fp8", "dyq", _E4M3, _conv_out(N, H, W, None, KH, KW, stride, pad), dyq)
    dev = _on_device("conv2d_wgrad_fp8", "dyq xq", dyq, xq)
    Cout = dyq.shape[-1]
    n = _L().mi355_conv2d_workspace_bytes(native.BF16, N, H, W, Cin, Cout, KH, KW, stride, pad)
    # split-K slabs + the two scale words: one workspace per (device, stream, size) — calls on different streams must not share slabs —
    # and at most 8 of them (the oldest goes first)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream, n)
    ws = _WGRAD_WS.get(key)
    if ws is None:
        while len(_WGRAD_WS) >= 8:
            _WGRAD_WS.pop(next(iter(_WGRAD_WS)))
        ws = _WGRAD_WS[key] = torch.empty(n + 256, dtype=_U8, device=dev)
    dw = torch.empty((Cout, KH, KW, Cin), dtype=_F32, device=dev)
    check(_L().mi355_conv2d_wgrad_fp8(ptr(dyq), ptr(xq), ptr(dw), 0.0, float(oscale), N, H, W, Cin, Cout, KH, KW, stride, pad, ptr(ws), n + 256, cur_stream()))
    return dw


def ingest_u8(packed, table_host, table_dev, S, mean=127.5, std=51.0, aug_host=None, aug_dev=None):
    """decoded u8 RGB crops (packed device bytes + mi355_crop table as a numpy structured array and its device copy) ->
    fp32 NCHW [N,3,S,S]: resize, window, [augment table: blur / colour / grey / erase], mirror, normalise (csrc/ingest.hip).
    table_dev, aug_dev: the records as device bytes (u8, 40 and 128 per sample)."""
    N = int(table_host.shape[0])
    if table_host.dtype.itemsize != 40 or not table_host.flags["C_CONTIGUOUS"]:
        raise ValueError(f"ingest_u8: table_host must be a contiguous numpy array of N 40-byte mi355_crop records, got {table_host.dtype} {table_host.shape}")
    if aug_host is not None and (aug_host.dtype.itemsize != 128 or aug_host.shape[0] != N or not aug_host.flags["C_CONTIGUOUS"]):
        raise ValueError(f"ingest_u8: aug_host must be a contiguous numpy array of {N} 128-byte mi355_augment records, got {aug_host.dtype} {aug_host.shape}")
    _arg("ingest_u8", "packed", _U8, None, packed)
    _arg("ingest_u8", "table_dev[40-byte-records]", _U8, 40 * N, table_dev)
    _arg("ingest_u8", "aug_dev[128-byte-records]", _U8, 128 * N, aug_dev, optional=aug_host is None)
    dev = _on_device("ingest_u8", "packed table_dev aug_dev", packed, table_dev, aug_dev)
    out = torch.empty((N, 3, S, S), dtype=_F32, device=dev)
    if aug_host is None:
        check(_L().mi355_ingest_u8(ptr(packed), packed.numel(), table_host.ctypes.data, ptr(table_dev), N, int(S), float(mean), float(std), ptr(out), cur_stream()))
        return out
    scratch = torch.empty((N, 3, S, S), dtype=_F32, device=dev) if bool((aug_host["blur_sigma"] > 0).any()) else None
    check(_L().mi355_ingest_u8_aug(ptr(packed), packed.numel(), table_host.ctypes.data, ptr(table_dev), aug_host.ctypes.data, ptr(aug_dev), N, int(S),
                                   float(mean), float(std), ptr(scratch), ptr(out), cur_stream()))
    return out


def _dgrad_args(who, dy, w, x_shape, stride, pad):
    """w [Cout,KH,KW,Cin] and dy, the conv's output shape in w's dtype, for the data gradient wrt an x of x_shape: (N, H, W, Cin, Cout, KH, KW)"""
    N, H, W, Cin = x_shape
    _arg(who, "w", _ACT, (None, None, None, Cin), w)
    Cout, KH, KW, _ = w.shape
    _arg(who, "dy", w.dtype, _conv_out(N, H, W, Cout, KH, KW, stride, pad), dy)
    return N, H, W, Cin, Cout, KH, KW


def conv2d_dgrad(dy, w, x_shape, stride=1, pad=0, addend=None):
    """dx [N,H,W,Cin] = conv_transpose(dy, w) (+ addend, laid out like dx)"""
    N, H, W, Cin, Cout, KH, KW = _dgrad_args("conv2d_dgrad", dy, w, x_shape, stride, pad)
    _arg("conv2d_dgrad", "addend", dy.dtype, (N, H, W, Cin), addend, optional=True)
    dev = _on_device("conv2d_dgrad", "dy w addend", dy, w, addend)
    dt = dtype_code(dy.dtype)
    ws, n = _scratch(_L().mi355_conv2d_workspace_bytes(dt, N, H, W, Cin, Cout, KH, KW, stride, pad), dev)
    dx = torch.empty((N, H, W, Cin), dtype=dy.dtype, device=dev)
    check(_L().mi355_conv2d_dgrad(dt, ptr(dy), ptr(w), ptr(dx), ptr(addend), N, H, W, Cin, Cout, KH, KW, stride, pad, ptr(ws), n, cur_stream()))
    return dx


def conv2d_dgrad_bn(dy, w, x_shape, stride=1, pad=0, addend=None, addend_bits=None, bn_y=None, bn_bits=None, bn_mean=None, bn_invstd=None, addend_sub2=False, slope=0.0):
    """the data gradient as the executor's backward launches it: dx = dgrad(dy) + addend (under the ReLU bits addend_bits), and — with
    bn_y / bn_bits / bn_mean / bn_invstd — the BN-backward partial rows [nblk][2][Cin] (sum dz, sum dz * xhat) of the layer dx is the
    activation gradient of.  addend_sub2: the addend is [N, H/2, W/2, Cin], standing for a full-resolution tensor that is zero at odd rows /
    columns.  slope: the sums under a leaky-ReLU mask (dz = dx * slope where the bit is clear; 0.01 at BResNet-50's shapes, mi355_conv2d_dgrad_bn_leaky).
    bn_y is laid out like dx, bn_mean / bn_invstd are fp32 [Cin]; the masks are u8 [N, H, W, Cin / V], one byte per 16-byte vector of dx (V = 16 bytes
    of elements) — their last extent is not tested here: a GPU test calls this in fp32 with masks sized for bf16 and expects the library's refusal.
    Returns (dx, partial or None)."""
    who = "conv2d_dgrad_bn"
    N, H, W, Cin, Cout, KH, KW = _dgrad_args(who, dy, w, x_shape, stride, pad)
    _arg(who, "addend", dy.dtype, _half(N, H, W, Cin) if addend_sub2 else (N, H, W, Cin), addend, optional=True)
    _arg(who, "bn_y", dy.dtype, (N, H, W, Cin), bn_y, optional=True)
    _arg(who, "addend_bits bn_bits", _U8, (N, H, W, None), addend_bits, bn_bits, optional=True)
    _arg(who, "bn_mean bn_invstd", _F32, Cin, bn_mean, bn_invstd, optional=True)
    dev = _on_device(who, "dy w addend addend_bits bn_y bn_bits bn_mean bn_invstd", dy, w, addend, addend_bits, bn_y, bn_bits, bn_mean, bn_invstd)
    dt = dtype_code(dy.dtype)
    ws, n = _scratch(_L().mi355_conv2d_workspace_bytes(dt, N, H, W, Cin, Cout, KH, KW, stride, pad), dev)
    dx = torch.empty((N, H, W, Cin), dtype=dy.dtype, device=dev)
    nblk = ctypes.c_int(0)
    part = torch.empty((DGRAD_BN_ROWS, 2, Cin), dtype=_F32, device=dev) if bn_y is not None else None
    check(_L().mi355_conv2d_dgrad_bn_leaky(dt, ptr(dy), ptr(w), ptr(dx), ptr(addend), ptr(addend_bits), int(addend_sub2), ptr(bn_y), ptr(bn_bits), ptr(bn_mean),
                                           ptr(bn_invstd), float(slope), ptr(part), 0 if part is None else part.numel() * 4, ctypes.byref(nblk), N, H, W, Cin, Cout,
                                           KH, KW, stride, pad, ptr(ws), n, cur_stream()))
    if part is not None:
        part = part[:nblk.value] if nblk.value > 0 else None
    return dx, part


def last_conv_kernel():
    """name of the kernel the last conv / weight-gradient launch of this thread went to (mi355_last_conv_kernel)"""
    return _L().mi355_last_conv_kernel().decode()


def conv2d_wgrad(dy, x, KH, KW, stride=1, pad=0, dw=None, beta=0.0):
    """fp32 dw [Cout,KH,KW,Cin] = beta * dw + sum_pixels dy (x) x; dy: the conv's output shape in x's dtype"""
    _arg("conv2d_wgrad", "x", _ACT, _NHWC, x)
    N, H, W, Cin = x.shape
    _arg("conv2d_wgrad", "dy", x.dtype, _conv_out(N, H, W, None, KH, KW, stride, pad), dy)
    Cout = dy.shape[-1]
    _arg("conv2d_wgrad", "dw", _F32, (Cout, KH, KW, Cin), dw, optional=True)
    dev = _on_device("conv2d_wgrad", "dy x dw", dy, x, dw)
    dt = dtype_code(dy.dtype)
    ws, n = _scratch(_L().mi355_conv2d_workspace_bytes(dt, N, H, W, Cin, Cout, KH, KW, stride, pad), dev)
    if dw is None:
        dw = torch.empty((Cout, KH, KW, Cin), dtype=_F32, device=dev)
    check(_L().mi355_conv2d_wgrad(dt, ptr(dy), ptr(x), ptr(dw), beta, N, H, W, Cin, Cout, KH, KW, stride, pad, ptr(ws), n, cur_stream()))
    return dw


def stem_ingest(x_nchw, dtype):
    """the loader's fp32 NCHW batch [N,3,H,W] -> the zero-padded NHWC4 `dtype` bytes the stem kernels read"""
    _arg("stem_ingest", "x_nchw", _F32, (None, 3, None, None), x_nchw)
    dev = _on_device("stem_ingest", "x_nchw", x_nchw)
    N, _, H, W = x_nchw.shape
    dt = dtype_code(dtype)
    xpad = torch.zeros(_L().mi355_stem_xpad_bytes(dt, N, H, W), dtype=_U8, device=dev)
    check(_L().mi355_stem_ingest(dt, ptr(x_nchw), ptr(xpad), N, H, W, cur_stream()))
    return xpad


def stem_fwd(xpad, w, N, H, W, dtype):
    """w: [64,7,7,3] fp32 (KRSC); xpad: the bytes stem_ingest returned for this N, H, W and dtype."""
    dt = dtype_code(dtype)
    _arg("stem_fwd", "xpad", _U8, _L().mi355_stem_xpad_bytes(dt, N, H, W), xpad)
    _arg("stem_fwd", "w", _F32, (64, 7, 7, 3), w)
    dev = _on_device("stem_fwd", "xpad w", xpad, w)
    ws, n = _scratch(_L().mi355_stem_workspace_bytes(dt, N, H, W), dev)
    y = torch.empty(_half(N, H, W, 64), dtype=dtype, device=dev)
    check(_L().mi355_stem_fwd(dt, ptr(xpad), ptr(w), ptr(y), N, H, W, ptr(ws), n, cur_stream()))
    return y


def stem_wgrad(dy, xpad, N, H, W):
    """fp32 dw [64,7,7,3] from dy [N,H/2,W/2,64] and the bytes stem_ingest returned for this N, H, W and dy's dtype"""
    _arg("stem_wgrad", "dy", _ACT, _half(N, H, W, 64), dy)
    dt = dtype_code(dy.dtype)
    _arg("stem_wgrad", "xpad", _U8, _L().mi355_stem_xpad_bytes(dt, N, H, W), xpad)
    dev = _on_device("stem_wgrad", "dy xpad", dy, xpad)
    ws, n = _scratch(_L().mi355_stem_workspace_bytes(dt, N, H, W), dev)
    dw = torch.empty((64, 7, 7, 3), dtype=_F32, device=dev)
    check(_L().mi355_stem_wgrad(dt, ptr(dy), ptr(xpad), ptr(dw), 0.0, N, H, W, ptr(ws), n, cur_stream()))
    return dw


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------------------------
def bn_fwd_train(x, gamma, beta, running_mean, running_var, residual=None, relu=True, eps=1e-5, momentum=0.1, stats=None):
    """x: [..., C] NHWC.  Updates running stats in place (as a pair they may be None).  Returns (out, save_mean, save_invstd).
    stats: the partial rows conv2d_fwd(stats=True) returned for THIS x (no reduction pass over x then)."""
    _arg("bn_fwd_train", "x", _ACT, None, x)
    C = x.shape[-1]
    _arg("bn_fwd_train", "gamma beta", _F32, C, gamma, beta)
    _arg("bn_fwd_train", "running_mean running_var", _F32, C, running_mean, running_var, optional=True)
    _arg("bn_fwd_train", "residual", x.dtype, x.shape, residual, optional=True)
    _arg("bn_fwd_train", "stats", _F32, (None, 2, C), stats, optional=True)
    dev = _on_device("bn_fwd_train", "x gamma beta running_mean running_var residual stats", x, gamma, beta, running_mean, running_var, residual, stats)
    M = x.numel() // C
    out = torch.empty_like(x)
    sm = torch.empty(C, dtype=_F32, device=dev)
    si = torch.empty(C, dtype=_F32, device=dev)
    if stats is not None:  # the conv that produced x already summed it
        ws, n = _scratch(8 * C, dev)  # 2*C floats
        check(_L().mi355_bn_fwd_train_partial(dtype_code(x.dtype), ptr(x), ptr(residual), ptr(out), ptr(gamma), ptr(beta), ptr(running_mean),
                                              ptr(running_var), ptr(sm), ptr(si), M, C, eps, momentum, int(relu), ptr(stats), stats.shape[0], ptr(ws),
                                              n, cur_stream()))
        return out, sm, si
    ws, n = _scratch(_L().mi355_bn_workspace_bytes(C), dev)
    check(_L().mi355_bn_fwd_train(dtype_code(x.dtype), ptr(x), ptr(residual), ptr(out), ptr(gamma), ptr(beta), ptr(running_mean),
                                  ptr(running_var), ptr(sm), ptr(si), M, C, eps, momentum, int(relu), ptr(ws), n, cur_stream()))
    return out, sm, si


def bn_fwd_eval(x, gamma, beta, running_mean, running_var, residual=None, relu=True, eps=1e-5):
    """x: [..., C] NHWC, residual like x, the four vectors fp32 [C].  Returns out."""
    _arg("bn_fwd_eval", "x", _ACT, None, x)
    C = x.shape[-1]
    _arg("bn_fwd_eval", "gamma beta running_mean running_var", _F32, C, gamma, beta, running_mean, running_var)
    _arg("bn_fwd_eval", "residual", x.dtype, x.shape, residual, optional=True)
    dev = _on_device("bn_fwd_eval", "x gamma beta running_mean running_var residual", x, gamma, beta, running_mean, running_var, residual)
    M = x.numel() // C
    out = torch.empty_like(x)
    ws, n = _scratch(_L().mi355_bn_workspace_bytes(C), dev)
    check(_L().mi355_bn_fwd_eval(dtype_code(x.dtype), ptr(x), ptr(residual), ptr(out), ptr(gamma), ptr(beta), ptr(running_mean),
                                 ptr(running_var), M, C, eps, int(relu), ptr(ws), n, cur_stream()))
    return out


def bn_bwd(dout, out, x, gamma, save_mean, save_invstd, relu=True, want_dz=False, dgamma=None, dbeta=None, beta_acc=0.0):
    """Returns (dx, dgamma, dbeta, dz or None).  dgamma / dbeta given: written in place (beta_acc = 1 accumulates onto them).
    dout, out: like x; gamma, save_mean, save_invstd, dgamma, dbeta: fp32 [C]."""
    _arg("bn_bwd", "x", _ACT, None, x)
    C = x.shape[-1]
    _arg("bn_bwd", "dout out", x.dtype, x.shape, dout, out)
    _arg("bn_bwd", "gamma save_mean save_invstd", _F32, C, gamma, save_mean, save_invstd)
    _arg("bn_bwd", "dgamma dbeta", _F32, C, dgamma, dbeta, optional=True)
    dev = _on_device("bn_bwd", "dout out x gamma save_mean save_invstd dgamma dbeta", dout, out, x, gamma, save_mean, save_invstd, dgamma, dbeta)
    M = x.numel() // C
    dx = torch.empty_like(x)
    dz = torch.empty_like(x) if want_dz else None
    dg = dgamma if dgamma is not None else torch.zeros(C, dtype=_F32, device=dev)
    db = dbeta if dbeta is not None else torch.zeros(C, dtype=_F32, device=dev)
    ws, n = _scratch(_L().mi355_bn_workspace_bytes(C), dev)
    check(_L().mi355_bn_bwd(dtype_code(x.dtype), ptr(dout), ptr(out), ptr(x), ptr(gamma), ptr(save_mean), ptr(save_invstd), ptr(dx),
                            ptr(dz), ptr(dg), ptr(db), float(beta_acc), M, C, int(relu), ptr(ws), n, cur_stream()))
    return dx, dg, db, dz


def bn_apply(x, scale, shift, residual=None, x2=None, scale2=None, shift2=None, relu=1, want_bits=False):
    """The executors' BatchNorm apply pass on given fp32 coefficients (mi355_bn_apply): act(x * scale + shift (+ residual | + x2 * scale2 + shift2)).
    relu: 0 / 1 / 2 (leaky, slope 0.01).  Returns (out, bits): bits [..., C/V] u8 (V = 16 bytes of elements, bit e of byte v = the sum of channel
    v * V + e was > 0) with want_bits, else None.  Combinations the kernels do not have raise (native.check)."""
    _arg("bn_apply", "x", _ACT, None, x)
    C = x.shape[-1]
    _arg("bn_apply", "scale shift", _F32, C, scale, shift)
    _arg("bn_apply", "residual x2", x.dtype, x.shape, residual, x2, optional=True)
    _arg("bn_apply", "scale2 shift2", _F32, C, scale2, shift2, optional=True)
    dev = _on_device("bn_apply", "x scale shift residual x2 scale2 shift2", x, scale, shift, residual, x2, scale2, shift2)
    M = x.numel() // C
    V = 16 // x.element_size()
    out = torch.empty_like(x)
    bits = torch.empty(tuple(x.shape[:-1]) + (C // V,), dtype=_U8, device=dev) if want_bits else None
    check(_L().mi355_bn_apply(dtype_code(x.dtype), ptr(x), ptr(scale), ptr(shift), ptr(residual), ptr(x2), ptr(scale2), ptr(shift2), ptr(out),
                              ptr(bits), M, C, int(relu), cur_stream()))
    return out, bits


def bn_bwd_bits(g, bits, x, gamma, mean, invstd, relu=1, dx=None, dz_out=None, dgamma=None, dbeta=None, beta_acc=0.0, partial=None):
    """The executors' BatchNorm backward from the ReLU bit mask (mi355_bn_bwd_bits): returns (dx, dgamma, dbeta).  relu 0: bits None.  dx / dz_out
    given: written in place, either may be g itself.  dgamma / dbeta given: written in place (beta_acc = 1 accumulates).  partial: fp32
    [nblk, 2, C] rows of (sum dz, sum dz * x_hat) from a fused data-gradient epilogue, in place of the reduce pass (ignored, as in the executor, when
    dz_out asks for the masked gradient).  bits: u8, one byte per 16-byte vector of x."""
    _arg("bn_bwd_bits", "x", _ACT, None, x)
    C = x.shape[-1]
    M = x.numel() // C
    _arg("bn_bwd_bits", "g", x.dtype, x.shape, g)
    _arg("bn_bwd_bits", "dx dz_out", x.dtype, x.shape, dx, dz_out, optional=True)
    _arg("bn_bwd_bits", "gamma mean invstd", _F32, C, gamma, mean, invstd)
    _arg("bn_bwd_bits", "dgamma dbeta", _F32, C, dgamma, dbeta, optional=True)
    _arg("bn_bwd_bits", "bits", _U8, M * C // (16 // x.element_size()), bits, optional=True)
    _arg("bn_bwd_bits", "partial", _F32, (None, 2, C), partial, optional=True)
    dev = _on_device("bn_bwd_bits", "g bits x gamma mean invstd dx dz_out dgamma dbeta partial", g, bits, x, gamma, mean, invstd, dx, dz_out, dgamma, dbeta, partial)
    nblk = 0 if partial is None else partial.shape[0]
    dx = dx if dx is not None else torch.empty_like(x)
    dg = dgamma if dgamma is not None else torch.zeros(C, dtype=_F32, device=dev)
    db = dbeta if dbeta is not None else torch.zeros(C, dtype=_F32, device=dev)
    ws, n = _scratch(_L().mi355_bn_workspace_bytes(C), dev)
    check(_L().mi355_bn_bwd_bits(dtype_code(x.dtype), ptr(g), ptr(bits), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx), ptr(dz_out), ptr(dg),
                                 ptr(db), float(beta_acc), M, C, int(relu), ptr(partial), nblk, ptr(ws), n, cur_stream()))
    return dx, dg, db


# ---- pools, the stem tail, the head --------------------------------------------------------------------------------------------------------------
def maxpool_fwd(x):
    """3x3 / stride 2 / pad 1 on x [N,H,W,C]: returns (y, idx), both [N,H/2,W/2,C], idx u8 = the window position of the first maximum"""
    _arg("maxpool_fwd", "x", _ACT, _NHWC, x)
    dev = _on_device("maxpool_fwd", "x", x)
    N, H, W, C = x.shape
    y = torch.empty(_half(N, H, W, C), dtype=x.dtype, device=dev)
    idx = torch.empty(_half(N, H, W, C), dtype=_U8, device=dev)
    check(_L().mi355_maxpool_fwd(dtype_code(x.dtype), ptr(x), ptr(y), ptr(idx), N, H, W, C, cur_stream()))
    return y, idx


def maxpool_bwd(dy, idx, x_shape):
    """dx [N,H,W,C] from dy and the u8 codes idx maxpool_fwd returned, both [N,H/2,W/2,C]"""
    N, H, W, C = x_shape
    _arg("maxpool_bwd", "dy", _ACT, _half(N, H, W, C), dy)
    _arg("maxpool_bwd", "idx", _U8, _half(N, H, W, C), idx)
    dev = _on_device("maxpool_bwd", "dy idx", dy, idx)
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dev)
    check(_L().mi355_maxpool_bwd(dtype_code(dy.dtype), ptr(dy), ptr(idx), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def bn_relu_maxpool(y, scale, shift, form=0):
    """The stem's fused tail on the raw conv output y [N,H,W,C]: (p, idx, bits) = pooled relu(y * scale + shift), argmax codes, ReLU bits
    [N,H,W,C/V] (V = 16 bytes of elements).  form: 0 the executor's rule, 1 / 2 / 3 one of the three kernels forced (mi355rn.h)."""
    _arg("bn_relu_maxpool", "y", _ACT, _NHWC, y)
    N, H, W, C = y.shape
    _arg("bn_relu_maxpool", "scale shift", _F32, C, scale, shift)
    dev = _on_device("bn_relu_maxpool", "y scale shift", y, scale, shift)
    p = torch.empty(_half(N, H, W, C), dtype=y.dtype, device=dev)
    idx = torch.empty(_half(N, H, W, C), dtype=_U8, device=dev)
    bits = torch.empty((N, H, W, C // (16 // y.element_size())), dtype=_U8, device=dev)
    check(_L().mi355_bn_relu_maxpool(dtype_code(y.dtype), ptr(y), ptr(scale), ptr(shift), ptr(p), ptr(idx), ptr(bits), N, H, W, C, int(form),
                                     cur_stream()))
    return p, idx, bits


def stem_bwd(dp, idx, bits, y, gamma, mean, invstd, dgamma=None, dbeta=None, beta_acc=0.0):
    """The executor's stem backward from the pooled gradient dp [N,H/2,W/2,64]: returns (dx wrt y, dgamma, dbeta).  dgamma / dbeta given:
    written in place (beta_acc = 1 accumulates onto them).  idx: u8 like dp; bits: u8 [N,H,W,C/V] (V = 16 bytes of elements)."""
    _arg("stem_bwd", "y", _ACT, _NHWC, y)
    N, H, W, C = y.shape
    _arg("stem_bwd", "dp", y.dtype, _half(N, H, W, C), dp)
    _arg("stem_bwd", "idx", _U8, _half(N, H, W, C), idx)
    _arg("stem_bwd", "bits", _U8, (N, H, W, C // (16 // y.element_size())), bits)
    _arg("stem_bwd", "gamma mean invstd", _F32, C, gamma, mean, invstd)
    _arg("stem_bwd", "dgamma dbeta", _F32, C, dgamma, dbeta, optional=True)
    dev = _on_device("stem_bwd", "dp idx bits y gamma mean invstd dgamma dbeta", dp, idx, bits, y, gamma, mean, invstd, dgamma, dbeta)
    dx = torch.empty_like(y)
    dg = dgamma if dgamma is not None else torch.zeros(C, dtype=_F32, device=dev)
    db = dbeta if dbeta is not None else torch.zeros(C, dtype=_F32, device=dev)
    ws, n = _scratch(_L().mi355_bn_workspace_bytes(C), dev)
    check(_L().mi355_stem_bwd(dtype_code(y.dtype), ptr(dp), ptr(idx), ptr(bits), ptr(y), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx), ptr(dg),
                              ptr(db), beta_acc, N, H, W, C, ptr(ws), n, cur_stream()))
    return dx, dg, db


def gap_fwd(x):
    """global average pool of x [N,H,W,C]: fp32 [N,C]"""
    _arg("gap_fwd", "x", _ACT, _NHWC, x)
    dev = _on_device("gap_fwd", "x", x)
    N, H, W, C = x.shape
    pooled = torch.empty((N, C), dtype=_F32, device=dev)
    check(_L().mi355_gap_fwd(dtype_code(x.dtype), ptr(x), ptr(pooled), N, H * W, C, cur_stream()))
    return pooled


def gap_bwd(dpooled, x_shape, dtype):
    """dx [N,H,W,C] in `dtype` from dpooled, fp32 [N,C]"""
    N, H, W, C = x_shape
    _arg("gap_bwd", "dpooled", _F32, (N, C), dpooled)
    dev = _on_device("gap_bwd", "dpooled", dpooled)
    dx = torch.empty((N, H, W, C), dtype=dtype, device=dev)
    check(_L().mi355_gap_bwd(dtype_code(dtype), ptr(dpooled), ptr(dx), N, H * W, C, cur_stream()))
    return dx


def ce_loss(logits, target, smoothing=0.0, grad_scale=1.0, need_grad=True):
    """logits, target (one-hot or soft): fp32 [N,C].  Returns (loss scalar tensor on device, dlogits or None)."""
    _arg("ce_loss", "logits", _F32, (None, None), logits)
    N, C = logits.shape
    _arg("ce_loss", "target", _F32, (N, C), target)
    dev = _on_device("ce_loss", "logits target", logits, target)
    loss = torch.empty((), dtype=_F32, device=dev)
    row = torch.empty(N, dtype=_F32, device=dev)
    dl = torch.empty_like(logits) if need_grad else None
    check(_L().mi355_ce_loss(ptr(logits), ptr(target), smoothing, grad_scale, ptr(loss), ptr(row), ptr(dl), N, C, cur_stream()))
    return loss, dl


# ---- the flat optimizer steps: p, the gradient and every state fp32 of ONE length ----------------------------------------------------------------
def sgd_step(p, g, m, lr, momentum=0.0, weight_decay=0.0, grad_scale=1.0, ema=None, ema_decay=0.0):
    """ema (optional, same shape as p): the moving average of the updated parameters, advanced in the same kernel (mi355_sgd_step_ema)"""
    _ema_step("sgd_step", "p g m ema", (p, g, m), (lr, momentum, weight_decay, grad_scale), ema, ema_decay)


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, grad_scale=1.0, ema=None, ema_decay=0.0):
    """one Adam (decoupled=False) / AdamW (decoupled=True) step of a flat range whose parameters have all taken `step` steps before
    this one (torch's state['step'] after its increment is step + 1).  The bias corrections are computed here in double, as torch
    does; ema (optional): the moving average of the updated parameters, advanced in the same kernel (mi355_adam_step_ema)"""
    b1, b2 = float(betas[0]), float(betas[1])
    t = float(step + 1)
    step_size = lr / (1.0 - b1 ** t)
    bc2_sqrt = (1.0 - b2 ** t) ** 0.5
    _ema_step("adam_step", "p g m v ema", (p, g, m, v), (b1, b2, eps, step_size, bc2_sqrt, lr, weight_decay, int(bool(decoupled)), grad_scale), ema, ema_decay)


def madgrad_step(p, g, grad_sum_sq, s, x0, k, lr, momentum=0.9, weight_decay=0.0, eps=1e-6, grad_scale=1.0, ema=None, ema_decay=0.0):
    """one MADGRAD step (the reference's src.optimizers.MADGRAD) of a flat range; k: the optimizer's global counter before this step
    (lamb = (lr + eps) * sqrt(k + 1) is formed natively in double); ema (optional): the moving average of the updated parameters,
    advanced in the same kernel (mi355_madgrad_step_ema)"""
    _ema_step("madgrad_step", "p g grad_sum_sq s x0 ema", (p, g, grad_sum_sq, s, x0),
              (float(lr), float(momentum), float(weight_decay), float(eps), int(k), float(grad_scale)), ema, ema_decay)


def adais_workspace_elems(n):
    """the number of float64 partial sums adais_moments writes for a range of n elements"""
    return _L().mi355_adais_workspace_bytes(int(n)) // 8


def adais_moments(g, v, step, beta2, workspace, grad_scale=1.0):
    """AdaiS stage (a): v = v*beta2 + (1 - beta2)*g*g in place and the per-workgroup sums of v / (1 - beta2^step) into `workspace`
    (float64, adais_workspace_elems(n) elements); step: the range's count after this step's increment"""
    n = _flat("adais_moments", "v g", v, g)
    _arg("adais_moments", "workspace", _F64, adais_workspace_elems(n), workspace)
    _on_device("adais_moments", "g v workspace", g, v, workspace)
    check(_L().mi355_adais_moments(ptr(g), ptr(v), n, float(beta2), int(step), float(grad_scale), ptr(workspace), cur_stream()))


def adais_mean(workspace, param_size, mean):
    """AdaiS stage (b): mean[0] = sum(workspace) / param_size, summed in a fixed order on the device (workspace: the float64 partial sums
    of every range, back to back; mean: a float32 CUDA tensor of one element)"""
    _arg("adais_mean", "workspace", _F64, (None,), workspace)
    _arg("adais_mean", "mean", _F32, 1, mean)
    _on_device("adais_mean", "workspace mean", workspace, mean)
    check(_L().mi355_adais_mean(ptr(workspace), workspace.numel() * 8, int(param_size), ptr(mean), cur_stream()))


def adais_step(p, g, m, v, beta1_prod, mean, step, lr, betas=(0.1, 0.99), eps=1e-3, weight_decay=0.0, grad_scale=1.0, ema=None, ema_decay=0.0):
    """AdaiS stage (c): the parameter update of a flat range from the device-resident mean of stage (b); ema (optional): the moving average
    of the updated parameters, advanced in the same kernel (mi355_adais_step_ema)"""
    _arg("adais_step", "mean", _F32, 1, mean)
    _ema_step("adais_step", "p g m v beta1_prod mean ema", (p, g, m, v, beta1_prod),
              (float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale)), ema, ema_decay,
              then=(mean,))


# ---- layer-wise optimizers (include/mi355rn.h, csrc/optim_lw.hip): MyNovograd, NovogradApex, AdamLayerwise, MyAdai of the reference ------
LW_NORMGRAD, LW_NOVOGRAD, LW_ADAI = 0, 1, 2  # the element rule: AdamLayerwise / NovogradApex, MyNovograd, MyAdai
LW_MEAN, LW_STABLE_WD, LW_SOFT_WD, LW_SGD_MOM, LW_SQRT_MOM = 1, 2, 4, 8, 16
_REC16 = (None, 2)  # a table of 16-byte records as pack_records leaves it: int64 [n, 2], n >= 1


def lw_item_elems():
    """W: the most elements one work item (= one workgroup) covers"""
    return int(_L().mi355_lw_item_elems())


def lw_sumsq(src, items, partial, n_tensors, scale=1.0):
    """stage (a), replaces the per-tensor grad.pow(2).sum() / .mean() of sota_imagenet/optimizers.py:138, :270, :369, :488:
    partial[i] = sum over work item i of (src * scale)^2 in double; src: the flat fp32 array the item offsets count from"""
    _arg("lw_sumsq", "src", _F32, None, src)
    _arg("lw_sumsq", "items", _I64, _REC16, items)
    _arg("lw_sumsq", "partial", _F64, items.shape[0], partial)
    _on_device("lw_sumsq", "src items partial", src, items, partial)
    check(_L().mi355_lw_sumsq(ptr(src), src.numel(), ptr(items), items.shape[0], int(n_tensors), float(scale), ptr(partial), cur_stream()))


def lw_coef(rule, flags, partial, tensors, v, coef, sums, beta1, beta2, eps, lr, weight_decay, mean=1.0):
    """stage (b), replaces optimizers.py:140-146, :273-274, :370-371, :489-501 for the tensors of one param group: sums[t] = the tensor's
    partials in a fixed order, v (float32 per tensor, updated in place; LW_ADAI: float64, read only) and coef[t] = (den, beta1, gw, wdf).
    partial: the WHOLE float64 array; tensors, v, coef (four float32 per tensor), sums (float64): the group's slices"""
    _arg("lw_coef", "tensors", _I64, _REC16, tensors)
    nt = tensors.shape[0]
    _arg("lw_coef", "partial", _F64, (None,), partial)
    _arg("lw_coef", "v", _F64 if rule == LW_ADAI else _F32, nt, v)
    _arg("lw_coef", "coef", _F32, 4 * nt, coef)
    _arg("lw_coef", "sums", _F64, nt, sums)
    _on_device("lw_coef", "partial tensors v coef sums", partial, tensors, v, coef, sums)
    check(_L().mi355_lw_coef(int(rule), int(flags), ptr(partial), partial.numel(), ptr(tensors), nt, ptr(v), ptr(coef), ptr(sums), float(beta1),
                             float(beta2), float(eps), float(lr), float(weight_decay), float(mean), cur_stream()))


def lw_update(rule, p, g, m, items, coef, lr, wd_eps=None, grad_scale=1.0, ema=None, ema_decay=0.0):
    """stage (c), replaces optimizers.py:144-159, :277-288, :374-391, :504-517 for the work items of one param group; p, g, m (and ema): the
    flat fp32 arrays the item offsets count from; coef: the whole [n_tensors, 4] table of stage (b)"""
    _arg("lw_update", "items", _I64, _REC16, items)
    _arg("lw_update", "coef", _F32, (None, 4), coef)
    _ema_step("lw_update", "p g m items coef ema", (p, g, m),
              (ptr(items), items.shape[0], ptr(coef), coef.shape[0], float(lr), int(wd_eps is not None), float(wd_eps or 0.0), float(grad_scale)),
              ema, ema_decay, lead=(int(rule),), others=(items, coef))


# ---- unitwise_norm=True of MyNovograd / NovogradApex (include/mi355rn.h, csrc/optim_lw.hip): one norm per slot ----------------------------------
def lw_unit_sumsq(src, pieces, partial, n_slots, scale=1.0):
    """stage (a), the per-output-unit sums behind unitwise_norm of sota_imagenet/optimizers.py:22: partial[i] = sum over piece i { off, len, slot }
    of (src * scale)^2 in double, a piece cut from one unit at any element offset; one wave per piece"""
    _arg("lw_unit_sumsq", "src", _F32, None, src)
    _arg("lw_unit_sumsq", "pieces", _I64, _REC16, pieces)
    _arg("lw_unit_sumsq", "partial", _F64, pieces.shape[0], partial)
    _on_device("lw_unit_sumsq", "src pieces partial", src, pieces, partial)
    check(_L().mi355_lw_unit_sumsq(ptr(src), src.numel(), ptr(pieces), pieces.shape[0], int(n_slots), float(scale), ptr(partial), cur_stream()))


def lw_unit_coef(partial, slots, v, den, sums, beta2, eps):
    """stage (b), replaces optimizers.py:134-146 and :267-274 for the slots of one param group: sums[s] = the slot's entries of partial[] (the
    WHOLE array) in a fixed order; v[s] = v[s]*beta2 + (1 - beta2)*sqrt(sums[s]), float32 in place; den[s] = sqrt(v[s]) + eps.  slots: CUDA int32
    [n, 2] of (first, count); v, den, sums: the group's slices, one element per slot"""
    _arg("lw_unit_coef", "slots", _I32, (None, 2), slots)
    ns = slots.shape[0]
    _arg("lw_unit_coef", "partial", _F64, (None,), partial)
    _arg("lw_unit_coef", "v den", _F32, ns, v, den)
    _arg("lw_unit_coef", "sums", _F64, ns, sums)
    _on_device("lw_unit_coef", "partial slots v den sums", partial, slots, v, den, sums)
    check(_L().mi355_lw_unit_coef(ptr(partial), partial.numel(), ptr(slots), ns, ptr(v), ptr(den), ptr(sums), float(beta2), float(eps), cur_stream()))


def lw_unit_update(rule, p, g, m, items, tensors, den, beta1, lr, weight_decay, wd_eps=None, grad_scale=1.0, ema=None, ema_decay=0.0):
    """stage (c), replaces optimizers.py:144-159 and :277-288 for the work items of one param group; p, g, m (and ema): the flat fp32 arrays the
    item offsets count from; tensors: the records { start, unit_len, slot0 } of ALL tensors; den: the whole per-slot array of stage (b)"""
    _arg("lw_unit_update", "items tensors", _I64, _REC16, items, tensors)
    _arg("lw_unit_update", "den", _F32, (None,), den)
    _ema_step("lw_unit_update", "p g m items tensors den ema", (p, g, m),
              (ptr(items), items.shape[0], ptr(tensors), tensors.shape[0], ptr(den), den.numel(), float(beta1), float(lr), float(weight_decay),
               int(wd_eps is not None), float(wd_eps or 0.0), float(grad_scale)),
              ema, ema_decay, lead=(int(rule),), others=(items, tensors, den))


# ---- AdamP (include/mi355rn.h, csrc/optim_adamp.hip): Adam with the projection of adamp.AdamP, restated from the published package --------------
def adamp_unit_sums(p, g, m, v, pieces, partial, n_slots, step, betas=(0.9, 0.999), eps=1e-8, nesterov=False, grad_scale=1.0):
    """stage (a): partial[k] = (sum ge^2, sum p^2, sum ge*p, sum p*u) over piece k { off, len, slot }, in double, ge = g*grad_scale and u the Adam
    direction of this step formed in registers from the OLD m and v (neither is written); step: the count after this step's increment;
    partial: float64 [n_pieces, 4]"""
    n = _flat("adamp_unit_sums", "p g m v", p, g, m, v)
    _arg("adamp_unit_sums", "pieces", _I64, _REC16, pieces)
    _arg("adamp_unit_sums", "partial", _F64, 4 * pieces.shape[0], partial)
    _on_device("adamp_unit_sums", "p g m v pieces partial", p, g, m, v, pieces, partial)
    check(_L().mi355_adamp_unit_sums(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(pieces), pieces.shape[0], int(n_slots), float(betas[0]),
                                     float(betas[1]), float(eps), int(step), int(bool(nesterov)), float(grad_scale), ptr(partial), cur_stream()))


def adamp_coef(partial, slots, decide, coef, wdf, mode, lr, weight_decay, eps=1e-8, delta=0.1, wd_ratio=0.1):
    """stage (b) for the tensors of one param group: decide = their records { slot0, n_slots, unit_len, kind } (CUDA int32 [n, 4]); partial
    (float64 [entries, 4]), slots (int32 [n_slots, 2]) and coef (float32 [n_slots, 2]) are the WHOLE arrays, wdf (float32) and mode (int32) the
    group's slices.  Writes coef[slot] = (d, s), wdf[t] and mode[t] (0: none, 1: the units, 2: the layer)"""
    _arg("adamp_coef", "slots", _I32, (None, 2), slots)
    _arg("adamp_coef", "decide", _I32, (None, 4), decide)
    nt = decide.shape[0]
    _arg("adamp_coef", "partial", _F64, (None, 4), partial)
    _arg("adamp_coef", "coef", _F32, (slots.shape[0], 2), coef)
    _arg("adamp_coef", "wdf", _F32, (nt,), wdf)
    _arg("adamp_coef", "mode", _I32, nt, mode)
    _on_device("adamp_coef", "partial slots decide coef wdf mode", partial, slots, decide, coef, wdf, mode)
    check(_L().mi355_adamp_coef(ptr(partial), partial.shape[0], ptr(slots), slots.shape[0], ptr(decide), nt, ptr(coef), ptr(wdf), ptr(mode),
                                float(lr), float(weight_decay), float(eps), float(delta), float(wd_ratio), cur_stream()))


def adamp_update(p, g, m, v, items, tensors, coef, wdf, step, lr, betas=(0.9, 0.999), eps=1e-8, nesterov=False, grad_scale=1.0, ema=None,
                 ema_decay=0.0):
    """stage (c) for the work items of one param group; p, g, m, v (and ema): the flat fp32 arrays the item offsets count from; tensors: the
    records { start, unit_len, slot0 } of ALL tensors; coef [n_slots, 2] and wdf [n_tensors]: the whole arrays of stage (b)"""
    _arg("adamp_update", "items tensors", _I64, _REC16, items, tensors)
    _arg("adamp_update", "coef", _F32, (None, 2), coef)
    _arg("adamp_update", "wdf", _F32, (tensors.shape[0],), wdf)
    _ema_step("adamp_update", "p g m v items tensors coef wdf ema", (p, g, m, v),
              (ptr(items), items.shape[0], ptr(tensors), tensors.shape[0], ptr(coef), coef.shape[0], ptr(wdf), float(lr), float(betas[0]),
               float(betas[1]), float(eps), int(step), int(bool(nesterov)), float(grad_scale)),
              ema, ema_decay, others=(items, tensors, coef, wdf))


# ---- sharpness-aware minimization (include/mi355rn.h, csrc/optim_sam.hip): the SAMOriginal callback of the reference -----------------------
def sam_sumsq(p, g, items, kind, partial, eta, grad_scale=1.0):
    """stage (a), replaces the per-tensor norms of sota_imagenet/callbacks.py:327-337: partial[i] = sum over work item i of w^2 in double,
    w = (g*grad_scale) * max(|p|, eta) for tensors with kind 1 and g*grad_scale for the others; p, g: the flat fp32 arrays the offsets count from;
    kind: int32, one element per tensor"""
    n = _flat("sam_sumsq", "p g", p, g)
    _arg("sam_sumsq", "items", _I64, _REC16, items)
    _arg("sam_sumsq", "kind", _I32, (None,), kind)
    _arg("sam_sumsq", "partial", _F64, items.shape[0], partial)
    _on_device("sam_sumsq", "p g items kind partial", p, g, items, kind, partial)
    check(_L().mi355_sam_sumsq(ptr(p), ptr(g), n, ptr(items), items.shape[0], ptr(kind), kind.numel(), float(eta), float(grad_scale), ptr(partial),
                               cur_stream()))


def sam_scale(partial, rho, out):
    """stage (b), replaces callbacks.py:337 and :297: norm = max(sqrt(sum(partial)), 2e-5) in double over ALL partials of the step;
    out[0] = rho / norm, out[1] = norm (a float32 CUDA tensor of two elements)"""
    _arg("sam_scale", "partial", _F64, (None,), partial)
    _arg("sam_scale", "out", _F32, 2, out)
    _on_device("sam_scale", "partial out", partial, out)
    check(_L().mi355_sam_scale(ptr(partial), partial.numel(), float(rho), ptr(out), cur_stream()))


def sam_perturb(p, g, eps, items, kind, out, eta, grad_scale=1.0):
    """stage (c), replaces callbacks.py:298-306: eps = (max(p*p, eta) * g*grad_scale) * out[0] for kind 1, (g*grad_scale) * out[0] otherwise;
    p += eps.  eps: a flat fp32 array laid out like p; out: the two float32 elements sam_scale wrote"""
    n = _flat("sam_perturb", "p g eps", p, g, eps)
    _arg("sam_perturb", "items", _I64, _REC16, items)
    _arg("sam_perturb", "kind", _I32, (None,), kind)
    _arg("sam_perturb", "out", _F32, 2, out)
    _on_device("sam_perturb", "p g eps items kind out", p, g, eps, items, kind, out)
    check(_L().mi355_sam_perturb(ptr(p), ptr(g), ptr(eps), n, ptr(items), items.shape[0], ptr(kind), kind.numel(), ptr(out), float(eta),
                                 float(grad_scale), cur_stream()))


def sam_restore(p, eps, items, n_tensors):
    """stage (d), replaces callbacks.py:319-323: p -= eps over the same work items"""
    n = _flat("sam_restore", "p eps", p, eps)
    _arg("sam_restore", "items", _I64, _REC16, items)
    _on_device("sam_restore", "p eps items", p, eps, items)
    check(_L().mi355_sam_restore(ptr(p), ptr(eps), n, ptr(items), items.shape[0], int(n_tensors), cur_stream()))


# ---- the SAM callback of the reference (include/mi355rn.h, csrc/optim_sam_lw.hip): one pair of norms per slot -----------------------------------
SAM_THREADS_PER_PIECE = 64  # one wave per piece: profiles/sam_lw_step.json


def sam_lw_sumsq(p, g, items, partial, n_tensors, grad_scale=1.0):
    """stage (a), the whole-tensor norms of sota_imagenet/callbacks.py:389-391: partial[i] = (sum of (g*grad_scale)^2, sum of p^2) over work item
    i, in double (a pair of float64 per item); p, g: the flat fp32 arrays the offsets count from"""
    n = _flat("sam_lw_sumsq", "p g", p, g)
    _arg("sam_lw_sumsq", "items", _I64, _REC16, items)
    _arg("sam_lw_sumsq", "partial", _F64, 2 * items.shape[0], partial)
    _on_device("sam_lw_sumsq", "p g items partial", p, g, items, partial)
    check(_L().mi355_sam_lw_sumsq(ptr(p), ptr(g), n, ptr(items), items.shape[0], int(n_tensors), float(grad_scale), ptr(partial), cur_stream()))


def sam_unit_sumsq(p, g, pieces, partial, n_slots, grad_scale=1.0, threads_per_piece=SAM_THREADS_PER_PIECE):
    """stage (a'), the per-output-unit norms of callbacks.py:269-276, :386-387: the same pair of sums over every piece { off, len, slot } of
    `pieces`, a piece cut from one unit at any element offset; one wave (threads_per_piece 64) or one workgroup (256) per piece"""
    n = _flat("sam_unit_sumsq", "p g", p, g)
    _arg("sam_unit_sumsq", "pieces", _I64, _REC16, pieces)
    _arg("sam_unit_sumsq", "partial", _F64, 2 * pieces.shape[0], partial)
    _on_device("sam_unit_sumsq", "p g pieces partial", p, g, pieces, partial)
    check(_L().mi355_sam_unit_sumsq(ptr(p), ptr(g), n, ptr(pieces), pieces.shape[0], int(n_slots), float(grad_scale), ptr(partial),
                                    int(threads_per_piece), cur_stream()))


def sam_lw_coef(partial, slots, coef, norms):
    """stage (b), callbacks.py:386-395 for every slot: (Sg, Sp) = the slot's entries of partial[] in a fixed order; gn = max(sqrt(Sg), 1e-5),
    wn = max(sqrt(Sp), 1e-3) in float32; coef[slot] = wn / gn, norms[slot] = (gn, wn).  slots: CUDA int32 [n_slots, 2] of (first, count);
    partial: the flat float64 array of whole pairs; coef: float32 [n_slots], norms: two float32 per slot"""
    _arg("sam_lw_coef", "partial", _F64, (None,), partial)
    _arg("sam_lw_coef", "partial[pairs]", _F64, max(2, partial.numel() // 2 * 2), partial)
    _arg("sam_lw_coef", "slots", _I32, (None, 2), slots)
    ns = slots.shape[0]
    _arg("sam_lw_coef", "coef", _F32, (ns,), coef)
    _arg("sam_lw_coef", "norms", _F32, 2 * ns, norms)
    _on_device("sam_lw_coef", "partial slots coef norms", partial, slots, coef, norms)
    check(_L().mi355_sam_lw_coef(ptr(partial), partial.numel() // 2, ptr(slots), ns, ptr(coef), ptr(norms), cur_stream()))


def sam_lw_perturb(p, g, eps, items, tensors, coef, rho, grad_scale=1.0):
    """stage (c), callbacks.py:395-404: eps = (coef[slot] * (g*grad_scale)) * rho, p += eps over the work items of all tensors; the slot of an
    element from its tensor's record { start, unit_len, slot0 } in `tensors`.  eps: a flat fp32 array laid out like p; coef: float32 [n_slots]"""
    n = _flat("sam_lw_perturb", "p g eps", p, g, eps)
    _arg("sam_lw_perturb", "items tensors", _I64, _REC16, items, tensors)
    _arg("sam_lw_perturb", "coef", _F32, (None,), coef)
    _on_device("sam_lw_perturb", "p g eps items tensors coef", p, g, eps, items, tensors, coef)
    check(_L().mi355_sam_lw_perturb(ptr(p), ptr(g), ptr(eps), n, ptr(items), items.shape[0], ptr(tensors), tensors.shape[0], ptr(coef),
                                    coef.numel(), float(rho), float(grad_scale), cur_stream()))


# ---- orthogonal initialisation (include/mi355rn.h, csrc/init_ortho.hip): the OrthoInitClb callback of the reference ---------------------------------
def ortho_init_(flat, records_host, records_dev, gain=1.0):
    """replaces the nn.init.orthogonal_ calls of sota_imagenet/callbacks.py:260-265: every matrix of the table, filled with N(0,1) draws by the
    caller, becomes in place the sign-fixed Q of its QR factorisation times gain.  flat: the fp32 array the offsets count from; records_host:
    [(off, rows, chans, taps)] (item_plan.ortho_records), records_dev: the same table packed for the device (item_plan.pack_records with
    ORTHO_FIELDS, CUDA int64 [n, 3]).  Records that overlap would race and raise here; one that does not fit the array is the kernel's to refuse.
    Returns status (CUDA int32 per record: 0 done, 1 rank-deficient input, 2 the record does not fit), not read back."""
    n_mats = len(records_host)
    _arg("ortho_init_", "flat", _F32, None, flat)
    _arg("ortho_init_", "records_dev", _I64, (None, 3), records_dev)
    if records_dev.shape[0] != n_mats:
        raise ValueError(f"ortho_init_: records_dev holds {records_dev.shape[0]} records, records_host {n_mats}")
    dev = _on_device("ortho_init_", "flat records_dev", flat, records_dev)
    _check_disjoint("ortho_init_: the record", ((off, max(rows, 0) * max(chans, 0) * max(taps, 0)) for off, rows, chans, taps in sorted(records_host)))
    status = torch.empty(n_mats, dtype=_I32, device=dev)
    check(_L().mi355_ortho_init(ptr(flat), flat.numel(), ptr(records_dev), n_mats, float(gain), ptr(status), cur_stream()))
    return status


# ---- backward centred weight normalisation (include/mi355rn.h, csrc/weight_norm.hip): the WeightNorm callback of the reference ----------------------
# stated once for the host; csrc/weight_norm.hip states the first for the kernel (mi355_wnorm_wave_row_max) and tests/test_weight_norm_host.py holds
# the two together
WNORM_WAVE_ROW_MAX = 1024  # rows up to this length take one wave, four rows at a time; longer rows the whole workgroup
WNORM_ITEM_ELEMS = 4096    # W: an item holds max(1, W // row_len) rows (item_plan.wnorm_items).  Host side only: the kernel takes any n_rows


def wnorm_check_items(items_host):
    """ValueError if two of the items [(first, row_len, n_rows)] overlap: two workgroups would rewrite the same elements"""
    _check_disjoint("weight_norm_rows_: the item", ((first, max(row_len, 0) * max(n_rows, 0)) for first, row_len, n_rows in sorted(items_host)))


def weight_norm_rows_(flat, items_host, items_dev):
    """replaces the loop of sota_imagenet/callbacks.py:116-123: every row of the table is centred on its mean and scaled to unit L2 norm, in place
    and in ONE launch.  flat: the fp32 array the offsets count from; items_host: [(first element, row_len, n_rows)] (item_plan.wnorm_items),
    items_dev: the same table packed for the device (item_plan.pack_records, CUDA int64 [n, 2]).  Items that overlap would race and raise here
    (wnorm_check_items); a caller that launches one table every step checks it once and passes items_host=None afterwards.  An item that does
    not fit the array is the kernel's to refuse.  Returns status (CUDA int32 per item: 0 done, 2 the item does not fit), not read back."""
    _arg("weight_norm_rows_", "flat", _F32, None, flat)
    _arg("weight_norm_rows_", "items_dev", _I64, _REC16, items_dev)
    if items_host is not None and len(items_host) != items_dev.shape[0]:
        raise ValueError(f"weight_norm_rows_: items_dev holds {items_dev.shape[0]} records, items_host {len(items_host)}")
    dev = _on_device("weight_norm_rows_", "flat items_dev", flat, items_dev)
    if items_host is not None:
        wnorm_check_items(items_host)
    status = torch.empty(items_dev.shape[0], dtype=_I32, device=dev)
    check(_L().mi355_weight_norm_rows(ptr(flat), flat.numel(), ptr(items_dev), items_dev.shape[0], ptr(status), cur_stream()))
    return status


# ---- forward weight transform per filter (include/mi355rn.h, csrc/weight_std.hip): weight_standardization / the ForwardWeightNorm callback ---------
# stated once for the host; include/mi355rn.h states them for the library (MI355_WS_*) and tests/test_weight_std_host.py holds the two together
WS_STANDARDISE, WS_CENTRE = 1, 2
WS_EPS = 1e-5  # oracle/bresnet50_ref.py::ws

def _ws_args(who, names, rows_dev, invstd, *arrays):
    """names: those of the flat arrays"""
    n = _flat(who, names, *arrays)
    _arg(who, "rows_dev", _I64, _REC16, rows_dev)
    _arg(who, "invstd", _F32, rows_dev.shape[0], invstd)
    _on_device(who, "rows_dev invstd " + names, rows_dev, invstd, *arrays)
    return n


def weight_std_rows_fwd(w, w_hat, invstd, rows_dev, mode, eps=WS_EPS):
    """w_hat = the per-row transform of w (mode WS_STANDARDISE: (w - mean) / sqrt(var + eps), WS_CENTRE: w - mean), invstd[k] = row k's factor,
    in ONE launch.  w, w_hat: flat fp32 arrays of one size the row offsets count from — the same tensor bakes the transform in place —;
    rows_dev: [(first element, row_len)] packed for the device (item_plan.ws_rows, pack_records; CUDA int64 [n, 2]); a row that does not fit
    the array is skipped by the kernel.  Elements outside the rows are neither read nor written."""
    n = _ws_args("weight_std_rows_fwd", "w w_hat", rows_dev, invstd, w, w_hat)
    check(_L().mi355_weight_std_rows_fwd(ptr(w), ptr(w_hat), ptr(invstd), n, ptr(rows_dev), rows_dev.shape[0], int(mode), float(eps), cur_stream()))


def weight_std_rows_bwd(g, w_hat, invstd, dw, rows_dev, mode, beta=0.0, row_begin=0, row_end=None):
    """dw = beta * dw + (the gradient wrt w of the rows [row_begin, row_end) of the table, from g = the gradient wrt w_hat), in ONE launch:
    invstd * (g - mean(g) - w_hat * mean(g * w_hat)) per row (WS_CENTRE: invstd * (g - mean(g)), invstd as the forward left it: 1)"""
    n = _ws_args("weight_std_rows_bwd", "g w_hat dw", rows_dev, invstd, g, w_hat, dw)
    row_end = rows_dev.shape[0] if row_end is None else int(row_end)
    if not 0 <= int(row_begin) < row_end <= rows_dev.shape[0]:
        raise ValueError(f"weight_std_rows_bwd: rows [{row_begin}, {row_end}) of a table of {rows_dev.shape[0]}")
    check(_L().mi355_weight_std_rows_bwd(ptr(g), ptr(w_hat), ptr(invstd), ptr(dw), n, ptr(rows_dev), int(row_begin), row_end, int(mode), float(beta),
                                         cur_stream()))


# ---- forward spectral normalisation per convolution (include/mi355rn.h, csrc/spectral_norm.hip): the ForwardSpectralNorm callback -------------------
# stated once for the host; include/mi355rn.h states them for the library (MI355_SN_*) and tests/test_spectral_host.py holds the two together
SN_EPS = 1e-12  # torch.nn.utils.parametrizations.spectral_norm's eps (rounded to float32 where it is used)
SN_WARM_ITERS = 15  # the power iterations torch runs at registration
SN_SLABS = 16  # row slabs per matrix of the column sums: the scratch holds one partial sum per slab and element of v


def spectral_scratch(u, v):
    """the float64 scratch spectral_fwd / spectral_bwd need for vectors of these sizes, on their device"""
    return torch.empty(_L().mi355_spectral_scratch_doubles(u.numel(), v.numel()), dtype=_F64, device=u.device)


def _sn_args(who, names, mats_dev, u, v, sigma, scratch, *arrays):
    """names: those of the flat arrays"""
    n = _flat(who, names, *arrays)
    _arg(who, "mats_dev", _I64, (None, 4), mats_dev)
    _arg(who, "u v", _F32, (None,), u, v)
    _arg(who, "sigma", _F32, mats_dev.shape[0], sigma)
    _arg(who, "scratch", _F64, _L().mi355_spectral_scratch_doubles(u.numel(), v.numel()), scratch)
    _on_device(who, "mats_dev u v sigma scratch " + names, mats_dev, u, v, sigma, scratch, *arrays)
    return n


def spectral_fwd(w, w_hat, u, v, sigma, scratch, mats_dev, iters):
    """`iters` power iterations of every matrix of the table on (u, v) — 1: a training forward; 0: the eval rule, u and v untouched —, sigma[i] of
    matrix i, and, unless w_hat is None, w_hat = w / sigma (w_hat is w: in place).  w, w_hat: flat fp32 arrays of one size the offsets count
    from; mats_dev: item_plan.spectral_mats packed with SPECTRAL_FIELDS (CUDA int64 [n, 4]); u, v: the sizes spectral_mats returns.  A matrix
    that does not fit the arrays is skipped by the kernels; elements outside the matrices are neither read nor written."""
    n = _sn_args("spectral_fwd", "w w_hat", mats_dev, u, v, sigma, scratch, *((w,) if w_hat is None else (w, w_hat)))
    check(_L().mi355_spectral_fwd(ptr(w), ptr(w_hat), ptr(u), ptr(v), ptr(sigma), ptr(scratch), n, u.numel(), v.numel(), ptr(mats_dev),
                                  mats_dev.shape[0], int(iters), cur_stream()))


def spectral_bwd(g, w_hat, u, v, sigma, dw, scratch, mats_dev, beta=0.0, row_begin=0, row_end=None):
    """dw = beta * dw + (the gradient wrt w, from g = the gradient wrt w_hat = w / sigma with u, v, sigma constants) for the matrices whose rows
    are the slice [row_begin, row_end) of u — whole matrices —: (g - (sum g * w_hat) * u_r * v_c) / sigma"""
    n = _sn_args("spectral_bwd", "g w_hat dw", mats_dev, u, v, sigma, scratch, g, w_hat, dw)
    row_end = u.numel() if row_end is None else int(row_end)
    if not 0 <= int(row_begin) < row_end <= u.numel():
        raise ValueError(f"spectral_bwd: rows [{row_begin}, {row_end}) of u[{u.numel()}]")
    check(_L().mi355_spectral_bwd(ptr(g), ptr(w_hat), ptr(u), ptr(v), ptr(sigma), ptr(dw), ptr(scratch), n, u.numel(), v.numel(), ptr(mats_dev),
                                  mats_dev.shape[0], int(row_begin), row_end, float(beta), cur_stream()))


# ---- weight penalties in the loss (include/mi355rn.h, csrc/ortho_loss.hip): the OrthoLossClb and NormLossClb callbacks of the reference -------------
# stated once for the host; include/mi355rn.h states the first two for the library (MI355_OL_*) and tests/test_ortho_loss_host.py holds them together
OL_TILE = 64    # rows and columns of a Gram tile; columns of K per gradient item
OL_KSLAB = 512  # elements of K per Gram item
NL_ITEM_ELEMS = 16384  # W of the norm penalty's items (item_plan.norm_loss_items).  Host side only: the kernels take any run of whole rows
_OL_TABLES = (("mats", 4), ("tiles", 2), ("items", 1), ("gitems", 2))  # int64 columns of the packed records


def ortho_loss_scratch(n_gram, n_mats, n_tiles, n_items, device):
    """what ortho_loss_fwd leaves and ortho_loss_bwd reads, on `device`: gram (every G, fp32), partial (the slab partials), tile_ss (float64 per
    tile), stats ([n_mats, 4]: F, F / O, gate, coefficient) and loss (the 0-dim fp32 total)"""
    L = _L()
    return dict(gram=torch.empty(n_gram, dtype=_F32, device=device),
                partial=torch.empty(L.mi355_ortho_loss_partial_floats(n_items), dtype=_F32, device=device),
                tile_ss=torch.empty(n_tiles, dtype=_F64, device=device),
                stats=torch.empty(L.mi355_ortho_loss_stats_floats(n_mats) // 4, 4, dtype=_F32, device=device),
                loss=torch.empty((), dtype=_F32, device=device))


def _ol_args(who, names, tables, scratch, s, *arrays):
    """tables and scratch by their keys: the packed int64 records, and what ortho_loss_scratch allocates for them; s: tested by the caller;
    names: those of the flat arrays"""
    n = _flat(who, names, *arrays)
    for name, cols in _OL_TABLES:
        _arg(who, name, _I64, (None, cols), tables[name])
    L = _L()
    n_mats, n_tiles, n_items = (tables[k].shape[0] for k in ("mats", "tiles", "items"))
    _arg(who, "gram", _F32, (None,), scratch["gram"])
    _arg(who, "partial", _F32, L.mi355_ortho_loss_partial_floats(n_items), scratch["partial"])
    _arg(who, "tile_ss", _F64, n_tiles, scratch["tile_ss"])
    _arg(who, "stats", _F32, L.mi355_ortho_loss_stats_floats(n_mats), scratch["stats"])
    _arg(who, "loss", _F32, 1, scratch["loss"])
    _on_device(who, "mats tiles items gitems gram partial tile_ss stats loss s " + names, *(tables[k] for k, _ in _OL_TABLES),
               *(scratch[k] for k in ("gram", "partial", "tile_ss", "stats", "loss")), s, *arrays)
    return n


def ortho_loss_fwd(w, tables, scratch, min_norm):
    """replaces the loop of sota_imagenet/callbacks.py:138-156 in 3 launches: for every matrix of the tables G = W W^T - I (scratch["gram"]), its
    Frobenius norm F, the gate F / O > min_norm and the gradient's coefficient (scratch["stats"]), and scratch["loss"] = sum of the gated F, which
    is returned (a view, not read back).  w: the flat fp32 array the offsets count from; tables: item_plan.ortho_loss_cut(.., OL_TILE, OL_KSLAB)
    packed for the device — mats (ORTHO_LOSS_FIELDS), tiles and gitems (OL_TILE_FIELDS), items (OL_ITEM_FIELDS).  A record that does not fit is
    skipped by the kernels; elements outside the matrices are not read."""
    n = _ol_args("ortho_loss_fwd", "w", tables, scratch, None, w)
    s = scratch
    check(_L().mi355_ortho_loss_fwd(ptr(w), n, ptr(s["gram"]), s["gram"].numel(), ptr(s["partial"]), ptr(s["tile_ss"]), ptr(s["stats"]), ptr(s["loss"]),
                                    ptr(tables["mats"]), tables["mats"].shape[0], ptr(tables["tiles"]), tables["tiles"].shape[0],
                                    ptr(tables["items"]), tables["items"].shape[0], float(min_norm), cur_stream()))
    return s["loss"]


def ortho_loss_bwd(w, dw, tables, scratch, s, accumulate=True):
    """dw (+)= s * (2 / F) G W for every matrix whose gate ortho_loss_fwd left open, in ONE launch, from the gram and stats it left in `scratch`;
    s: a 1-element CUDA fp32 tensor (the upstream gradient times the callback's weight: it stays on the device); accumulate=False overwrites the
    matrices' elements (zeros where the gate is closed) and leaves every other element of dw alone."""
    _arg("ortho_loss_bwd", "s", _F32, 1, s)
    n = _ol_args("ortho_loss_bwd", "w dw", tables, scratch, s, w, dw)
    check(_L().mi355_ortho_loss_bwd(ptr(w), ptr(dw), n, ptr(scratch["gram"]), scratch["gram"].numel(), ptr(scratch["stats"]), ptr(s),
                                    ptr(tables["mats"]), tables["mats"].shape[0], tables["tiles"].shape[0], ptr(tables["gitems"]),
                                    tables["gitems"].shape[0], int(bool(accumulate)), cur_stream()))


def norm_loss_scratch(n_items, n_tensors, device):
    """what norm_loss_fwd leaves: part (float64 per item), tensor_loss (float64 per tensor: its mean) and loss (the 0-dim fp32 total)"""
    return dict(part=torch.empty(n_items, dtype=_F64, device=device), tensor_loss=torch.empty(n_tensors, dtype=_F64, device=device),
                loss=torch.empty((), dtype=_F32, device=device))

def _nl_args(who, names, items_dev, tensors_dev, *arrays):
    n = _flat(who, names, *arrays)
    _arg(who, "items_dev tensors_dev", _I64, _REC16, items_dev, tensors_dev)
    return n


def norm_loss_fwd(w, items_dev, tensors_dev, scratch):
    """replaces the loop of sota_imagenet/callbacks.py:213-221 in 2 launches: scratch["loss"] = sum over the tensors of mean_r (1 - |row r|)^2,
    which is returned (a view, not read back).  items_dev, tensors_dev: item_plan.norm_loss_items packed for the device (CUDA int64 [n, 2]);
    scratch: what norm_loss_scratch allocates for them."""
    n = _nl_args("norm_loss_fwd", "w", items_dev, tensors_dev, w)
    part, tensor_loss, loss = scratch["part"], scratch["tensor_loss"], scratch["loss"]
    _arg("norm_loss_fwd", "part", _F64, items_dev.shape[0], part)
    _arg("norm_loss_fwd", "tensor_loss", _F64, tensors_dev.shape[0], tensor_loss)
    _arg("norm_loss_fwd", "loss", _F32, 1, loss)
    _on_device("norm_loss_fwd", "w items_dev tensors_dev part tensor_loss loss", w, items_dev, tensors_dev, part, tensor_loss, loss)
    check(_L().mi355_norm_loss_fwd(ptr(w), n, ptr(part), ptr(tensor_loss), ptr(loss), ptr(items_dev), items_dev.shape[0], ptr(tensors_dev),
                                   tensors_dev.shape[0], cur_stream()))
    return loss


def norm_loss_bwd(w, dw, items_dev, tensors_dev, s, accumulate=True):
    """dw (+)= s * (2 / R)(n_r - 1) / n_r * w for every row of the tables (0 where n_r == 0), in ONE launch; s as in ortho_loss_bwd"""
    n = _nl_args("norm_loss_bwd", "w dw", items_dev, tensors_dev, w, dw)
    _arg("norm_loss_bwd", "s", _F32, 1, s)
    _on_device("norm_loss_bwd", "w dw items_dev tensors_dev s", w, dw, items_dev, tensors_dev, s)
    check(_L().mi355_norm_loss_bwd(ptr(w), ptr(dw), n, ptr(s), ptr(items_dev), items_dev.shape[0], ptr(tensors_dev), tensors_dev.shape[0],
                                   int(bool(accumulate)), cur_stream()))


# ---- the log histogram of |x| (include/mi355rn.h, csrc/optim_hist.hip): the GradDistributionTB callback of the reference ----------------------------
# the bins, stated once for the host; csrc/absbin.h states them for the kernels and tests/test_grad_dist_host.py holds the two together
ABSBIN_BINS, ABSBIN_SHIFT, ABSBIN_K0 = 512, 20, (77 << 3) + 2
ABSBIN_BAD_REP = 2 ** 64 - 1  # what mi355_subsample_counts writes into every count when a rep[t] < 1


def absbin_edges():
    """float32 [511]: the lower edges of bins 1..511 (= the upper edges of bins 0..510), the floats with bits (K0 + b) << SHIFT"""
    return ((np.arange(1, ABSBIN_BINS, dtype=np.int64) + ABSBIN_K0) << ABSBIN_SHIFT).astype(np.uint32).view(np.float32)


def absbin_log10_limits():
    """float64 [512]: log10 of the bins' upper edges, formed in double — the bucket limits of the histogram; the last bin takes everything up to
    infinity and NaN and is closed at the largest float32.  The lower side of bin 0 is -15, the reference's clamp."""
    return np.log10(np.append(absbin_edges().astype(np.float64), float(np.finfo(np.float32).max)))


def absbin_hist(src, items, hist):
    """replaces the per-tensor .abs().sort() of sota_imagenet/callbacks.py:47 and :56: ADDS into hist[t] (CUDA int32 [n_tensors, 512], read as
    unsigned; zeroed by the caller) the bin counts of |src| over the work items { first element, length <= lw_item_elems(), t } of `items`; src:
    the flat fp32 array the item offsets count from.  Elements outside the items are not counted, an item outside src is skipped."""
    _arg("absbin_hist", "src", _F32, None, src)
    _arg("absbin_hist", "items", _I64, _REC16, items)
    _arg("absbin_hist", "hist", _I32, (None, ABSBIN_BINS), hist)
    _on_device("absbin_hist", "src items hist", src, items, hist)
    check(_L().mi355_absbin_hist(ptr(src), src.numel(), ptr(items), items.shape[0], hist.shape[0], ptr(hist), cur_stream()))


def subsample_counts(hist, rep, subsample, counts, rep_host=None):
    """replaces the [::subsample], torch.cat, second sort and second [::subsample] of callbacks.py:47-50 and :56-59: counts[k] (CUDA int64 [512]) =
    the number of values of the twice-subsampled set in bin k, from the per-tensor histograms hist [n, 512] and rep (CUDA int32 [n]: shown elements
    per counted element, >= 1).  rep lives on the device: a rep < 1 makes the kernel write -1 (ABSBIN_BAD_REP unsigned) into every count; rep_host,
    the same numbers on the host where the caller has them, is tested here and raises ValueError."""
    _arg("subsample_counts", "hist", _I32, (None, ABSBIN_BINS), hist)
    _arg("subsample_counts", "rep", _I32, (hist.shape[0],), rep)
    _arg("subsample_counts", "counts", _I64, (ABSBIN_BINS,), counts)
    _on_device("subsample_counts", "hist rep counts", hist, rep, counts)
    if rep_host is not None and (len(rep_host) != hist.shape[0] or any(int(r) < 1 for r in rep_host)):
        raise ValueError(f"subsample_counts: rep must hold one number >= 1 per tensor, got {list(rep_host)[:8]}...")
    check(_L().mi355_subsample_counts(ptr(hist), ptr(rep), hist.shape[0], int(subsample), ptr(counts), cur_stream()))


# ---- the histogram over TensorBoard's default bins (include/mi355rn.h, csrc/optim_wdist.hip): the WeightDistributionTB callback ---------------------
TBBIN_POS = 774                 # positive edges
TBBIN_BINS = 2 * TBBIN_POS      # 1548 bins between 1549 edges
TBBIN_NOBIN = TBBIN_BINS        # the row's entry that counts what lies in no bin: NaN, infinities, values outside the table
TBBIN_ROW = 1552                # entries per row of hist[]: a whole number of 16-byte vectors
TBBIN_STATS = 5                 # doubles per work item in partial[]: min, max, sum, sum of squares, NaN seen
_tbbin_dev = {}                 # device -> the positive edges there


def tbbin_edges():
    """float64 [1549]: the default bins of SummaryWriter.add_histogram (bins="tensorflow") — v = 1e-12, v *= 1.1 in double while v < 1e20 gives the
    774 positive edges; the table is their negatives reversed, 0, and they.  Formed by the recurrence, not by a power: the rounding of every
    product is part of the rule."""
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    assert len(pos) == TBBIN_POS
    return np.array([-e for e in reversed(pos)] + [0.0] + pos, dtype=np.float64)


def tbbin_hist(src, items, hist, partial):
    """replaces the per-tensor p.flatten() -> host -> np.histogram / min / max / sum / dot of add_histogram (sota_imagenet/callbacks.py:16): ADDS into
    hist[t] (CUDA int32 [n_tensors, 1552], read as unsigned; zeroed by the caller) the counts of src over the 1548 default bins, entry TBBIN_NOBIN
    counting what lies in no bin, for the work items { first element, length <= lw_item_elems(), t } of `items`, and writes partial[i] (CUDA float64
    [n_items, 5]) = min, max, sum, sum of squares, NaN seen of item i.  src: the flat fp32 array the item offsets count from.  Elements outside the
    items are not read, an item outside src is skipped."""
    _arg("tbbin_hist", "src", _F32, None, src)
    _arg("tbbin_hist", "items", _I64, _REC16, items)
    _arg("tbbin_hist", "hist", _I32, (None, TBBIN_ROW), hist)
    _arg("tbbin_hist", "partial", _F64, (items.shape[0], TBBIN_STATS), partial)
    dev = _on_device("tbbin_hist", "src items hist partial", src, items, hist, partial)
    edges = _tbbin_dev.get(dev)
    if edges is None:
        edges = _tbbin_dev[dev] = torch.from_numpy(tbbin_edges()[TBBIN_POS + 1:].copy()).to(dev)
    check(_L().mi355_tbbin_hist(ptr(src), src.numel(), ptr(items), items.shape[0], hist.shape[0], ptr(edges), edges.numel(), ptr(hist), ptr(partial),
                                cur_stream()))


# ---- BResNet-50 variant blocks (include/mi355rn.h, csrc/variant.hip) ---------------------------------------------------
def _pool2_fwd(stem, x):
    """the 2x2 / stride-2 down-sampling ops without a second output: y [N,H/2,W/2,C] from x [N,H,W,C]"""
    _arg(stem, "x", _ACT, _NHWC, x)
    dev = _on_device(stem, "x", x)
    N, H, W, C = x.shape
    y = torch.empty(_half(N, H, W, C), dtype=x.dtype, device=dev)
    check(getattr(_L(), "mi355_" + stem)(dtype_code(x.dtype), ptr(x), ptr(y), N, H, W, C, cur_stream()))
    return y


def _pool2_bwd(stem, dy, x_shape):
    """their backward: dx [N,H,W,C] from dy [N,H/2,W/2,C]"""
    N, H, W, C = x_shape
    _arg(stem, "dy", _ACT, _half(N, H, W, C), dy)
    dev = _on_device(stem, "dy", dy)
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dev)
    check(getattr(_L(), "mi355_" + stem)(dtype_code(dy.dtype), ptr(dy), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def blurpool_fwd(x):
    return _pool2_fwd("blurpool_fwd", x)


def blurpool_bwd(dy, x_shape):
    return _pool2_bwd("blurpool_bwd", dy, x_shape)


def avgpool2_fwd(x):
    return _pool2_fwd("avgpool2_fwd", x)


def avgpool2_bwd(dy, x_shape):
    return _pool2_bwd("avgpool2_bwd", dy, x_shape)


def maxpool3s1_fwd(x):
    """3x3 / stride 1 / pad 1 on x [N,H,W,C]: returns (y, idx) like x, idx u8 = the window position of the first maximum"""
    _arg("maxpool3s1_fwd", "x", _ACT, _NHWC, x)
    dev = _on_device("maxpool3s1_fwd", "x", x)
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    idx = torch.empty((N, H, W, C), dtype=_U8, device=dev)
    check(_L().mi355_maxpool3s1_fwd(dtype_code(x.dtype), ptr(x), ptr(y), ptr(idx), N, H, W, C, cur_stream()))
    return y, idx


def maxpool3s1_bwd(dy, idx):
    """dx like dy [N,H,W,C] from the u8 codes idx maxpool3s1_fwd returned, of dy's shape"""
    _arg("maxpool3s1_bwd", "dy", _ACT, _NHWC, dy)
    _arg("maxpool3s1_bwd", "idx", _U8, dy.shape, idx)
    _on_device("maxpool3s1_bwd", "dy idx", dy, idx)
    N, H, W, C = dy.shape
    dx = torch.empty_like(dy)
    check(_L().mi355_maxpool3s1_bwd(dtype_code(dy.dtype), ptr(dy), ptr(idx), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def eca_fwd(x, w):
    """x [N,H,W,C], w: the k fp32 taps (k odd <= 9 is the library's to refuse).  returns (y, pooled [N,C] fp32, gate [N,C] fp32)"""
    _arg("eca_fwd", "x", _ACT, _NHWC, x)
    _arg("eca_fwd", "w", _F32, None, w)
    dev = _on_device("eca_fwd", "x w", x, w)
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    pooled = torch.empty((N, C), dtype=_F32, device=dev)
    gate = torch.empty((N, C), dtype=_F32, device=dev)
    check(_L().mi355_eca_fwd(dtype_code(x.dtype), ptr(x), ptr(w), w.numel(), ptr(y), ptr(pooled), ptr(gate), N, H * W, C, cur_stream()))
    return y, pooled, gate


def eca_bwd(dy, x, w, pooled, gate, dw=None, beta=0.0):
    """dy like x; pooled, gate: what eca_fwd returned.  returns (dx, dw [k] fp32); with dw given: dw = beta * dw + the gradient (beta 0: dw is
    only written)"""
    _arg("eca_bwd", "x", _ACT, _NHWC, x)
    N, H, W, C = x.shape
    _arg("eca_bwd", "dy", x.dtype, x.shape, dy)
    _arg("eca_bwd", "w", _F32, None, w)
    _arg("eca_bwd", "pooled gate", _F32, (N, C), pooled, gate)
    _arg("eca_bwd", "dw", _F32, w.numel(), dw, optional=True)
    dev = _on_device("eca_bwd", "dy x w pooled gate dw", dy, x, w, pooled, gate, dw)
    dx = torch.empty_like(x)
    if dw is None:
        dw = torch.empty_like(w)
    ws, _ = _scratch(4 * (2 * N * C + 128 * 9), dev)  # mi355_eca_bwd: sprod, dpool, dw partials (floats)
    check(_L().mi355_eca_bwd(dtype_code(x.dtype), ptr(dy), ptr(x), ptr(w), w.numel(), ptr(pooled), ptr(gate), ptr(dx), ptr(dw), beta, ptr(ws),
                             N, H * W, C, cur_stream()))
    return dx, dw


def weight_std_fwd(w, eps=1e-5):
    """w: [Cout, ...] fp32 contiguous.  returns (w_hat, invstd [Cout])"""
    _arg("weight_std_fwd", "w", _F32, None, w)
    dev = _on_device("weight_std_fwd", "w", w)
    Cout = w.shape[0]
    K = w.numel() // Cout
    w_hat = torch.empty_like(w)
    mean = torch.empty(Cout, dtype=_F32, device=dev)
    invstd = torch.empty(Cout, dtype=_F32, device=dev)
    check(_L().mi355_weight_std_fwd(ptr(w), ptr(w_hat), ptr(mean), ptr(invstd), Cout, K, eps, cur_stream()))
    return w_hat, invstd


def weight_std_bwd(dw_hat, w_hat, invstd, dw=None, beta=0.0):
    """w_hat [Cout, ...] and invstd [Cout] as weight_std_fwd returned them, dw_hat (and dw) fp32 of w_hat's size.  with dw given:
    dw = beta * dw + the gradient (beta 0: dw is only written)"""
    _arg("weight_std_bwd", "w_hat", _F32, None, w_hat)
    Cout = w_hat.shape[0]
    _arg("weight_std_bwd", "dw_hat", _F32, w_hat.numel(), dw_hat)
    _arg("weight_std_bwd", "invstd", _F32, Cout, invstd)
    _arg("weight_std_bwd", "dw", _F32, w_hat.numel(), dw, optional=True)
    _on_device("weight_std_bwd", "dw_hat w_hat invstd dw", dw_hat, w_hat, invstd, dw)
    if dw is None:
        dw = torch.empty_like(w_hat)
    check(_L().mi355_weight_std_bwd(ptr(dw_hat), ptr(w_hat), ptr(invstd), ptr(dw), beta, Cout, w_hat.numel() // Cout, cur_stream()))
    return dw


def residual_act_fwd(branch, shortcut=None, scale_n=None, act=1):
    """out = act(branch * scale_n[n] + shortcut): branch [N, ...], shortcut like it, scale_n fp32 [N] (both optional)"""
    _arg("residual_act_fwd", "branch", _ACT, None, branch)
    N = branch.shape[0]
    _arg("residual_act_fwd", "shortcut", branch.dtype, branch.shape, shortcut, optional=True)
    _arg("residual_act_fwd", "scale_n", _F32, N, scale_n, optional=True)
    _on_device("residual_act_fwd", "branch shortcut scale_n", branch, shortcut, scale_n)
    out = torch.empty_like(branch)
    check(_L().mi355_residual_act_fwd(dtype_code(branch.dtype), ptr(branch), ptr(scale_n), ptr(shortcut), ptr(out), N, branch.numel() // N, act, cur_stream()))
    return out


def residual_act_bwd(dout, out, scale_n=None, act=1, want_shortcut=True):
    """(dbranch, dshortcut or None) from `out` [N, ...] as residual_act_fwd returned it, dout like it, scale_n fp32 [N] (optional)"""
    _arg("residual_act_bwd", "out", _ACT, None, out)
    N = out.shape[0]
    _arg("residual_act_bwd", "dout", out.dtype, out.shape, dout)
    _arg("residual_act_bwd", "scale_n", _F32, N, scale_n, optional=True)
    _on_device("residual_act_bwd", "dout out scale_n", dout, out, scale_n)
    db = torch.empty_like(out)
    ds = torch.empty_like(out) if want_shortcut else None
    check(_L().mi355_residual_act_bwd(dtype_code(out.dtype), ptr(dout), ptr(out), ptr(scale_n), ptr(db), ptr(ds), N, out.numel() // N, act, cur_stream()))
    return db, ds


def keep_scale(n, p, seed, counter, device):
    keep = torch.empty(n, dtype=_F32, device=device)
    check(_L().mi355_keep_scale(ptr(keep), n, float(p), int(seed), int(counter), cur_stream()))
    return keep
