"""Per-op Python entry points over the C-ABI (include/mi355rn.h) on PyTorch-ROCm tensors.

These are the unit-level handles the parity tests use; the training path goes through the whole-network
executor (sota_imagenet_amd/models.py).  Tensors are NHWC (`[N,H,W,C]`), conv weights KRSC (`[Cout,KH,KW,Cin]`).
Every function enqueues on torch's current stream and raises RuntimeError on any native failure.
"""
import ctypes

import numpy as np
import torch

from . import native
from .native import check, cur_stream, dtype_code, ptr


def _L():
    return native.lib()


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise ValueError("tensors must be contiguous CUDA (ROCm) tensors")


def _out_dim(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def conv2d_fwd(x, w, stride=1, pad=0, stats=False):
    """stats=True: returns (y, partial) — `partial` = the BN batch-statistics rows the conv epilogue summed over y, an fp32
    tensor [nblk, 2, Cout] (or None where the launch could not carry them) to hand to bn_fwd_train(y, ..., stats=partial):
    an explicit value owned by the caller, valid for exactly this y as long as y is not modified."""
    _need_cuda(x, w)
    N, H, W, Cin = x.shape
    Cout, KH, KW, _ = w.shape
    y = torch.empty((N, _out_dim(H, KH, stride, pad), _out_dim(W, KW, stride, pad), Cout), dtype=x.dtype, device=x.device)
    if not stats:
        check(_L().mi355_conv2d_fwd(dtype_code(x.dtype), ptr(x), ptr(w), ptr(y), N, H, W, Cin, Cout, KH, KW, stride, pad, cur_stream()))
        return y
    # rows of the statistics scratch: the implicit-GEMM kernels write <= 768, the generated kernels one per pixel tile (3584 for a
    # 56 x 56 x 64 conv at batch 256, 14336 for a 112 x 112 x 64 one: two-row tiles); the library takes the kernel the buffer allows (the static
    # executors give it their widest layer's)
    rows = 16384 if Cout <= 128 else (8192 if Cout <= 256 else 768)
    partial = torch.empty(rows * 2 * Cout, dtype=torch.float32, device=x.device)
    nblk = ctypes.c_int(0)
    check(_L().mi355_conv2d_fwd_stats(dtype_code(x.dtype), ptr(x), ptr(w), ptr(y), ptr(partial), partial.numel() * 4, ctypes.byref(nblk), N, H, W, Cin,
                                      Cout, KH, KW, stride, pad, cur_stream()))
    return y, (partial[: nblk.value * 2 * Cout].view(nblk.value, 2, Cout) if nblk.value > 0 else None)


def conv2d_fwd_bn_in(y_in, scale, shift, w, pad=1):
    """the forward conv with the previous layer's BatchNorm + ReLU in its operand path (mi355_conv2d_fwd_bn_in): returns
    (y, partial, a, a_bits) — y = conv(a, w) with a = relu(y_in * scale + shift) rounded to y_in's dtype, the BN statistics rows of y, and
    the by-products a and its ReLU bits (1 byte per 8 channels) the same launch leaves for the backward pass"""
    _need_cuda(y_in, scale, shift, w)
    N, H, W, Cin = y_in.shape
    Cout, KH, KW, _ = w.shape
    y = torch.empty((N, H, W, Cout), dtype=y_in.dtype, device=y_in.device)
    a = torch.empty_like(y_in)
    bits = torch.empty((N, H, W, Cin // 8), dtype=torch.uint8, device=y_in.device)
    ss = torch.cat([scale.float().reshape(-1), shift.float().reshape(-1)]).contiguous()
    rows = 8192 if Cout <= 256 else 768
    partial = torch.empty(rows * 2 * Cout, dtype=torch.float32, device=y_in.device)
    nblk = ctypes.c_int(0)
    check(_L().mi355_conv2d_fwd_bn_in(dtype_code(y_in.dtype), ptr(y_in), ptr(ss), ptr(w), ptr(y), ptr(a), ptr(bits), ptr(partial), partial.numel() * 4,
                                      ctypes.byref(nblk), N, H, W, Cin, Cout, KH, KW, 1, pad, cur_stream()))
    return y, (partial[: nblk.value * 2 * Cout].view(nblk.value, 2, Cout) if nblk.value > 0 else None), a, bits


def quantize_fp8(x, scale=1.0):
    """q = saturate_e4m3fn(x * scale) as a torch.float8_e4m3fn tensor of x's shape (x fp32 or bf16, numel % 8 == 0)."""
    _need_cuda(x)
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(_L().mi355_quantize_fp8(dtype_code(x.dtype), ptr(x), ptr(q), float(scale), x.numel(), cur_stream()))
    return q.view(torch.float8_e4m3fn)


def conv2d_fwd_fp8(xq, wq, stride=1, pad=0, oscale=1.0):
    """bf16 y = conv(xq NHWC e4m3, wq KRSC e4m3) * oscale on the fp8 MFMA path (Cin, Cout multiples of 128)."""
    _need_cuda(xq, wq)
    N, H, W, Cin = xq.shape
    Cout, KH, KW, _ = wq.shape
    y = torch.empty((N, _out_dim(H, KH, stride, pad), _out_dim(W, KW, stride, pad), Cout), dtype=torch.bfloat16, device=xq.device)
    check(_L().mi355_conv2d_fwd_fp8(ptr(xq), ptr(wq), ptr(y), float(oscale), N, H, W, Cin, Cout, KH, KW, stride, pad, cur_stream()))
    return y


def conv2d_dgrad_fp8(dyq, wq, x_shape, stride=1, pad=0, oscale=1.0, wt=None):
    """bf16 dx for the conv above from e4m3 dy and the KRSC e4m3 weights (transposed here to [Cin][KH][KW][Cout])."""
    _need_cuda(dyq, wq)
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = wq.shape
    if wt is None:
        wt = wq.view(torch.uint8).permute(3, 1, 2, 0).contiguous()
    dx = torch.empty((N, H, W, Cin), dtype=torch.bfloat16, device=dyq.device)
    check(_L().mi355_conv2d_dgrad_fp8(ptr(dyq), ptr(wt), ptr(dx), float(oscale), N, H, W, Cin, Cout, KH, KW, stride, pad, cur_stream()))
    return dx


_WGRAD_WS = {}


def conv2d_wgrad_fp8(dyq, xq, KH, KW, stride=1, pad=0, oscale=1.0):
    """fp32 dw [Cout,KH,KW,Cin] = oscale * sum_pixels dyq (x) xq from e4m3 dy (NHWC) and x (NHWC) on the fp8 MFMA path."""
    _need_cuda(dyq, xq)
    N, H, W, Cin = xq.shape
    Cout = dyq.shape[-1]
    n = _L().mi355_conv2d_workspace_bytes(native.BF16, N, H, W, Cin, Cout, KH, KW, stride, pad)
    # split-K slabs + the two scale words: one workspace per (device, stream, size) — calls on different streams must not share slabs —
    # and at most 8 of them (the oldest goes first)
    key = (dyq.device, torch.cuda.current_stream(dyq.device).cuda_stream, n)
    ws = _WGRAD_WS.get(key)
    if ws is None:
        while len(_WGRAD_WS) >= 8:
            _WGRAD_WS.pop(next(iter(_WGRAD_WS)))
        ws = _WGRAD_WS[key] = torch.empty(n + 256, dtype=torch.uint8, device=dyq.device)
    dw = torch.empty((Cout, KH, KW, Cin), dtype=torch.float32, device=dyq.device)
    check(_L().mi355_conv2d_wgrad_fp8(ptr(dyq), ptr(xq), ptr(dw), 0.0, float(oscale), N, H, W, Cin, Cout, KH, KW, stride, pad, ptr(ws), n + 256, cur_stream()))
    return dw


def ingest_u8(packed, table_host, table_dev, S, mean=127.5, std=51.0, aug_host=None, aug_dev=None):
    """decoded u8 RGB crops (packed device bytes + mi355_crop table as a numpy structured array and its device copy) ->
    fp32 NCHW [N,3,S,S]: resize, window, [augment table: blur / colour / grey / erase], mirror, normalise (csrc/ingest.hip)."""
    _need_cuda(packed, table_dev, aug_dev)
    N = int(table_host.shape[0])
    if table_host.dtype.itemsize != 40 or table_dev.numel() * table_dev.element_size() != 40 * N or not table_host.flags["C_CONTIGUOUS"]:
        raise ValueError("ingest_u8: the descriptor table must be N contiguous 40-byte mi355_crop records on both sides")
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device=packed.device)
    if aug_host is None:
        check(_L().mi355_ingest_u8(ptr(packed), packed.numel(), table_host.ctypes.data, ptr(table_dev), N, int(S), float(mean), float(std), ptr(out), cur_stream()))
        return out
    if aug_host.dtype.itemsize != 128 or aug_host.shape[0] != N or aug_dev is None or aug_dev.numel() * aug_dev.element_size() != 128 * N or not aug_host.flags["C_CONTIGUOUS"]:
        raise ValueError("ingest_u8: the augment table must be N contiguous 128-byte mi355_augment records on both sides")
    scratch = torch.empty((N, 3, S, S), dtype=torch.float32, device=packed.device) if bool((aug_host["blur_sigma"] > 0).any()) else None
    check(_L().mi355_ingest_u8_aug(ptr(packed), packed.numel(), table_host.ctypes.data, ptr(table_dev), aug_host.ctypes.data, ptr(aug_dev), N, int(S),
                                   float(mean), float(std), ptr(scratch), ptr(out), cur_stream()))
    return out


def _conv_ws(dt, N, H, W, Cin, Cout, KH, KW, stride, pad, device):
    n = _L().mi355_conv2d_workspace_bytes(dt, N, H, W, Cin, Cout, KH, KW, stride, pad)
    return torch.empty(n, dtype=torch.uint8, device=device), n


def conv2d_dgrad(dy, w, x_shape, stride=1, pad=0, addend=None):
    _need_cuda(dy, w, addend)
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = w.shape
    dt = dtype_code(dy.dtype)
    ws, n = _conv_ws(dt, N, H, W, Cin, Cout, KH, KW, stride, pad, dy.device)
    dx = torch.empty((N, H, W, Cin), dtype=dy.dtype, device=dy.device)
    check(_L().mi355_conv2d_dgrad(dt, ptr(dy), ptr(w), ptr(dx), ptr(addend), N, H, W, Cin, Cout, KH, KW, stride, pad, ptr(ws), n, cur_stream()))
    return dx


def conv2d_dgrad_bn(dy, w, x_shape, stride=1, pad=0, addend=None, addend_bits=None, bn_y=None, bn_bits=None, bn_mean=None, bn_invstd=None, addend_sub2=False, slope=0.0):
    """the data gradient as the executor's backward launches it: dx = dgrad(dy) + addend (under the ReLU bits addend_bits), and — with
    bn_y / bn_bits / bn_mean / bn_invstd — the BN-backward partial rows [nblk][2][Cin] (sum dz, sum dz * xhat) of the layer dx is the
    activation gradient of.  addend_sub2: the addend is [N, H/2, W/2, Cin], standing for a full-resolution tensor that is zero at odd rows /
    columns.  slope: the sums under a leaky-ReLU mask (dz = dx * slope where the bit is clear; 0.01 at BResNet-50's shapes, mi355_conv2d_dgrad_bn_leaky).
    Returns (dx, partial or None)."""
    _need_cuda(dy, w, addend, addend_bits, bn_y, bn_bits, bn_mean, bn_invstd)
    N, H, W, Cin = x_shape
    Cout, KH, KW, _ = w.shape
    dt = dtype_code(dy.dtype)
    ws, n = _conv_ws(dt, N, H, W, Cin, Cout, KH, KW, stride, pad, dy.device)
    dx = torch.empty((N, H, W, Cin), dtype=dy.dtype, device=dy.device)
    part = None
    nblk = ctypes.c_int(0)
    if bn_y is not None:
        part = torch.empty((4096, 2, Cin), dtype=torch.float32, device=dy.device)
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
    _need_cuda(dy, x, dw)
    N, H, W, Cin = x.shape
    Cout = dy.shape[-1]
    dt = dtype_code(dy.dtype)
    ws, n = _conv_ws(dt, N, H, W, Cin, Cout, KH, KW, stride, pad, dy.device)
    if dw is None:
        dw = torch.empty((Cout, KH, KW, Cin), dtype=torch.float32, device=dy.device)
    check(_L().mi355_conv2d_wgrad(dt, ptr(dy), ptr(x), ptr(dw), beta, N, H, W, Cin, Cout, KH, KW, stride, pad, ptr(ws), n, cur_stream()))
    return dw


def stem_ingest(x_nchw, dtype):
    _need_cuda(x_nchw)
    N, _, H, W = x_nchw.shape
    dt = dtype_code(dtype)
    nbytes = _L().mi355_stem_xpad_bytes(dt, N, H, W)
    xpad = torch.zeros(nbytes, dtype=torch.uint8, device=x_nchw.device)
    check(_L().mi355_stem_ingest(dt, ptr(x_nchw), ptr(xpad), N, H, W, cur_stream()))
    return xpad


def stem_fwd(xpad, w, N, H, W, dtype):
    """w: [64,7,7,3] fp32 (KRSC)."""
    _need_cuda(xpad, w)
    dt = dtype_code(dtype)
    n = _L().mi355_stem_workspace_bytes(dt, N, H, W)
    ws = torch.empty(n, dtype=torch.uint8, device=w.device)
    y = torch.empty((N, H // 2, W // 2, 64), dtype=dtype, device=w.device)
    check(_L().mi355_stem_fwd(dt, ptr(xpad), ptr(w), ptr(y), N, H, W, ptr(ws), n, cur_stream()))
    return y


def stem_wgrad(dy, xpad, N, H, W):
    _need_cuda(dy, xpad)
    dt = dtype_code(dy.dtype)
    n = _L().mi355_stem_workspace_bytes(dt, N, H, W)
    ws = torch.empty(n, dtype=torch.uint8, device=dy.device)
    dw = torch.empty((64, 7, 7, 3), dtype=torch.float32, device=dy.device)
    check(_L().mi355_stem_wgrad(dt, ptr(dy), ptr(xpad), ptr(dw), 0.0, N, H, W, ptr(ws), n, cur_stream()))
    return dw


def _bn_ws(C, device):
    n = _L().mi355_bn_workspace_bytes(C)
    return torch.empty(n, dtype=torch.uint8, device=device), n


def bn_fwd_train(x, gamma, beta, running_mean, running_var, residual=None, relu=True, eps=1e-5, momentum=0.1, stats=None):
    """x: [..., C] NHWC.  Updates running stats in place.  Returns (out, save_mean, save_invstd).
    stats: the partial rows conv2d_fwd(stats=True) returned for THIS x (no reduction pass over x then)."""
    _need_cuda(x, gamma, beta, running_mean, running_var, residual)
    C = x.shape[-1]
    M = x.numel() // C
    out = torch.empty_like(x)
    sm = torch.empty(C, dtype=torch.float32, device=x.device)
    si = torch.empty(C, dtype=torch.float32, device=x.device)
    if stats is not None:  # the conv that produced x already summed it
        _need_cuda(stats)
        if stats.dim() != 3 or stats.shape[1:] != (2, C) or stats.dtype != torch.float32:
            raise ValueError(f"bn_fwd_train: stats must be the fp32 [nblk, 2, {C}] rows conv2d_fwd(stats=True) returned for this tensor")
        ws = torch.empty(2 * C, dtype=torch.float32, device=x.device)
        check(_L().mi355_bn_fwd_train_partial(dtype_code(x.dtype), ptr(x), ptr(residual), ptr(out), ptr(gamma), ptr(beta), ptr(running_mean),
                                              ptr(running_var), ptr(sm), ptr(si), M, C, eps, momentum, int(relu), ptr(stats), stats.shape[0], ptr(ws),
                                              ws.numel() * 4, cur_stream()))
        return out, sm, si
    ws, n = _bn_ws(C, x.device)
    check(_L().mi355_bn_fwd_train(dtype_code(x.dtype), ptr(x), ptr(residual), ptr(out), ptr(gamma), ptr(beta), ptr(running_mean),
                                  ptr(running_var), ptr(sm), ptr(si), M, C, eps, momentum, int(relu), ptr(ws), n, cur_stream()))
    return out, sm, si


def bn_fwd_eval(x, gamma, beta, running_mean, running_var, residual=None, relu=True, eps=1e-5):
    _need_cuda(x, gamma, beta, running_mean, running_var, residual)
    C = x.shape[-1]
    M = x.numel() // C
    out = torch.empty_like(x)
    ws, n = _bn_ws(C, x.device)
    check(_L().mi355_bn_fwd_eval(dtype_code(x.dtype), ptr(x), ptr(residual), ptr(out), ptr(gamma), ptr(beta), ptr(running_mean),
                                 ptr(running_var), M, C, eps, int(relu), ptr(ws), n, cur_stream()))
    return out


def _bn_c_vectors(who, C, **named):
    for name, t in named.items():
        if t is not None and (t.dtype != torch.float32 or t.numel() != C or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be {C} contiguous fp32 values")


def _bn_like(who, x, **named):
    for name, t in named.items():
        if t is not None and (t.shape != x.shape or t.dtype != x.dtype or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous {tuple(x.shape)} {x.dtype} tensor like x")


def bn_bwd(dout, out, x, gamma, save_mean, save_invstd, relu=True, want_dz=False, dgamma=None, dbeta=None, beta_acc=0.0):
    """Returns (dx, dgamma, dbeta, dz or None).  dgamma / dbeta given: written in place (beta_acc = 1 accumulates onto them)."""
    _need_cuda(dout, out, x, gamma, save_mean, save_invstd, dgamma, dbeta)
    C = x.shape[-1]
    M = x.numel() // C
    _bn_c_vectors("bn_bwd", C, dgamma=dgamma, dbeta=dbeta)
    dx = torch.empty_like(x)
    dz = torch.empty_like(x) if want_dz else None
    dg = dgamma if dgamma is not None else torch.zeros(C, dtype=torch.float32, device=x.device)
    db = dbeta if dbeta is not None else torch.zeros(C, dtype=torch.float32, device=x.device)
    ws, n = _bn_ws(C, x.device)
    check(_L().mi355_bn_bwd(dtype_code(x.dtype), ptr(dout), ptr(out), ptr(x), ptr(gamma), ptr(save_mean), ptr(save_invstd), ptr(dx),
                            ptr(dz), ptr(dg), ptr(db), float(beta_acc), M, C, int(relu), ptr(ws), n, cur_stream()))
    return dx, dg, db, dz


def bn_apply(x, scale, shift, residual=None, x2=None, scale2=None, shift2=None, relu=1, want_bits=False):
    """The executors' BatchNorm apply pass on given fp32 coefficients (mi355_bn_apply): act(x * scale + shift (+ residual | + x2 * scale2 + shift2)).
    relu: 0 / 1 / 2 (leaky, slope 0.01).  Returns (out, bits): bits [..., C/V] u8 (V = 16 bytes of elements, bit e of byte v = the sum of channel
    v * V + e was > 0) with want_bits, else None.  Combinations the kernels do not have raise (native.check)."""
    _need_cuda(x, scale, shift, residual, x2, scale2, shift2)
    C = x.shape[-1]
    M = x.numel() // C
    V = 16 // x.element_size()
    if not x.is_contiguous():
        raise ValueError("bn_apply: x must be contiguous")
    _bn_c_vectors("bn_apply", C, scale=scale, shift=shift, scale2=scale2, shift2=shift2)
    _bn_like("bn_apply", x, residual=residual, x2=x2)
    out = torch.empty_like(x)
    bits = torch.empty(tuple(x.shape[:-1]) + (C // V,), dtype=torch.uint8, device=x.device) if want_bits else None
    check(_L().mi355_bn_apply(dtype_code(x.dtype), ptr(x), ptr(scale), ptr(shift), ptr(residual), ptr(x2), ptr(scale2), ptr(shift2), ptr(out),
                              ptr(bits), M, C, int(relu), cur_stream()))
    return out, bits


def bn_bwd_bits(g, bits, x, gamma, mean, invstd, relu=1, dx=None, dz_out=None, dgamma=None, dbeta=None, beta_acc=0.0, partial=None):
    """The executors' BatchNorm backward from the ReLU bit mask (mi355_bn_bwd_bits): returns (dx, dgamma, dbeta).  relu 0: bits None.  dx / dz_out
    given: written in place, either may be g itself.  dgamma / dbeta given: written in place (beta_acc = 1 accumulates).  partial: fp32
    [nblk, 2, C] rows of (sum dz, sum dz * x_hat) from a fused data-gradient epilogue, in place of the reduce pass (ignored, as in the executor, when
    dz_out asks for the masked gradient)."""
    _need_cuda(g, bits, x, gamma, mean, invstd, dx, dz_out, dgamma, dbeta, partial)
    C = x.shape[-1]
    M = x.numel() // C
    V = 16 // x.element_size()
    if not x.is_contiguous():
        raise ValueError("bn_bwd_bits: x must be contiguous")
    _bn_like("bn_bwd_bits", x, g=g, dx=dx, dz_out=dz_out)
    _bn_c_vectors("bn_bwd_bits", C, gamma=gamma, mean=mean, invstd=invstd, dgamma=dgamma, dbeta=dbeta)
    if bits is not None and (bits.dtype != torch.uint8 or bits.numel() != M * C // V or not bits.is_contiguous()):
        raise ValueError(f"bn_bwd_bits: bits must be {M * C // V} contiguous u8 values (one per 16-byte vector)")
    nblk = 0
    if partial is not None:
        if partial.dim() != 3 or partial.shape[1:] != (2, C) or partial.dtype != torch.float32 or not partial.is_contiguous():
            raise ValueError(f"bn_bwd_bits: partial must be contiguous fp32 [nblk, 2, {C}] rows")
        nblk = partial.shape[0]
    dx = dx if dx is not None else torch.empty_like(x)
    dg = dgamma if dgamma is not None else torch.zeros(C, dtype=torch.float32, device=x.device)
    db = dbeta if dbeta is not None else torch.zeros(C, dtype=torch.float32, device=x.device)
    ws, n = _bn_ws(C, x.device)
    check(_L().mi355_bn_bwd_bits(dtype_code(x.dtype), ptr(g), ptr(bits), ptr(x), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx), ptr(dz_out), ptr(dg),
                                 ptr(db), float(beta_acc), M, C, int(relu), ptr(partial), nblk, ptr(ws), n, cur_stream()))
    return dx, dg, db


def maxpool_fwd(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    idx = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
    check(_L().mi355_maxpool_fwd(dtype_code(x.dtype), ptr(x), ptr(y), ptr(idx), N, H, W, C, cur_stream()))
    return y, idx


def maxpool_bwd(dy, idx, x_shape):
    _need_cuda(dy, idx)
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    check(_L().mi355_maxpool_bwd(dtype_code(dy.dtype), ptr(dy), ptr(idx), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def bn_relu_maxpool(y, scale, shift, form=0):
    """The stem's fused tail on the raw conv output y [N,H,W,C]: (p, idx, bits) = pooled relu(y * scale + shift), argmax codes, ReLU bits
    [N,H,W,C/V] (V = 16 bytes of elements).  form: 0 the executor's rule, 1 / 2 / 3 one of the three kernels forced (mi355rn.h)."""
    _need_cuda(y, scale, shift)
    N, H, W, C = y.shape
    V = 16 // y.element_size()
    for name, t in (("scale", scale), ("shift", shift)):
        if t.dtype != torch.float32 or t.numel() != C:
            raise ValueError(f"bn_relu_maxpool: {name} must be {C} fp32 values")
    p = torch.empty((N, H // 2, W // 2, C), dtype=y.dtype, device=y.device)
    idx = torch.empty((N, H // 2, W // 2, C), dtype=torch.uint8, device=y.device)
    bits = torch.empty((N, H, W, C // V), dtype=torch.uint8, device=y.device)
    check(_L().mi355_bn_relu_maxpool(dtype_code(y.dtype), ptr(y), ptr(scale), ptr(shift), ptr(p), ptr(idx), ptr(bits), N, H, W, C, int(form),
                                     cur_stream()))
    return p, idx, bits


def stem_bwd(dp, idx, bits, y, gamma, mean, invstd, dgamma=None, dbeta=None, beta_acc=0.0):
    """The executor's stem backward from the pooled gradient dp [N,H/2,W/2,64]: returns (dx wrt y, dgamma, dbeta).  dgamma / dbeta given:
    written in place (beta_acc = 1 accumulates onto them)."""
    _need_cuda(dp, idx, bits, y, gamma, mean, invstd, dgamma, dbeta)
    N, H, W, C = y.shape
    V = 16 // y.element_size()
    if (tuple(dp.shape) != (N, H // 2, W // 2, C) or dp.dtype != y.dtype or tuple(idx.shape) != tuple(dp.shape) or idx.dtype != torch.uint8
            or tuple(bits.shape) != (N, H, W, C // V) or bits.dtype != torch.uint8):
        raise ValueError(f"stem_bwd: dp / idx [N,H/2,W/2,C] and bits [N,H,W,C/{V}] u8 do not match y {tuple(y.shape)} {y.dtype}")
    for name, t in (("gamma", gamma), ("mean", mean), ("invstd", invstd), ("dgamma", dgamma), ("dbeta", dbeta)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != C):
            raise ValueError(f"stem_bwd: {name} must be {C} fp32 values")
    dx = torch.empty_like(y)
    dg = dgamma if dgamma is not None else torch.zeros(C, dtype=torch.float32, device=y.device)
    db = dbeta if dbeta is not None else torch.zeros(C, dtype=torch.float32, device=y.device)
    ws, n = _bn_ws(C, y.device)
    check(_L().mi355_stem_bwd(dtype_code(y.dtype), ptr(dp), ptr(idx), ptr(bits), ptr(y), ptr(gamma), ptr(mean), ptr(invstd), ptr(dx), ptr(dg),
                              ptr(db), beta_acc, N, H, W, C, ptr(ws), n, cur_stream()))
    return dx, dg, db


def gap_fwd(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    pooled = torch.empty((N, C), dtype=torch.float32, device=x.device)
    check(_L().mi355_gap_fwd(dtype_code(x.dtype), ptr(x), ptr(pooled), N, H * W, C, cur_stream()))
    return pooled


def gap_bwd(dpooled, x_shape, dtype):
    _need_cuda(dpooled)
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dtype, device=dpooled.device)
    check(_L().mi355_gap_bwd(dtype_code(dtype), ptr(dpooled), ptr(dx), N, H * W, C, cur_stream()))
    return dx


def ce_loss(logits, target, smoothing=0.0, grad_scale=1.0, need_grad=True):
    """Returns (loss scalar tensor on device, dlogits or None)."""
    _need_cuda(logits, target)
    N, C = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    row = torch.empty(N, dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if need_grad else None
    check(_L().mi355_ce_loss(ptr(logits), ptr(target), smoothing, grad_scale, ptr(loss), ptr(row), ptr(dl), N, C, cur_stream()))
    return loss, dl


def sgd_step(p, g, m, lr, momentum=0.0, weight_decay=0.0, grad_scale=1.0, ema=None, ema_decay=0.0):
    """ema (optional, same shape as p): the moving average of the updated parameters, advanced in the same kernel (mi355_sgd_step_ema)"""
    _need_cuda(p, g, m)
    if ema is None:
        check(_L().mi355_sgd_step(ptr(p), ptr(g), ptr(m), p.numel(), lr, momentum, weight_decay, grad_scale, cur_stream()))
        return
    _need_cuda(ema)
    assert ema.numel() == p.numel() and ema.dtype == torch.float32 and ema.is_contiguous()
    check(_L().mi355_sgd_step_ema(ptr(p), ptr(g), ptr(m), ptr(ema), p.numel(), lr, momentum, weight_decay, grad_scale, ema_decay, cur_stream()))


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, grad_scale=1.0, ema=None, ema_decay=0.0):
    """one Adam (decoupled=False) / AdamW (decoupled=True) step of a flat range whose parameters have all taken `step` steps before
    this one (torch's state['step'] after its increment is step + 1).  The bias corrections are computed here in double, as torch
    does; ema (optional): the moving average of the updated parameters, advanced in the same kernel (mi355_adam_step_ema)"""
    _need_cuda(p, g, m, v)
    b1, b2 = float(betas[0]), float(betas[1])
    t = float(step + 1)
    step_size = lr / (1.0 - b1 ** t)
    bc2_sqrt = (1.0 - b2 ** t) ** 0.5
    args = (p.numel(), b1, b2, eps, step_size, bc2_sqrt, lr, weight_decay, int(bool(decoupled)), grad_scale)
    if ema is None:
        check(_L().mi355_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), *args, cur_stream()))
        return
    _need_cuda(ema)
    assert ema.numel() == p.numel() and ema.dtype == torch.float32 and ema.is_contiguous()
    check(_L().mi355_adam_step_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), *args, ema_decay, cur_stream()))


def _flat_f32(n, **named):
    """every named tensor: contiguous CUDA fp32 of n elements"""
    for name, t in named.items():
        _need_cuda(t)
        if t.dtype != torch.float32 or t.numel() != n:
            raise ValueError(f"{name}: expected a float32 tensor of {n} elements, got {t.dtype} with {t.numel()}")


def madgrad_step(p, g, grad_sum_sq, s, x0, k, lr, momentum=0.9, weight_decay=0.0, eps=1e-6, grad_scale=1.0, ema=None, ema_decay=0.0):
    """one MADGRAD step (the reference's src.optimizers.MADGRAD) of a flat range; k: the optimizer's global counter before this step
    (lamb = (lr + eps) * sqrt(k + 1) is formed natively in double); ema (optional): the moving average of the updated parameters,
    advanced in the same kernel (mi355_madgrad_step_ema)"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, grad_sum_sq=grad_sum_sq, s=s, x0=x0)
    args = (n, float(lr), float(momentum), float(weight_decay), float(eps), int(k), float(grad_scale))
    if ema is None:
        check(_L().mi355_madgrad_step(ptr(p), ptr(g), ptr(grad_sum_sq), ptr(s), ptr(x0), *args, cur_stream()))
        return
    _flat_f32(n, ema=ema)
    check(_L().mi355_madgrad_step_ema(ptr(p), ptr(g), ptr(grad_sum_sq), ptr(s), ptr(x0), ptr(ema), *args, float(ema_decay), cur_stream()))


def adais_workspace_elems(n):
    """the number of float64 partial sums adais_moments writes for a range of n elements"""
    return _L().mi355_adais_workspace_bytes(int(n)) // 8


def adais_moments(g, v, step, beta2, workspace, grad_scale=1.0):
    """AdaiS stage (a): v = v*beta2 + (1 - beta2)*g*g in place and the per-workgroup sums of v / (1 - beta2^step) into `workspace`
    (float64, adais_workspace_elems(n) elements); step: the range's count after this step's increment"""
    n = v.numel()
    _flat_f32(n, g=g, v=v)
    _need_cuda(workspace)
    if workspace.dtype != torch.float64 or workspace.numel() != adais_workspace_elems(n):
        raise ValueError(f"workspace: expected {adais_workspace_elems(n)} float64 elements, got {workspace.dtype} with {workspace.numel()}")
    check(_L().mi355_adais_moments(ptr(g), ptr(v), n, float(beta2), int(step), float(grad_scale), ptr(workspace), cur_stream()))


def adais_mean(workspace, param_size, mean):
    """AdaiS stage (b): mean[0] = sum(workspace) / param_size, summed in a fixed order on the device (workspace: the float64 partial sums
    of every range, back to back; mean: a float32 CUDA tensor of one element)"""
    _need_cuda(workspace, mean)
    if workspace.dtype != torch.float64 or mean.dtype != torch.float32 or mean.numel() != 1:
        raise ValueError("adais_mean: workspace must be float64 and mean one float32 element")
    check(_L().mi355_adais_mean(ptr(workspace), workspace.numel() * 8, int(param_size), ptr(mean), cur_stream()))


def adais_step(p, g, m, v, beta1_prod, mean, step, lr, betas=(0.1, 0.99), eps=1e-3, weight_decay=0.0, grad_scale=1.0, ema=None, ema_decay=0.0):
    """AdaiS stage (c): the parameter update of a flat range from the device-resident mean of stage (b); ema (optional): the moving average
    of the updated parameters, advanced in the same kernel (mi355_adais_step_ema)"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, m=m, v=v, beta1_prod=beta1_prod)
    _flat_f32(1, mean=mean)
    args = (n, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale))
    if ema is None:
        check(_L().mi355_adais_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(beta1_prod), ptr(mean), *args, cur_stream()))
        return
    _flat_f32(n, ema=ema)
    check(_L().mi355_adais_step_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(beta1_prod), ptr(mean), ptr(ema), *args, float(ema_decay), cur_stream()))


# ---- layer-wise optimizers (include/mi355rn.h, csrc/optim_lw.hip): MyNovograd, NovogradApex, AdamLayerwise, MyAdai of the reference ------
LW_NORMGRAD, LW_NOVOGRAD, LW_ADAI = 0, 1, 2  # the element rule: AdamLayerwise / NovogradApex, MyNovograd, MyAdai
LW_MEAN, LW_STABLE_WD, LW_SOFT_WD, LW_SGD_MOM, LW_SQRT_MOM = 1, 2, 4, 8, 16


def lw_item_elems():
    """W: the most elements one work item (= one workgroup) covers"""
    return int(_L().mi355_lw_item_elems())


def _lw_table(name, t):
    _need_cuda(t)
    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != 2 or t.shape[0] < 1:
        raise ValueError(f"{name}: expected a CUDA int64 tensor [n, 2] of 16-byte records, got {t.dtype} {tuple(t.shape)}")


def lw_sumsq(src, items, partial, n_tensors, scale=1.0):
    """stage (a), replaces the per-tensor grad.pow(2).sum() / .mean() of sota_imagenet/optimizers.py:138, :270, :369, :488:
    partial[i] = sum over work item i of (src * scale)^2 in double; src: the flat fp32 array the item offsets count from"""
    _flat_f32(src.numel(), src=src)
    _lw_table("items", items)
    _need_cuda(partial)
    if partial.dtype != torch.float64 or partial.numel() != items.shape[0]:
        raise ValueError(f"partial: expected {items.shape[0]} float64 elements, got {partial.dtype} with {partial.numel()}")
    check(_L().mi355_lw_sumsq(ptr(src), src.numel(), ptr(items), items.shape[0], int(n_tensors), float(scale), ptr(partial), cur_stream()))


def lw_coef(rule, flags, partial, tensors, v, coef, sums, beta1, beta2, eps, lr, weight_decay, mean=1.0):
    """stage (b), replaces optimizers.py:140-146, :273-274, :370-371, :489-501 for the tensors of one param group: sums[t] = the tensor's
    partials in a fixed order, v (float32 per tensor, updated in place; LW_ADAI: float64, read only) and coef[t] = (den, beta1, gw, wdf)"""
    _lw_table("tensors", tensors)
    nt = tensors.shape[0]
    _need_cuda(partial, v, coef, sums)
    if partial.dtype != torch.float64 or sums.dtype != torch.float64 or sums.numel() != nt:
        raise ValueError("lw_coef: partial and sums must be float64, sums one element per tensor")
    if v.dtype != (torch.float64 if rule == LW_ADAI else torch.float32) or v.numel() != nt:
        raise ValueError(f"lw_coef: v must hold one {'float64' if rule == LW_ADAI else 'float32'} per tensor")
    if coef.dtype != torch.float32 or coef.numel() != 4 * nt:
        raise ValueError("lw_coef: coef must hold four float32 per tensor")
    check(_L().mi355_lw_coef(int(rule), int(flags), ptr(partial), partial.numel(), ptr(tensors), nt, ptr(v), ptr(coef), ptr(sums), float(beta1),
                             float(beta2), float(eps), float(lr), float(weight_decay), float(mean), cur_stream()))


def lw_update(rule, p, g, m, items, coef, lr, wd_eps=None, grad_scale=1.0, ema=None, ema_decay=0.0):
    """stage (c), replaces optimizers.py:144-159, :277-288, :374-391, :504-517 for the work items of one param group; p, g, m (and ema): the
    flat fp32 arrays the item offsets count from; coef: the whole [n_tensors, 4] table of stage (b)"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, m=m)
    _lw_table("items", items)
    _need_cuda(coef)
    if coef.dtype != torch.float32 or coef.numel() % 4:
        raise ValueError("lw_update: coef must hold four float32 per tensor")
    args = (n, ptr(items), items.shape[0], ptr(coef), coef.numel() // 4, float(lr), int(wd_eps is not None), float(wd_eps or 0.0), float(grad_scale))
    if ema is None:
        check(_L().mi355_lw_update(int(rule), ptr(p), ptr(g), ptr(m), *args, cur_stream()))
        return
    _flat_f32(n, ema=ema)
    check(_L().mi355_lw_update_ema(int(rule), ptr(p), ptr(g), ptr(m), ptr(ema), *args, float(ema_decay), cur_stream()))


# ---- unitwise_norm=True of MyNovograd / NovogradApex (include/mi355rn.h, csrc/optim_lw.hip): one norm per slot ----------------------------------
def _unit_slots(name, slots):
    _need_cuda(slots)
    if slots.dtype != torch.int32 or slots.dim() != 2 or slots.shape[1] != 2 or slots.shape[0] < 1:
        raise ValueError(f"{name}: slots must be a contiguous CUDA int32 tensor [n, 2], got {slots.dtype} {tuple(slots.shape)}")


def lw_unit_sumsq(src, pieces, partial, n_slots, scale=1.0):
    """stage (a), the per-output-unit sums behind unitwise_norm of sota_imagenet/optimizers.py:22: partial[i] = sum over piece i { off, len, slot }
    of (src * scale)^2 in double, a piece cut from one unit at any element offset; one wave per piece"""
    _flat_f32(src.numel(), src=src)
    _lw_table("pieces", pieces)
    _need_cuda(partial)
    if partial.dtype != torch.float64 or partial.numel() != pieces.shape[0]:
        raise ValueError(f"partial: expected {pieces.shape[0]} float64 elements, got {partial.dtype} with {partial.numel()}")
    check(_L().mi355_lw_unit_sumsq(ptr(src), src.numel(), ptr(pieces), pieces.shape[0], int(n_slots), float(scale), ptr(partial), cur_stream()))


def lw_unit_coef(partial, slots, v, den, sums, beta2, eps):
    """stage (b), replaces optimizers.py:134-146 and :267-274 for the slots of one param group: sums[s] = the slot's entries of partial[] (the
    WHOLE array) in a fixed order; v[s] = v[s]*beta2 + (1 - beta2)*sqrt(sums[s]), float32 in place; den[s] = sqrt(v[s]) + eps.  slots: CUDA int32
    [n, 2] of (first, count); v, den, sums: the group's slices, one element per slot"""
    _unit_slots("lw_unit_coef", slots)
    ns = slots.shape[0]
    _need_cuda(partial, v, den, sums)
    if partial.dtype != torch.float64 or sums.dtype != torch.float64 or sums.numel() != ns:
        raise ValueError("lw_unit_coef: partial and sums must be float64, sums one element per slot")
    if v.dtype != torch.float32 or den.dtype != torch.float32 or v.numel() != ns or den.numel() != ns:
        raise ValueError("lw_unit_coef: v and den must hold one float32 per slot")
    check(_L().mi355_lw_unit_coef(ptr(partial), partial.numel(), ptr(slots), ns, ptr(v), ptr(den), ptr(sums), float(beta2), float(eps), cur_stream()))


def lw_unit_update(rule, p, g, m, items, tensors, den, beta1, lr, weight_decay, wd_eps=None, grad_scale=1.0, ema=None, ema_decay=0.0):
    """stage (c), replaces optimizers.py:144-159 and :277-288 for the work items of one param group; p, g, m (and ema): the flat fp32 arrays the
    item offsets count from; tensors: the records { start, unit_len, slot0 } of ALL tensors; den: the whole per-slot array of stage (b)"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, m=m)
    _lw_table("items", items)
    _lw_table("tensors", tensors)
    _need_cuda(den)
    if den.dtype != torch.float32 or den.dim() != 1 or den.numel() < 1:
        raise ValueError("lw_unit_update: den must hold one float32 per slot")
    args = (n, ptr(items), items.shape[0], ptr(tensors), tensors.shape[0], ptr(den), den.numel(), float(beta1), float(lr), float(weight_decay),
            int(wd_eps is not None), float(wd_eps or 0.0), float(grad_scale))
    if ema is None:
        check(_L().mi355_lw_unit_update(int(rule), ptr(p), ptr(g), ptr(m), *args, cur_stream()))
        return
    _flat_f32(n, ema=ema)
    check(_L().mi355_lw_unit_update_ema(int(rule), ptr(p), ptr(g), ptr(m), ptr(ema), *args, float(ema_decay), cur_stream()))


# ---- AdamP (include/mi355rn.h, csrc/optim_adamp.hip): Adam with the projection of adamp.AdamP, restated from the published package --------------
def _adamp_coef_arrays(name, coef, wdf):
    _need_cuda(coef, wdf)
    if coef.dtype != torch.float32 or coef.dim() != 2 or coef.shape[1] != 2 or coef.shape[0] < 1 or not coef.is_contiguous():
        raise ValueError(f"{name}: coef must be a contiguous CUDA float32 tensor [n_slots, 2], got {coef.dtype} {tuple(coef.shape)}")
    if wdf.dtype != torch.float32 or wdf.dim() != 1 or wdf.numel() < 1:
        raise ValueError(f"{name}: wdf must hold one float32 per tensor")


def adamp_unit_sums(p, g, m, v, pieces, partial, n_slots, step, betas=(0.9, 0.999), eps=1e-8, nesterov=False, grad_scale=1.0):
    """stage (a): partial[k] = (sum ge^2, sum p^2, sum ge*p, sum p*u) over piece k { off, len, slot }, in double, ge = g*grad_scale and u the Adam
    direction of this step formed in registers from the OLD m and v (neither is written); step: the count after this step's increment;
    partial: float64 [n_pieces, 4]"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, m=m, v=v)
    _lw_table("pieces", pieces)
    _need_cuda(partial)
    if partial.dtype != torch.float64 or partial.numel() != 4 * pieces.shape[0] or not partial.is_contiguous():
        raise ValueError(f"partial: expected {pieces.shape[0]} contiguous quadruples of float64, got {partial.dtype} with {partial.numel()} elements")
    check(_L().mi355_adamp_unit_sums(ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(pieces), pieces.shape[0], int(n_slots), float(betas[0]),
                                     float(betas[1]), float(eps), int(step), int(bool(nesterov)), float(grad_scale), ptr(partial), cur_stream()))


def adamp_coef(partial, slots, decide, coef, wdf, mode, lr, weight_decay, eps=1e-8, delta=0.1, wd_ratio=0.1):
    """stage (b) for the tensors of one param group: decide = their records { slot0, n_slots, unit_len, kind } (CUDA int32 [n, 4]); partial
    (float64 [entries, 4]), slots (int32 [n_slots, 2]) and coef (float32 [n_slots, 2]) are the WHOLE arrays, wdf (float32) and mode (int32) the
    group's slices.  Writes coef[slot] = (d, s), wdf[t] and mode[t] (0: none, 1: the units, 2: the layer)"""
    _unit_slots("adamp_coef", slots)
    _adamp_coef_arrays("adamp_coef", coef, wdf)
    _need_cuda(partial, decide, mode)
    nt = decide.shape[0]
    if decide.dtype != torch.int32 or decide.dim() != 2 or decide.shape[1] != 4 or nt < 1:
        raise ValueError(f"adamp_coef: decide must be a contiguous CUDA int32 tensor [n, 4], got {decide.dtype} {tuple(decide.shape)}")
    if partial.dtype != torch.float64 or partial.numel() < 4 or partial.numel() % 4:
        raise ValueError("adamp_coef: partial must be a contiguous float64 tensor of quadruples")
    if coef.shape[0] != slots.shape[0] or wdf.numel() != nt or mode.dtype != torch.int32 or mode.numel() != nt:
        raise ValueError("adamp_coef: coef must hold one pair per slot, wdf one float32 and mode one int32 per tensor record")
    check(_L().mi355_adamp_coef(ptr(partial), partial.numel() // 4, ptr(slots), slots.shape[0], ptr(decide), nt, ptr(coef), ptr(wdf), ptr(mode),
                                float(lr), float(weight_decay), float(eps), float(delta), float(wd_ratio), cur_stream()))


def adamp_update(p, g, m, v, items, tensors, coef, wdf, step, lr, betas=(0.9, 0.999), eps=1e-8, nesterov=False, grad_scale=1.0, ema=None,
                 ema_decay=0.0):
    """stage (c) for the work items of one param group; p, g, m, v (and ema): the flat fp32 arrays the item offsets count from; tensors: the
    records { start, unit_len, slot0 } of ALL tensors; coef [n_slots, 2] and wdf [n_tensors]: the whole arrays of stage (b)"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, m=m, v=v)
    _lw_table("items", items)
    _lw_table("tensors", tensors)
    _adamp_coef_arrays("adamp_update", coef, wdf)
    if wdf.numel() != tensors.shape[0]:
        raise ValueError("adamp_update: wdf must hold one float32 per tensor record")
    args = (n, ptr(items), items.shape[0], ptr(tensors), tensors.shape[0], ptr(coef), coef.shape[0], ptr(wdf), float(lr), float(betas[0]),
            float(betas[1]), float(eps), int(step), int(bool(nesterov)), float(grad_scale))
    if ema is None:
        check(_L().mi355_adamp_update(ptr(p), ptr(g), ptr(m), ptr(v), *args, cur_stream()))
        return
    _flat_f32(n, ema=ema)
    check(_L().mi355_adamp_update_ema(ptr(p), ptr(g), ptr(m), ptr(v), ptr(ema), *args, float(ema_decay), cur_stream()))


# ---- sharpness-aware minimization (include/mi355rn.h, csrc/optim_sam.hip): the SAMOriginal callback of the reference -----------------------
def _sam_kind(kind):
    _need_cuda(kind)
    if kind.dtype != torch.int32 or kind.dim() != 1 or kind.numel() < 1 or not kind.is_contiguous():
        raise ValueError(f"kind: expected a contiguous CUDA int32 tensor with one element per tensor, got {kind.dtype} {tuple(kind.shape)}")


def sam_sumsq(p, g, items, kind, partial, eta, grad_scale=1.0):
    """stage (a), replaces the per-tensor norms of sota_imagenet/callbacks.py:327-337: partial[i] = sum over work item i of w^2 in double,
    w = (g*grad_scale) * max(|p|, eta) for tensors with kind 1 and g*grad_scale for the others; p, g: the flat fp32 arrays the offsets count from"""
    n = p.numel()
    _flat_f32(n, p=p, g=g)
    _lw_table("items", items)
    _sam_kind(kind)
    _need_cuda(partial)
    if partial.dtype != torch.float64 or partial.numel() != items.shape[0]:
        raise ValueError(f"partial: expected {items.shape[0]} float64 elements, got {partial.dtype} with {partial.numel()}")
    check(_L().mi355_sam_sumsq(ptr(p), ptr(g), n, ptr(items), items.shape[0], ptr(kind), kind.numel(), float(eta), float(grad_scale), ptr(partial),
                               cur_stream()))


def sam_scale(partial, rho, out):
    """stage (b), replaces callbacks.py:337 and :297: norm = max(sqrt(sum(partial)), 2e-5) in double over ALL partials of the step;
    out[0] = rho / norm, out[1] = norm (a float32 CUDA tensor of two elements)"""
    _need_cuda(partial, out)
    if partial.dtype != torch.float64 or partial.numel() < 1 or not partial.is_contiguous():
        raise ValueError("sam_scale: partial must be a contiguous float64 tensor")
    if out.dtype != torch.float32 or out.numel() != 2 or not out.is_contiguous():
        raise ValueError("sam_scale: out must hold two float32 elements")
    check(_L().mi355_sam_scale(ptr(partial), partial.numel(), float(rho), ptr(out), cur_stream()))


def sam_perturb(p, g, eps, items, kind, out, eta, grad_scale=1.0):
    """stage (c), replaces callbacks.py:298-306: eps = (max(p*p, eta) * g*grad_scale) * out[0] for kind 1, (g*grad_scale) * out[0] otherwise;
    p += eps.  eps: a flat fp32 array laid out like p"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, eps=eps)
    _lw_table("items", items)
    _sam_kind(kind)
    _need_cuda(out)
    if out.dtype != torch.float32 or out.numel() != 2:
        raise ValueError("sam_perturb: out must be the two float32 elements sam_scale wrote")
    check(_L().mi355_sam_perturb(ptr(p), ptr(g), ptr(eps), n, ptr(items), items.shape[0], ptr(kind), kind.numel(), ptr(out), float(eta),
                                 float(grad_scale), cur_stream()))


def sam_restore(p, eps, items, n_tensors):
    """stage (d), replaces callbacks.py:319-323: p -= eps over the same work items"""
    n = p.numel()
    _flat_f32(n, p=p, eps=eps)
    _lw_table("items", items)
    check(_L().mi355_sam_restore(ptr(p), ptr(eps), n, ptr(items), items.shape[0], int(n_tensors), cur_stream()))


# ---- the SAM callback of the reference (include/mi355rn.h, csrc/optim_sam_lw.hip): one pair of norms per slot -----------------------------------
SAM_THREADS_PER_PIECE = 64  # one wave per piece: profiles/sam_lw_step.json


def _sam_partial(name, partial, entries):
    _need_cuda(partial)
    if partial.dtype != torch.float64 or partial.numel() != 2 * entries or not partial.is_contiguous():
        raise ValueError(f"{name}: partial must hold {entries} contiguous pairs of float64, got {partial.dtype} with {partial.numel()} elements")


def _sam_slots(name, coef, n_slots=None):
    _need_cuda(coef)
    if coef.dtype != torch.float32 or coef.dim() != 1 or coef.numel() < 1 or not coef.is_contiguous() or n_slots not in (None, coef.numel()):
        raise ValueError(f"{name}: coef must be a contiguous CUDA float32 tensor with one element per slot, got {coef.dtype} {tuple(coef.shape)}")


def sam_lw_sumsq(p, g, items, partial, n_tensors, grad_scale=1.0):
    """stage (a), the whole-tensor norms of sota_imagenet/callbacks.py:389-391: partial[i] = (sum of (g*grad_scale)^2, sum of p^2) over work item
    i, in double; p, g: the flat fp32 arrays the offsets count from"""
    n = p.numel()
    _flat_f32(n, p=p, g=g)
    _lw_table("items", items)
    _sam_partial("sam_lw_sumsq", partial, items.shape[0])
    check(_L().mi355_sam_lw_sumsq(ptr(p), ptr(g), n, ptr(items), items.shape[0], int(n_tensors), float(grad_scale), ptr(partial), cur_stream()))


def sam_unit_sumsq(p, g, pieces, partial, n_slots, grad_scale=1.0, threads_per_piece=SAM_THREADS_PER_PIECE):
    """stage (a'), the per-output-unit norms of callbacks.py:269-276, :386-387: the same pair of sums over every piece { off, len, slot } of
    `pieces`, a piece cut from one unit at any element offset; one wave (threads_per_piece 64) or one workgroup (256) per piece"""
    n = p.numel()
    _flat_f32(n, p=p, g=g)
    _lw_table("pieces", pieces)
    _sam_partial("sam_unit_sumsq", partial, pieces.shape[0])
    check(_L().mi355_sam_unit_sumsq(ptr(p), ptr(g), n, ptr(pieces), pieces.shape[0], int(n_slots), float(grad_scale), ptr(partial),
                                    int(threads_per_piece), cur_stream()))


def sam_lw_coef(partial, slots, coef, norms):
    """stage (b), callbacks.py:386-395 for every slot: (Sg, Sp) = the slot's entries of partial[] in a fixed order; gn = max(sqrt(Sg), 1e-5),
    wn = max(sqrt(Sp), 1e-3) in float32; coef[slot] = wn / gn, norms[slot] = (gn, wn).  slots: CUDA int32 [n_slots, 2] of (first, count)"""
    _need_cuda(partial, slots, norms)
    if partial.dtype != torch.float64 or partial.numel() < 2 or partial.numel() % 2 or not partial.is_contiguous():
        raise ValueError("sam_lw_coef: partial must be a contiguous float64 tensor of pairs")
    if slots.dtype != torch.int32 or slots.dim() != 2 or slots.shape[1] != 2 or slots.shape[0] < 1 or not slots.is_contiguous():
        raise ValueError(f"sam_lw_coef: slots must be a contiguous CUDA int32 tensor [n, 2], got {slots.dtype} {tuple(slots.shape)}")
    _sam_slots("sam_lw_coef", coef, slots.shape[0])
    if norms.dtype != torch.float32 or norms.numel() != 2 * slots.shape[0] or not norms.is_contiguous():
        raise ValueError("sam_lw_coef: norms must hold two contiguous float32 per slot")
    check(_L().mi355_sam_lw_coef(ptr(partial), partial.numel() // 2, ptr(slots), slots.shape[0], ptr(coef), ptr(norms), cur_stream()))


def sam_lw_perturb(p, g, eps, items, tensors, coef, rho, grad_scale=1.0):
    """stage (c), callbacks.py:395-404: eps = (coef[slot] * (g*grad_scale)) * rho, p += eps over the work items of all tensors; the slot of an
    element from its tensor's record { start, unit_len, slot0 } in `tensors`.  eps: a flat fp32 array laid out like p"""
    n = p.numel()
    _flat_f32(n, p=p, g=g, eps=eps)
    _lw_table("items", items)
    _lw_table("tensors", tensors)
    _sam_slots("sam_lw_perturb", coef)
    check(_L().mi355_sam_lw_perturb(ptr(p), ptr(g), ptr(eps), n, ptr(items), items.shape[0], ptr(tensors), tensors.shape[0], ptr(coef),
                                    coef.numel(), float(rho), float(grad_scale), cur_stream()))


def _check_disjoint(what, spans):
    """ValueError if one of the spans [(first element, length)], given in sorted order, begins before the one in front of it ends: two workgroups
    would rewrite the same elements.  what: "<op>: the record" or "<op>: the item", as the message names it"""
    end = None
    for first, length in spans:
        if end is not None and first < end:
            raise ValueError(f"{what} at offset {first} overlaps the one before it (which ends at {end})")
        end = first + length


# ---- orthogonal initialisation (include/mi355rn.h, csrc/init_ortho.hip): the OrthoInitClb callback of the reference ---------------------------------
def ortho_init_(flat, records_host, records_dev, gain=1.0):
    """replaces the nn.init.orthogonal_ calls of sota_imagenet/callbacks.py:260-265: every matrix of the table, filled with N(0,1) draws by the
    caller, becomes in place the sign-fixed Q of its QR factorisation times gain.  flat: the fp32 array the offsets count from; records_host:
    [(off, rows, chans, taps)] (item_plan.ortho_records), records_dev: the same table packed for the device (item_plan.pack_records with
    ORTHO_FIELDS, CUDA int64 [n, 3]).  Records that overlap would race and raise here; one that does not fit the array is the kernel's to refuse.
    Returns status (CUDA int32 per record: 0 done, 1 rank-deficient input, 2 the record does not fit), not read back."""
    _flat_f32(flat.numel(), flat=flat)
    _need_cuda(records_dev)
    n_mats = len(records_host)
    if records_dev.dtype != torch.int64 or records_dev.dim() != 2 or records_dev.shape[1] != 3 or records_dev.shape[0] != n_mats or n_mats < 1:
        raise ValueError(f"records_dev: expected a CUDA int64 tensor [{n_mats}, 3] of 24-byte records, got {records_dev.dtype} {tuple(records_dev.shape)}")
    if records_dev.device != flat.device:
        raise ValueError("ortho_init_: the records and the array must live on one device")
    _check_disjoint("ortho_init_: the record", ((off, max(rows, 0) * max(chans, 0) * max(taps, 0)) for off, rows, chans, taps in sorted(records_host)))
    status = torch.empty(n_mats, dtype=torch.int32, device=flat.device)
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
    _flat_f32(flat.numel(), flat=flat)
    _lw_table("items_dev", items_dev)
    if items_dev.device != flat.device:
        raise ValueError("weight_norm_rows_: the items and the array must live on one device")
    if items_host is not None:
        if len(items_host) != items_dev.shape[0]:
            raise ValueError(f"items_dev: expected {len(items_host)} records, got {items_dev.shape[0]}")
        wnorm_check_items(items_host)
    status = torch.empty(items_dev.shape[0], dtype=torch.int32, device=flat.device)
    check(_L().mi355_weight_norm_rows(ptr(flat), flat.numel(), ptr(items_dev), items_dev.shape[0], ptr(status), cur_stream()))
    return status


# ---- forward weight transform per filter (include/mi355rn.h, csrc/weight_std.hip): weight_standardization / the ForwardWeightNorm callback ---------
# stated once for the host; include/mi355rn.h states them for the library (MI355_WS_*) and tests/test_weight_std_host.py holds the two together
WS_STANDARDISE, WS_CENTRE = 1, 2
WS_EPS = 1e-5  # oracle/bresnet50_ref.py::ws


def _ws_args(who, n_rows, rows_dev, invstd, **arrays):
    n = next(iter(arrays.values())).numel()
    _flat_f32(n, **arrays)
    _lw_table("rows_dev", rows_dev)
    _need_cuda(invstd)
    if invstd.dtype != torch.float32 or invstd.numel() != rows_dev.shape[0]:
        raise ValueError(f"invstd: expected {rows_dev.shape[0]} float32 elements (one per row of the table), got {invstd.dtype} with {invstd.numel()}")
    if len({t.device for t in (rows_dev, invstd, *arrays.values())}) != 1:
        raise ValueError(f"{who}: the table, invstd and the arrays must live on one device")
    return n


def weight_std_rows_fwd(w, w_hat, invstd, rows_dev, mode, eps=WS_EPS):
    """w_hat = the per-row transform of w (mode WS_STANDARDISE: (w - mean) / sqrt(var + eps), WS_CENTRE: w - mean), invstd[k] = row k's factor,
    in ONE launch.  w, w_hat: flat fp32 arrays of one size the row offsets count from — the same tensor bakes the transform in place —;
    rows_dev: [(first element, row_len)] packed for the device (item_plan.ws_rows, pack_records; CUDA int64 [n, 2]); a row that does not fit
    the array is skipped by the kernel.  Elements outside the rows are neither read nor written."""
    n = _ws_args("weight_std_rows_fwd", rows_dev.shape[0], rows_dev, invstd, w=w, w_hat=w_hat)
    check(_L().mi355_weight_std_rows_fwd(ptr(w), ptr(w_hat), ptr(invstd), n, ptr(rows_dev), rows_dev.shape[0], int(mode), float(eps), cur_stream()))


def weight_std_rows_bwd(g, w_hat, invstd, dw, rows_dev, mode, beta=0.0, row_begin=0, row_end=None):
    """dw = beta * dw + (the gradient wrt w of the rows [row_begin, row_end) of the table, from g = the gradient wrt w_hat), in ONE launch:
    invstd * (g - mean(g) - w_hat * mean(g * w_hat)) per row (WS_CENTRE: invstd * (g - mean(g)), invstd as the forward left it: 1)"""
    row_end = rows_dev.shape[0] if row_end is None else int(row_end)
    if not 0 <= int(row_begin) < row_end <= rows_dev.shape[0]:
        raise ValueError(f"weight_std_rows_bwd: rows [{row_begin}, {row_end}) of a table of {rows_dev.shape[0]}")
    n = _ws_args("weight_std_rows_bwd", rows_dev.shape[0], rows_dev, invstd, g=g, w_hat=w_hat, dw=dw)
    check(_L().mi355_weight_std_rows_bwd(ptr(g), ptr(w_hat), ptr(invstd), ptr(dw), n, ptr(rows_dev), int(row_begin), row_end, int(mode), float(beta),
                                         cur_stream()))


# ---- forward spectral normalisation per convolution (include/mi355rn.h, csrc/spectral_norm.hip): the ForwardSpectralNorm callback -------------------
# stated once for the host; include/mi355rn.h states them for the library (MI355_SN_*) and tests/test_spectral_host.py holds the two together
SN_EPS = 1e-12  # torch.nn.utils.parametrizations.spectral_norm's eps (rounded to float32 where it is used)
SN_WARM_ITERS = 15  # the power iterations torch runs at registration
SN_SLABS = 16  # row slabs per matrix of the column sums: the scratch holds one partial sum per slab and element of v


def spectral_scratch(u, v):
    """the float64 scratch spectral_fwd / spectral_bwd need for vectors of these sizes, on their device"""
    return torch.empty(_L().mi355_spectral_scratch_doubles(u.numel(), v.numel()), dtype=torch.float64, device=u.device)


def _sn_args(who, mats_dev, u, v, sigma, scratch, **arrays):
    n = next(iter(arrays.values())).numel()
    _flat_f32(n, **arrays)
    _need_cuda(mats_dev, u, v, sigma, scratch)
    if mats_dev.dtype != torch.int64 or mats_dev.dim() != 2 or mats_dev.shape[1] != 4 or mats_dev.shape[0] < 1:
        raise ValueError(f"mats_dev: expected a CUDA int64 tensor [n, 4] of 32-byte records, got {mats_dev.dtype} {tuple(mats_dev.shape)}")
    for name, t in (("u", u), ("v", v)):
        if t.dtype != torch.float32 or t.numel() < 1:
            raise ValueError(f"{name}: expected a non-empty float32 tensor, got {t.dtype} with {t.numel()}")
    if sigma.dtype != torch.float32 or sigma.numel() != mats_dev.shape[0]:
        raise ValueError(f"sigma: expected {mats_dev.shape[0]} float32 elements (one per matrix), got {sigma.dtype} with {sigma.numel()}")
    need = _L().mi355_spectral_scratch_doubles(u.numel(), v.numel())
    if scratch.dtype != torch.float64 or scratch.numel() < need:
        raise ValueError(f"scratch: expected {need} float64 elements (spectral_scratch), got {scratch.dtype} with {scratch.numel()}")
    if len({t.device for t in (mats_dev, u, v, sigma, scratch, *arrays.values())}) != 1:
        raise ValueError(f"{who}: the table, u, v, sigma, the scratch and the arrays must live on one device")
    return n


def spectral_fwd(w, w_hat, u, v, sigma, scratch, mats_dev, iters):
    """`iters` power iterations of every matrix of the table on (u, v) — 1: a training forward; 0: the eval rule, u and v untouched —, sigma[i] of
    matrix i, and, unless w_hat is None, w_hat = w / sigma (w_hat is w: in place).  w, w_hat: flat fp32 arrays of one size the offsets count
    from; mats_dev: item_plan.spectral_mats packed with SPECTRAL_FIELDS (CUDA int64 [n, 4]); u, v: the sizes spectral_mats returns.  A matrix
    that does not fit the arrays is skipped by the kernels; elements outside the matrices are neither read nor written."""
    arrays = dict(w=w) if w_hat is None else dict(w=w, w_hat=w_hat)
    n = _sn_args("spectral_fwd", mats_dev, u, v, sigma, scratch, **arrays)
    check(_L().mi355_spectral_fwd(ptr(w), ptr(w_hat), ptr(u), ptr(v), ptr(sigma), ptr(scratch), n, u.numel(), v.numel(), ptr(mats_dev),
                                  mats_dev.shape[0], int(iters), cur_stream()))


def spectral_bwd(g, w_hat, u, v, sigma, dw, scratch, mats_dev, beta=0.0, row_begin=0, row_end=None):
    """dw = beta * dw + (the gradient wrt w, from g = the gradient wrt w_hat = w / sigma with u, v, sigma constants) for the matrices whose rows
    are the slice [row_begin, row_end) of u — whole matrices —: (g - (sum g * w_hat) * u_r * v_c) / sigma"""
    row_end = u.numel() if row_end is None else int(row_end)
    if not 0 <= int(row_begin) < row_end <= u.numel():
        raise ValueError(f"spectral_bwd: rows [{row_begin}, {row_end}) of u[{u.numel()}]")
    n = _sn_args("spectral_bwd", mats_dev, u, v, sigma, scratch, g=g, w_hat=w_hat, dw=dw)
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
    return dict(gram=torch.empty(n_gram, dtype=torch.float32, device=device),
                partial=torch.empty(L.mi355_ortho_loss_partial_floats(n_items), dtype=torch.float32, device=device),
                tile_ss=torch.empty(n_tiles, dtype=torch.float64, device=device),
                stats=torch.empty(L.mi355_ortho_loss_stats_floats(n_mats) // 4, 4, dtype=torch.float32, device=device),
                loss=torch.empty((), dtype=torch.float32, device=device))


def _ol_args(who, tables, scratch, **arrays):
    n = next(iter(arrays.values())).numel()
    _flat_f32(n, **arrays)
    for name, cols in _OL_TABLES:
        t = tables[name]
        _need_cuda(t)
        if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != cols or t.shape[0] < 1:
            raise ValueError(f"{name}: expected a CUDA int64 tensor [n, {cols}] of {8 * cols}-byte records, got {t.dtype} {tuple(t.shape)}")
    L = _L()
    n_mats, n_tiles, n_items = (tables[k].shape[0] for k in ("mats", "tiles", "items"))
    want = dict(gram=(torch.float32, 1), partial=(torch.float32, L.mi355_ortho_loss_partial_floats(n_items)), tile_ss=(torch.float64, n_tiles),
                stats=(torch.float32, L.mi355_ortho_loss_stats_floats(n_mats)), loss=(torch.float32, 1))
    for name, (dt, need) in want.items():
        t = scratch[name]
        _need_cuda(t)
        if t.dtype != dt or t.numel() < need or (name in ("stats", "loss") and t.numel() != need):
            raise ValueError(f"{name}: expected {need} {dt} elements (ortho_loss_scratch), got {t.dtype} with {t.numel()}")
    if len({t.device for t in (*tables.values(), *scratch.values(), *arrays.values())}) != 1:
        raise ValueError(f"{who}: the tables, the scratch and the arrays must live on one device")
    return n


def ortho_loss_fwd(w, tables, scratch, min_norm):
    """replaces the loop of sota_imagenet/callbacks.py:138-156 in 3 launches: for every matrix of the tables G = W W^T - I (scratch["gram"]), its
    Frobenius norm F, the gate F / O > min_norm and the gradient's coefficient (scratch["stats"]), and scratch["loss"] = sum of the gated F, which
    is returned (a view, not read back).  w: the flat fp32 array the offsets count from; tables: item_plan.ortho_loss_cut(.., OL_TILE, OL_KSLAB)
    packed for the device — mats (ORTHO_LOSS_FIELDS), tiles and gitems (OL_TILE_FIELDS), items (OL_ITEM_FIELDS).  A record that does not fit is
    skipped by the kernels; elements outside the matrices are not read."""
    n = _ol_args("ortho_loss_fwd", tables, scratch, w=w)
    s = scratch
    check(_L().mi355_ortho_loss_fwd(ptr(w), n, ptr(s["gram"]), s["gram"].numel(), ptr(s["partial"]), ptr(s["tile_ss"]), ptr(s["stats"]), ptr(s["loss"]),
                                    ptr(tables["mats"]), tables["mats"].shape[0], ptr(tables["tiles"]), tables["tiles"].shape[0],
                                    ptr(tables["items"]), tables["items"].shape[0], float(min_norm), cur_stream()))
    return s["loss"]


def _dev_scalar(name, s, like):
    _need_cuda(s)
    if s.dtype != torch.float32 or s.numel() != 1 or s.device != like.device:
        raise ValueError(f"{name}: expected ONE float32 element on {like.device} (the upstream gradient stays on the device), got {s.dtype} with "
                         f"{s.numel()} on {s.device}")


def ortho_loss_bwd(w, dw, tables, scratch, s, accumulate=True):
    """dw (+)= s * (2 / F) G W for every matrix whose gate ortho_loss_fwd left open, in ONE launch, from the gram and stats it left in `scratch`;
    s: a 1-element CUDA fp32 tensor (the upstream gradient times the callback's weight); accumulate=False overwrites the matrices' elements
    (zeros where the gate is closed) and leaves every other element of dw alone."""
    n = _ol_args("ortho_loss_bwd", tables, scratch, w=w, dw=dw)
    _dev_scalar("s", s, w)
    check(_L().mi355_ortho_loss_bwd(ptr(w), ptr(dw), n, ptr(scratch["gram"]), scratch["gram"].numel(), ptr(scratch["stats"]), ptr(s),
                                    ptr(tables["mats"]), tables["mats"].shape[0], tables["tiles"].shape[0], ptr(tables["gitems"]),
                                    tables["gitems"].shape[0], int(bool(accumulate)), cur_stream()))


def norm_loss_scratch(n_items, n_tensors, device):
    """what norm_loss_fwd leaves: part (float64 per item), tensor_loss (float64 per tensor: its mean) and loss (the 0-dim fp32 total)"""
    return dict(part=torch.empty(n_items, dtype=torch.float64, device=device), tensor_loss=torch.empty(n_tensors, dtype=torch.float64, device=device),
                loss=torch.empty((), dtype=torch.float32, device=device))


def _nl_args(who, items_dev, tensors_dev, **arrays):
    n = next(iter(arrays.values())).numel()
    _flat_f32(n, **arrays)
    _lw_table("items_dev", items_dev)
    _lw_table("tensors_dev", tensors_dev)
    if len({t.device for t in (items_dev, tensors_dev, *arrays.values())}) != 1:
        raise ValueError(f"{who}: the tables and the arrays must live on one device")
    return n


def norm_loss_fwd(w, items_dev, tensors_dev, scratch):
    """replaces the loop of sota_imagenet/callbacks.py:213-221 in 2 launches: scratch["loss"] = sum over the tensors of mean_r (1 - |row r|)^2,
    which is returned (a view, not read back).  items_dev, tensors_dev: item_plan.norm_loss_items packed for the device (CUDA int64 [n, 2])."""
    n = _nl_args("norm_loss_fwd", items_dev, tensors_dev, w=w)
    for name, dt, need in (("part", torch.float64, items_dev.shape[0]), ("tensor_loss", torch.float64, tensors_dev.shape[0]), ("loss", torch.float32, 1)):
        t = scratch[name]
        _need_cuda(t)
        if t.dtype != dt or t.numel() != need or t.device != w.device:
            raise ValueError(f"{name}: expected {need} {dt} elements on {w.device} (norm_loss_scratch), got {t.dtype} with {t.numel()} on {t.device}")
    check(_L().mi355_norm_loss_fwd(ptr(w), n, ptr(scratch["part"]), ptr(scratch["tensor_loss"]), ptr(scratch["loss"]), ptr(items_dev), items_dev.shape[0],
                                   ptr(tensors_dev), tensors_dev.shape[0], cur_stream()))
    return scratch["loss"]


def norm_loss_bwd(w, dw, items_dev, tensors_dev, s, accumulate=True):
    """dw (+)= s * (2 / R)(n_r - 1) / n_r * w for every row of the tables (0 where n_r == 0), in ONE launch; s as in ortho_loss_bwd"""
    n = _nl_args("norm_loss_bwd", items_dev, tensors_dev, w=w, dw=dw)
    _dev_scalar("s", s, w)
    check(_L().mi355_norm_loss_bwd(ptr(w), ptr(dw), n, ptr(s), ptr(items_dev), items_dev.shape[0], ptr(tensors_dev), tensors_dev.shape[0],
                                   int(bool(accumulate)), cur_stream()))


# ---- the log histogram of |x| (include/mi355rn.h, csrc/optim_hist.hip): the GradDistributionTB callback of the reference ----------------------------
# the bins, stated once for the host; csrc/absbin.h states them for the kernels and tests/test_grad_dist_host.py holds the two together
ABSBIN_BINS, ABSBIN_SHIFT, ABSBIN_K0 = 512, 20, (77 << 3) + 2
ABSBIN_BAD_REP = 2 ** 64 - 1  # what mi355_subsample_counts writes into every count when a rep[t] < 1


def _hist_table(hist, row):
    """the table both counting kernels add into: int32 [n_tensors, row]"""
    if hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[1] != row or hist.shape[0] < 1:
        raise ValueError(f"hist: expected a contiguous CUDA int32 tensor [n_tensors, {row}], got {hist.dtype} {tuple(hist.shape)}")


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
    _flat_f32(src.numel(), src=src)
    _lw_table("items", items)
    _need_cuda(hist)
    _hist_table(hist, ABSBIN_BINS)
    if not (src.device == items.device == hist.device):
        raise ValueError("absbin_hist: the array, the table and the histograms must live on one device")
    check(_L().mi355_absbin_hist(ptr(src), src.numel(), ptr(items), items.shape[0], hist.shape[0], ptr(hist), cur_stream()))


def subsample_counts(hist, rep, subsample, counts, rep_host=None):
    """replaces the [::subsample], torch.cat, second sort and second [::subsample] of callbacks.py:47-50 and :56-59: counts[k] (CUDA int64 [512]) =
    the number of values of the twice-subsampled set in bin k, from the per-tensor histograms hist [n, 512] and rep (CUDA int32 [n]: shown elements
    per counted element, >= 1).  rep lives on the device: a rep < 1 makes the kernel write -1 (ABSBIN_BAD_REP unsigned) into every count; rep_host,
    the same numbers on the host where the caller has them, is tested here and raises ValueError."""
    _need_cuda(hist, rep, counts)
    _hist_table(hist, ABSBIN_BINS)
    if rep.dtype != torch.int32 or rep.dim() != 1 or rep.numel() != hist.shape[0]:
        raise ValueError(f"rep: expected {hist.shape[0]} int32 elements, got {rep.dtype} {tuple(rep.shape)}")
    if counts.dtype != torch.int64 or counts.dim() != 1 or counts.numel() != ABSBIN_BINS:
        raise ValueError(f"counts: expected {ABSBIN_BINS} int64 elements, got {counts.dtype} {tuple(counts.shape)}")
    if not (hist.device == rep.device == counts.device):
        raise ValueError("subsample_counts: the histograms, rep and counts must live on one device")
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
    _flat_f32(src.numel(), src=src)
    _lw_table("items", items)
    _need_cuda(hist, partial)
    _hist_table(hist, TBBIN_ROW)
    if partial.dtype != torch.float64 or tuple(partial.shape) != (items.shape[0], TBBIN_STATS):
        raise ValueError(f"partial: expected a float64 tensor [{items.shape[0]}, {TBBIN_STATS}], got {partial.dtype} {tuple(partial.shape)}")
    if not (src.device == items.device == hist.device == partial.device):
        raise ValueError("tbbin_hist: the array, the table, the histograms and the partial statistics must live on one device")
    edges = _tbbin_dev.get(src.device)
    if edges is None:
        edges = _tbbin_dev[src.device] = torch.from_numpy(tbbin_edges()[TBBIN_POS + 1:].copy()).to(src.device)
    check(_L().mi355_tbbin_hist(ptr(src), src.numel(), ptr(items), items.shape[0], hist.shape[0], ptr(edges), edges.numel(), ptr(hist), ptr(partial),
                                cur_stream()))


# ---- BResNet-50 variant blocks (include/mi355rn.h, csrc/variant.hip) ---------------------------------------------------
def blurpool_fwd(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    check(_L().mi355_blurpool_fwd(dtype_code(x.dtype), ptr(x), ptr(y), N, H, W, C, cur_stream()))
    return y


def blurpool_bwd(dy, x_shape):
    _need_cuda(dy)
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    check(_L().mi355_blurpool_bwd(dtype_code(dy.dtype), ptr(dy), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def avgpool2_fwd(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    y = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    check(_L().mi355_avgpool2_fwd(dtype_code(x.dtype), ptr(x), ptr(y), N, H, W, C, cur_stream()))
    return y


def avgpool2_bwd(dy, x_shape):
    _need_cuda(dy)
    N, H, W, C = x_shape
    dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
    check(_L().mi355_avgpool2_bwd(dtype_code(dy.dtype), ptr(dy), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def maxpool3s1_fwd(x):
    _need_cuda(x)
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    idx = torch.empty((N, H, W, C), dtype=torch.uint8, device=x.device)
    check(_L().mi355_maxpool3s1_fwd(dtype_code(x.dtype), ptr(x), ptr(y), ptr(idx), N, H, W, C, cur_stream()))
    return y, idx


def maxpool3s1_bwd(dy, idx):
    _need_cuda(dy, idx)
    N, H, W, C = dy.shape
    dx = torch.empty_like(dy)
    check(_L().mi355_maxpool3s1_bwd(dtype_code(dy.dtype), ptr(dy), ptr(idx), ptr(dx), N, H, W, C, cur_stream()))
    return dx


def eca_fwd(x, w):
    """returns (y, pooled [N,C] fp32, gate [N,C] fp32)"""
    _need_cuda(x, w)
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    pooled = torch.empty((N, C), dtype=torch.float32, device=x.device)
    gate = torch.empty((N, C), dtype=torch.float32, device=x.device)
    check(_L().mi355_eca_fwd(dtype_code(x.dtype), ptr(x), ptr(w), w.numel(), ptr(y), ptr(pooled), ptr(gate), N, H * W, C, cur_stream()))
    return y, pooled, gate


def eca_bwd(dy, x, w, pooled, gate, dw=None, beta=0.0):
    """returns (dx, dw [k] fp32); with dw given: dw = beta * dw + the gradient (beta 0: dw is only written)"""
    _need_cuda(dy, x, w, pooled, gate, dw)
    N, H, W, C = x.shape
    dx = torch.empty_like(x)
    if dw is None:
        dw = torch.empty_like(w)
    elif dw.dtype != torch.float32 or dw.numel() != w.numel():
        raise ValueError("eca_bwd: dw must be fp32 with one element per tap")
    ws = torch.empty(2 * N * C + 128 * 9, dtype=torch.float32, device=x.device)  # mi355_eca_bwd: sprod, dpool, dw partials
    check(_L().mi355_eca_bwd(dtype_code(x.dtype), ptr(dy), ptr(x), ptr(w), w.numel(), ptr(pooled), ptr(gate), ptr(dx), ptr(dw), beta, ptr(ws),
                             N, H * W, C, cur_stream()))
    return dx, dw


def weight_std_fwd(w, eps=1e-5):
    """w: [Cout, ...] fp32 contiguous.  returns (w_hat, invstd [Cout])"""
    _need_cuda(w)
    Cout = w.shape[0]
    K = w.numel() // Cout
    w_hat = torch.empty_like(w)
    mean = torch.empty(Cout, dtype=torch.float32, device=w.device)
    invstd = torch.empty(Cout, dtype=torch.float32, device=w.device)
    check(_L().mi355_weight_std_fwd(ptr(w), ptr(w_hat), ptr(mean), ptr(invstd), Cout, K, eps, cur_stream()))
    return w_hat, invstd


def weight_std_bwd(dw_hat, w_hat, invstd, dw=None, beta=0.0):
    """with dw given: dw = beta * dw + the gradient (beta 0: dw is only written)"""
    _need_cuda(dw_hat, w_hat, invstd, dw)
    Cout = w_hat.shape[0]
    if dw is None:
        dw = torch.empty_like(w_hat)
    elif dw.dtype != torch.float32 or dw.numel() != w_hat.numel():
        raise ValueError("weight_std_bwd: dw must be fp32 with the shape of w_hat")
    check(_L().mi355_weight_std_bwd(ptr(dw_hat), ptr(w_hat), ptr(invstd), ptr(dw), beta, Cout, w_hat.numel() // Cout, cur_stream()))
    return dw


def residual_act_fwd(branch, shortcut=None, scale_n=None, act=1):
    _need_cuda(branch, shortcut, scale_n)
    N = branch.shape[0]
    out = torch.empty_like(branch)
    check(_L().mi355_residual_act_fwd(dtype_code(branch.dtype), ptr(branch), ptr(scale_n), ptr(shortcut), ptr(out), N, branch.numel() // N, act, cur_stream()))
    return out


def residual_act_bwd(dout, out, scale_n=None, act=1, want_shortcut=True):
    _need_cuda(dout, out, scale_n)
    N = out.shape[0]
    db = torch.empty_like(out)
    ds = torch.empty_like(out) if want_shortcut else None
    check(_L().mi355_residual_act_bwd(dtype_code(out.dtype), ptr(dout), ptr(out), ptr(scale_n), ptr(db), ptr(ds), N, out.numel() // N, act, cur_stream()))
    return db, ds


def keep_scale(n, p, seed, counter, device):
    keep = torch.empty(n, dtype=torch.float32, device=device)
    check(_L().mi355_keep_scale(ptr(keep), n, float(p), int(seed), int(counter), cur_stream()))
    return keep
