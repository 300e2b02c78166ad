"""ORACLE (test infrastructure — never imported by the product path).

One BACKWARD segment of the ResNet-50 executor (sota_imagenet_amd/csrc/resnet_exec.cpp: backward_fc, backward_block,
backward_stem), restated in plain torch on the CPU from the executor's documented semantics.  Every stage is rebuilt
from the tensors the executor STORED for that stage (teacher forcing, as tests/test_resnet_gpu.py does for the forward):
ReLU masks are the stored activations (`a1 > 0`, `a2 > 0`, `out > 0`), BatchNorm statistics are recomputed from the
stored conv output, and the incoming gradient is the one the previous segment left, so an error in one stage does not
leak into the reference of the next.

Conventions: activations and gradients are NHWC (what `debug_tensor` returns), conv weights are torch's OIHW
(`named_parameters()`), the incoming gradient of a block is the gradient with respect to the block's output BEFORE that
output's ReLU mask (resnet_exec.cpp, backward_block: "gradient wrt the block output, BEFORE its ReLU mask"), and the
returned one is the same thing for the block below.

Arithmetic is fp64 unless `lowprec` is given.  The `lowprec` chain is the YARDSTICK of tests/test_resnet_bwd_gpu.py — what
the same mathematics loses in the run's number format, computed from this file alone:
  "fp32"  the identical chain in fp32 arithmetic
  "bf16"  fp64 arithmetic, but every gradient tensor the executor stores in bf16 between two stages is rounded to bf16.
          The storage points (resnet_exec.cpp, with the line of each call):
            dy3        :655  bn_backward(c, b.c3, G, b.out_bits, nullptr, B1, ...)          "B1 = dy3"
            dyd        :660  bn_backward(c, b.ds, G, b.out_bits, nullptr, B2, ...)          "B2 = dyd"
            shortcut   :661  conv_dgrad_compact(c, b.ds, B2, c->gsub, ws)                   "gsub = shortcut gradient at half resolution"
                       :662  conv_dgrad(c, b.ds, B2, Gn, nullptr, ws)                       "Gn = shortcut gradient" (MI355_DS_COMPACT=0, stride 1)
            da2        :666  conv_dgrad(c, b.c3, B1, B3, ...)                               "B3 = da2 (+ bn2's sums)"
            dy2        :667  bn_backward(c, b.c2, B3, b.a2_bits, nullptr, B3, ...)          "B3 = dy2"
            da1        :670  conv_dgrad(c, b.c2, B3, B4, ...)                               "B4 = da1 (+ bn1's sums)"
            dy1        :671  bn_backward(c, b.c1, B4, b.a1_bits, nullptr, B4, ...)          "B4 = dy1"
            outgoing   :677  conv_dgrad(c, b.c1, B4, Gn, sub2 ? c->gsub : Gn, ...)          "Gn = dx_in" (entry block)
                       :681  conv_dgrad(c, b.c1, B4, G, G, s, b.out_bits, ...)              "G = dx_in" (identity block)
                       conv1's data gradient + the shortcut addend, rounded once; the identity shortcut's addend is the incoming
                       bf16 tensor under its mask and is not rounded again
            head       :641  launch_gap_bwd(c->dtype, c->dpooled, c->cur_dout, ...)         backward_fc (dpooled itself stays fp32)
            stem       :711  launch_maxpool_bwd(c->dtype, G, c->pool_idx, B1, ...)          the pool's input gradient: a pixel's window
                       :707  launch_stem_bwd_apply(c->dtype, G, c->pool_idx, ...)           sum, which the fused form "rounds as the kernel stored it"
                                                                                            (tests/test_resnet_gpu.py, stem A/B test); then
                                                                                            "B1 = dy of the stem conv" (:695, :713)
          Parameter gradients are fp32 in the executor and are not rounded.
"""
import torch
import torch.nn.functional as F

EPS = 1e-5


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def arith(t, lowprec):
    """a stored tensor / parameter in the chain's arithmetic type"""
    return t.detach().to(torch.float32 if lowprec == "fp32" else torch.float64)


def stored(t, lowprec):
    """a gradient tensor at one of the executor's storage points (module docstring)"""
    return t.bfloat16().to(t.dtype) if lowprec == "bf16" else t


def relu_mask(g, act):
    return g * (act > 0).to(g.dtype)


def bn_stats(y2):
    """batch statistics of y2 [M, C], biased variance: (mean, invstd, M)"""
    M = y2.shape[0]
    return y2.mean(0), (y2.var(0, unbiased=False) + EPS).rsqrt(), M


def bn_bwd(y, gamma, g):
    """training-mode BatchNorm backward on the stored conv output y under the gradient g: (dy, dgamma, dbeta)"""
    C = y.shape[-1]
    y2, g2 = y.reshape(-1, C), g.reshape(-1, C)
    mean, invstd, M = bn_stats(y2)
    xhat = (y2 - mean) * invstd
    dbeta = g2.sum(0)
    dgamma = (g2 * xhat).sum(0)
    dx = gamma * invstd * (g2 - dbeta / M - xhat * dgamma / M)
    return dx.reshape(y.shape), dgamma, dbeta


def conv_bwd(x, w, dy, stride, pad, need_dx=True):
    """(gradient wrt the NHWC input x or None, gradient wrt the OIHW weight w) of conv2d(x, w, stride, pad) under dy"""
    xn, dyn = _nchw(x), _nchw(dy)
    dw = torch.nn.grad.conv2d_weight(xn, w.shape, dyn, stride=stride, padding=pad)
    dx = _nhwc(torch.nn.grad.conv2d_input(xn.shape, w, dyn, stride=stride, padding=pad)) if need_dx else None
    return dx, dw


def shortcut_bwd(t, p, Gm, stride, lowprec=None):
    """the shortcut's share of the gradient wrt the block input under the MASKED incoming gradient Gm: (parameter gradients, gradient).
    Identity block: Gm itself.  Entry block: downsample BN backward on yd, then the 1x1 downsample conv backward at its stride."""
    if "yd" not in t:
        return {}, Gm
    dyd, dg, db = bn_bwd(t["yd"], p["downsample.1.weight"], Gm)
    dyd = stored(dyd, lowprec)
    dsc, dw = conv_bwd(t["prev"], p["downsample.0.weight"], dyd, stride, 0)
    return {"downsample.0.weight": dw, "downsample.1.weight": dg, "downsample.1.bias": db}, stored(dsc, lowprec)


def block_bwd(t, p, G, stride, lowprec=None):
    """One bottleneck block.
    t       stored tensors, NHWC: prev (the block below's out, or stem.p0), y1, a1, y2, a2, y3, out, and yd for an entry block
    p       the block's parameters by their names inside the block (conv1.weight, bn1.weight, ..., downsample.0.weight,
            downsample.1.weight), conv weights already rounded to the run's dtype
    G       incoming gradient (wrt out, before out's ReLU mask)
    stride  of conv2 and of the downsample conv
    Returns ({parameter name inside the block: gradient}, gradient wrt prev — again before prev's mask)."""
    t = {k: arith(v, lowprec) for k, v in t.items()}
    p = {k: arith(v, lowprec) for k, v in p.items()}
    grads = {}
    Gm = relu_mask(arith(G, lowprec), t["out"])
    dy3, grads["bn3.weight"], grads["bn3.bias"] = bn_bwd(t["y3"], p["bn3.weight"], Gm)
    dy3 = stored(dy3, lowprec)
    da2, grads["conv3.weight"] = conv_bwd(t["a2"], p["conv3.weight"], dy3, 1, 0)
    da2 = stored(da2, lowprec)
    dy2, grads["bn2.weight"], grads["bn2.bias"] = bn_bwd(t["y2"], p["bn2.weight"], relu_mask(da2, t["a2"]))
    dy2 = stored(dy2, lowprec)
    da1, grads["conv2.weight"] = conv_bwd(t["a1"], p["conv2.weight"], dy2, stride, 1)
    da1 = stored(da1, lowprec)
    dy1, grads["bn1.weight"], grads["bn1.bias"] = bn_bwd(t["y1"], p["bn1.weight"], relu_mask(da1, t["a1"]))
    dy1 = stored(dy1, lowprec)
    dmain, grads["conv1.weight"] = conv_bwd(t["prev"], p["conv1.weight"], dy1, 1, 0)
    gs, dsc = shortcut_bwd(t, p, Gm, stride, lowprec)
    grads.update(gs)
    return grads, stored(dmain + dsc, lowprec)


def head_bwd(dlogits, pooled, w, shape, lowprec=None):
    """Global average pool + FC.  shape: (N, H, W, C) of the last block's output.
    Returns ({fc.weight, fc.bias: gradient}, dpooled, gradient wrt the last block's output)."""
    dl, pooled, w = arith(dlogits, lowprec), arith(pooled, lowprec), arith(w, lowprec)
    N, H, W, C = shape
    grads = {"fc.weight": dl.t() @ pooled, "fc.bias": dl.sum(0)}
    dpooled = dl @ w
    out = (dpooled / (H * W)).view(N, 1, 1, C).expand(N, H, W, C).contiguous()
    return grads, dpooled, stored(out, lowprec)


def tie_pick(eq):
    """which of a window's maxima takes the gradient: eq [N, C, 9, L] marks the window elements equal to the maximum, row-major;
    the FIRST one wins, as in torch's max_pool2d backward and in the executor's argmax codes"""
    k = eq.shape[2]
    rank = torch.arange(k, 0, -1, dtype=torch.int64).view(1, 1, k, 1)
    return (eq.to(torch.int64) * rank).argmax(2, keepdim=True)


def maxpool_bwd(a, dp):
    """3x3 / stride 2 / pad 1 max pool backward: a NHWC pool input, dp NHWC gradient wrt the pool output -> gradient wrt a"""
    an, dpn = _nchw(a), _nchw(dp)
    N, C, H, W = an.shape
    win = F.unfold(F.pad(an, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, C, 9, -1)
    pick = tie_pick(win == win.max(2, keepdim=True).values)
    route = torch.zeros_like(win).scatter_(2, pick, dpn.reshape(N, C, 1, -1))
    dx = F.fold(route.view(N, C * 9, -1), (H + 2, W + 2), 3, stride=2)
    return _nhwc(dx[:, :, 1:-1, 1:-1])


def stem_a0(y, gamma, beta, dtype):
    """relu(bn(y)) as the executor pools it: rounded to the run's dtype"""
    C = y.shape[-1]
    mean, invstd, _ = bn_stats(y.reshape(-1, C))
    a0 = torch.relu((y - mean) * invstd * gamma + beta)
    return a0.to(dtype).to(y.dtype)


def stem_bwd(dp0, y, gamma, beta, x, wshape, dtype, lowprec=None):
    """The stem: conv 7x7/2 -> BN -> ReLU -> max pool 3x3/2.
    dp0  gradient wrt stem.p0; y the stored conv1.y; x the input image NHWC, rounded to the run's dtype; wshape conv1.weight's
    OIHW shape; dtype the run's storage type (torch.float32 / torch.bfloat16).  There is no input gradient.
    Returns {conv1.weight, bn1.weight, bn1.bias: gradient}."""
    dp0, y, gamma, beta, x = (arith(v, lowprec) for v in (dp0, y, gamma, beta, x))
    a0 = stem_a0(y, gamma, beta, dtype)
    da0 = stored(maxpool_bwd(a0, dp0), lowprec)
    dy, dg, db = bn_bwd(y, gamma, relu_mask(da0, a0))
    dy = stored(dy, lowprec)
    dw = torch.nn.grad.conv2d_weight(_nchw(x), wshape, _nchw(dy), stride=2, padding=3)
    return {"conv1.weight": dw, "bn1.weight": dg, "bn1.bias": db}


# ---- the network as backward segments (the order of the executor's grad_segments: head, layer4.2 ... layer1.0, stem) ----
BLOCKS = [(f"layer{st}.{i}", 2 if (i == 0 and st > 1) else 1) for st, nb in zip((1, 2, 3, 4), (3, 4, 6, 3)) for i in range(nb)]
SEGMENTS = ["head"] + [pre for pre, _ in reversed(BLOCKS)] + ["stem"]


def segment_bwd(seg, T, P, G, dtype, lowprec=None, image=None):
    """Backward segment `seg` (a name of SEGMENTS) from stored tensors.
    T      callable: the executor's debug-tensor name (stem.p0, conv1.y, layerS.I.conv1.y / .a1 / .a2 / .out / .downsample.0.y,
           pooled) -> that stored tensor, NHWC
    P      {torchvision parameter name: fp32 master value}; conv weights are rounded to `dtype` here, as the executor's are
    G      the segment's incoming gradient: dlogits for the head, else the gradient the segment above left
    dtype  the run's storage type; image: the NCHW input batch (stem only)
    Returns {parameter name: gradient, ..., "out": outgoing gradient (not for the stem), "dpooled": (head only)}."""
    q = lambda w: w.to(dtype).to(w.dtype)
    if seg == "head":
        grads, dpooled, out = head_bwd(G, T("pooled"), P["fc.weight"], T(BLOCKS[-1][0] + ".out").shape, lowprec)
        return {**grads, "dpooled": dpooled, "out": out}
    if seg == "stem":
        x = _nhwc(q(image))
        return stem_bwd(G, T("conv1.y"), P["bn1.weight"], P["bn1.bias"], x, P["conv1.weight"].shape, dtype, lowprec)
    i = [pre for pre, _ in BLOCKS].index(seg)
    stride = BLOCKS[i][1]
    t = {"prev": T(BLOCKS[i - 1][0] + ".out" if i > 0 else "stem.p0"), "y1": T(seg + ".conv1.y"), "a1": T(seg + ".a1"),
         "y2": T(seg + ".conv2.y"), "a2": T(seg + ".a2"), "y3": T(seg + ".conv3.y"), "out": T(seg + ".out")}
    if seg.endswith(".0"):
        t["yd"] = T(seg + ".downsample.0.y")
    p = {k[len(seg) + 1:]: (q(v) if v.dim() == 4 else v) for k, v in P.items() if k.startswith(seg + ".")}
    grads, dprev = block_bwd(t, p, G, stride, lowprec)
    return {**{f"{seg}.{k}": v for k, v in grads.items()}, "out": dprev}
