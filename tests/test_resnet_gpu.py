"""Whole-network parity of the native executor against the torch-CPU oracle (oracle/resnet50_ref.py).

north_star bar: fp32 logits within 1e-3 rel of the CPU forward ("rel" = max|got-ref| / max|ref| over the tensor),
loss curve reproduced on the same seed.

Gradients and multi-step curves of a randomly initialised ResNet-50 on noise images are ill-conditioned:
torch's OWN fp32 CPU path deviates ~1.5e-2 (relative L2) from an fp64 run of the same oracle, and its bf16
autocast path ~1e-1..3e-1 on the logits.  Those quantities are therefore judged with the reference as the
yardstick: the native path's distance to the fp64 oracle must not exceed ~the torch-CPU path's own distance
to it in the same precision (factor + floor written at each assert).  Layer-wise, teacher-forced checks pin every
stage without the chaotic amplification: the forward here (test_teacher_forced_layers), the backward segment by segment
in test_resnet_bwd_gpu.py.
"""
import os

import pytest
import torch

from oracle import ops_ref as R
from oracle import resnet50_ref as O
from sota_imagenet_amd.synth import synthetic_batch

pytestmark = pytest.mark.gpu


def nerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def l2err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def gflat(params):
    return torch.cat([p.grad.detach().double().cpu().flatten() for p in params])


def ce64(out, target, s=0.1):
    lp = torch.log_softmax(out.double(), 1)
    return ((1 - s) * -(lp * target.double()).sum(1) + s * -lp.mean(1)).mean()


def build(dtype, num_classes=1000):
    from sota_imagenet_amd.models import resnet50

    m = resnet50(num_classes=num_classes, dtype=dtype)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.cuda(), sd


def oracle_step(sd, data, target, mode):
    """one forward+backward of the oracle in fp64 / fp32 / torch-CPU bf16 autocast: (logits, loss, flat grads, model)."""
    ref = O.make_reference(sd)
    ref.train()
    if mode == "fp64":
        ref = ref.double()
        out = ref(data.double())
        loss = ce64(out, target)
    elif mode == "fp32":
        out = ref(data)
        loss = O.smooth_ce(out, target, 0.1)
    else:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = ref(data)
        loss = O.smooth_ce(out.float(), target, 0.1)
    loss.backward()
    return out.detach(), loss.item(), gflat(ref.parameters()), ref


def oracle_step_one_thread(sd, data, target, mode):
    """oracle_step on ONE intra-op thread: torch-CPU's reduction order (and so its fp32 distance to fp64, the yardstick below)
    depends on the thread count — at 8 x 64 px it is 2.0e-2 on one thread but 9.9e-3 on 4 or more — so the bound is pinned
    to one host-independent value instead of the host's core count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return oracle_step(sd, data, target, mode)
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("shape", [(8, 64), (2, 224), (3, 96)])
def test_fp32_forward_backward_matches_cpu(dev, shape):
    from sota_imagenet_amd.losses import CrossEntropyLoss

    N, S = shape
    m, sd = build("fp32")
    data, target = synthetic_batch(N, S, seed=0, index=3)
    o32, l32, g32, ref = oracle_step_one_thread(sd, data, target, "fp32")
    o64, l64, g64, _ = oracle_step_one_thread(sd, data, target, "fp64")

    m.train()
    out = m(data.cuda())
    loss = CrossEntropyLoss(smoothing=0.1)(out, target.cuda())
    loss.backward()
    torch.cuda.synchronize()

    assert nerr(out, o32) < 1e-3, "logits vs the CPU fp32 forward (north_star: 1e-3 rel)"
    assert nerr(out, o64) < 1e-3, "logits vs the fp64 oracle"
    assert abs(loss.item() - l32) < 1e-4 * abs(l32)
    # gradients: no further from the fp64 oracle than 1.5x torch-CPU fp32's own distance (+1e-3 floor)
    yard = l2err(g32, g64)
    got = l2err(gflat(m.parameters()), g64)
    assert got < 1.5 * yard + 1e-3, f"grad rel-L2 vs fp64: native {got:.3e}, torch-cpu fp32 {yard:.3e}"
    # the classifier gradient does not pass through the ill-conditioned part: tight
    rp = dict(ref.named_parameters())
    mp = dict(m.named_parameters())
    assert nerr(mp["fc.weight"].grad, rp["fc.weight"].grad) < 1e-3
    assert nerr(mp["fc.bias"].grad, rp["fc.bias"].grad) < 1e-4
    rb = dict(ref.named_buffers())
    for name, b in m.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b.item()) == int(rb[name].item()) == 1
        else:
            assert nerr(b, rb[name]) < 1e-3, name


def test_fp32_eval_forward_matches_cpu(dev):
    N, S = 3, 64
    m, sd = build("fp32")
    ref = O.make_reference(sd)
    # give the running statistics non-trivial values first (one training forward on both sides)
    data, target = synthetic_batch(N, S, seed=1, index=0)
    ref.train()
    ref(data)
    m.train()
    with torch.no_grad():
        m(data.cuda())
    ref.eval()
    m.eval()
    d2, _ = synthetic_batch(N, S, seed=1, index=1)
    with torch.no_grad():
        assert nerr(m(d2.cuda()), ref(d2)) < 1e-3


def _native_curve(m, batches, lrs):
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.optim import SGD

    crit = CrossEntropyLoss(smoothing=0.1)
    opt = SGD([{"params": list(m.parameters())}], lr=0.0, momentum=0.9, weight_decay=3e-5)
    opt.attach_model(m)
    m.train()
    losses = []
    for (data, target), lr in zip(batches, lrs):
        for g in opt.param_groups:
            g["lr"] = lr
        loss = crit(m(data.cuda()), target.cuda())
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_loss_curve_matches_cpu(dev, dtype):
    """8 SGD-momentum steps (warm-up shape of configs/hydra_exp/1.r50_baseline.yaml:41-44, peak LR scaled by the
    linear rule to the small batch), same seed, same batches.  Step 0 must agree tightly; later steps are judged
    against the fp64 oracle with the torch-CPU fp32 curve as yardstick (the trajectory is chaotic)."""
    N, S, steps = 16, 64, 8
    m, sd = build(dtype)
    batches = [synthetic_batch(N, S, seed=0, index=i) for i in range(steps)]
    stages = [dict(ep=(0, 1), lr=(0.0005, 0.004), mode="linear")]
    lrs = [O.phase_lr(stages, 0, i, steps) for i in range(steps)]
    l32, _ = O.train_steps(O.make_reference(sd), batches, lrs, momentum=0.9, weight_decay=3e-5, smoothing=0.1)
    l64, _ = O.train_steps(O.make_reference(sd).double(), [(d.double(), t.double()) for d, t in batches], lrs,
                           momentum=0.9, weight_decay=3e-5, smoothing=0.1)
    losses = _native_curve(m, batches, lrs)
    from test_golden_gpu import check_curve

    check_curve(losses, l32, l64, dtype)


def test_bf16_forward_backward_vs_cpu_yardstick(dev):
    from sota_imagenet_amd.losses import CrossEntropyLoss

    N, S = 2, 224
    m, sd = build("bf16")
    data, target = synthetic_batch(N, S, seed=0, index=5)
    o64, l64, g64, _ = oracle_step(sd, data, target, "fp64")
    ob, lb, gb, _ = oracle_step(sd, data, target, "bf16")
    m.train()
    out = m(data.cuda())
    loss = CrossEntropyLoss(smoothing=0.1)(out, target.cuda())
    loss.backward()
    yard, got = l2err(ob, o64), l2err(out, o64)
    assert got < 1.5 * yard + 2e-2, f"bf16 logits rel-L2 vs fp64: native {got:.3e}, torch-cpu bf16 autocast {yard:.3e}"
    assert abs(loss.item() - l64) < 2e-2 * l64
    g = gflat(m.parameters())
    assert torch.isfinite(g).all()
    assert l2err(g, g64) < 1.5 * l2err(gb, g64) + 5e-2


IGEMM8_TILES = ["224x256", "256x256f", "256x128f", "224x128", "256x256k", "224x128kf"]  # MI355_IGEMM8 values (conv_igemm8.hip)


@pytest.mark.parametrize("dtype,tol,big", [("fp32", 2e-5, None), ("bf16", 2e-2, None), ("bf16", 2e-2, "1"), ("bf16", 2e-2, "3")] +
                         [("bf16", 2e-2, "8:" + t) for t in IGEMM8_TILES])
def test_teacher_forced_layers(dev, dtype, tol, big, monkeypatch):
    """Every forward stage of the executor, re-derived by the oracle FROM THE EXECUTOR'S OWN INPUT to that stage
    (saved activations read back through the debug hook): conv, BN(+ReLU), residual add, maxpool, GAP, FC."""
    if big is not None and big.startswith("8:"):  # the 8-wave ping-pong kernel, that tile wherever it is legal
        monkeypatch.setenv("MI355_IGEMM8", big[2:])
    elif big is not None:  # force the 256x256 ("1") / 256x128 8-wave 3-stage ("3") conv tiles, normally chosen only at
        monkeypatch.setenv("MI355_IGEMM8", "0")
        monkeypatch.setenv("MI355_IGEMM_BIG", big)  # training-size batches, on every layer whose channel count allows
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    N, S = 4, 64
    key = (N, S, S)
    m, sd = build(dtype)
    data, _ = synthetic_batch(N, S, seed=3, index=0)
    m.train()
    with torch.no_grad():
        logits = m(data.cuda())
    P = {k: v.float() for k, v in sd.items()}
    T = lambda name: m.debug_tensor(key, name).float().cpu()
    q = lambda t: t.to(tdt).float()  # the rounding the native path applies to weights / stored activations

    def check_bn(bn, x, out, residual=None, relu=True):
        ref, _, _, mean, invstd = R.bn_train(x, P[bn + ".weight"], P[bn + ".bias"], torch.zeros_like(P[bn + ".bias"]),
                                             torch.ones_like(P[bn + ".bias"]), residual, relu)
        assert nerr(out, ref) < max(tol, 1e-5), bn
        assert nerr(T(bn + ".save_mean"), mean) < 1e-4 and nerr(T(bn + ".save_invstd"), invstd) < 1e-4, bn
        return ref

    x0 = R.nchw_to_nhwc(q(data))
    y = T("conv1.y")
    assert nerr(y, R.conv2d_fwd(x0, q(R.oihw_to_krsc(P["conv1.weight"])), 2, 3)) < tol, "stem conv"
    # the stem's BN + ReLU + max pool are one kernel: the full-resolution activation is never stored
    a0, _, _, mean, invstd = R.bn_train(y, P["bn1.weight"], P["bn1.bias"], torch.zeros_like(P["bn1.bias"]),
                                        torch.ones_like(P["bn1.bias"]), None, True)
    assert nerr(T("bn1.save_mean"), mean) < 1e-4 and nerr(T("bn1.save_invstd"), invstd) < 1e-4, "bn1"
    p0 = T("stem.p0")
    assert nerr(p0, R.maxpool(q(a0))[0]) < max(tol, 1e-5), "bn1 + maxpool"
    prev = p0
    for st, nb in zip((1, 2, 3, 4), (3, 4, 6, 3)):
        for i in range(nb):
            pre = f"layer{st}.{i}"
            stride = 2 if (i == 0 and st > 1) else 1
            w = lambda n: q(R.oihw_to_krsc(P[f"{pre}.{n}.weight"]))
            y1 = T(f"{pre}.conv1.y")
            assert nerr(y1, R.conv2d_fwd(prev, w("conv1"), 1, 0)) < tol, pre + ".conv1"
            a1 = T(f"{pre}.a1")
            check_bn(f"{pre}.bn1", y1, a1)
            y2 = T(f"{pre}.conv2.y")
            assert nerr(y2, R.conv2d_fwd(a1, w("conv2"), stride, 1)) < tol, pre + ".conv2"
            a2 = T(f"{pre}.a2")
            check_bn(f"{pre}.bn2", y2, a2)
            y3 = T(f"{pre}.conv3.y")
            assert nerr(y3, R.conv2d_fwd(a2, w("conv3"), 1, 0)) < tol, pre + ".conv3"
            out = T(f"{pre}.out")
            if i == 0:
                yd = T(f"{pre}.downsample.0.y")
                assert nerr(yd, R.conv2d_fwd(prev, w("downsample.0"), stride, 0)) < tol, pre + ".downsample"
                sc, _, _, _, _ = R.bn_train(yd, P[f"{pre}.downsample.1.weight"], P[f"{pre}.downsample.1.bias"],
                                            torch.zeros(yd.shape[-1]), torch.ones(yd.shape[-1]), None, False)
                check_bn(f"{pre}.bn3", y3, out, residual=sc)
            else:
                check_bn(f"{pre}.bn3", y3, out, residual=prev)
            prev = out
    pooled = T("pooled")
    assert nerr(pooled, R.gap(prev)) < 1e-5
    ref_logits = pooled @ P["fc.weight"].t() + P["fc.bias"]
    assert nerr(logits, ref_logits) < 1e-4, "fc"


def test_gradient_accumulation_and_segments(dev):
    """two backward passes without zero_grad accumulate (accumulate_steps > 1, arg_parser.py:85-86);
    segment-wise backward with a sync hook equals the one-shot backward."""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    N, S = 2, 64
    m, _ = build("fp32")
    crit = CrossEntropyLoss(smoothing=0.1)
    data, target = synthetic_batch(N, S, seed=2, index=0)
    data, target = data.cuda(), target.cuda()
    m.train()
    crit(m(data), target).backward()
    g1 = m.flat_grads.clone()
    crit(m(data), target).backward()  # not cleaned: accumulates
    assert nerr(m.flat_grads, 2 * g1) < 1e-5
    m.mark_grads_clean()
    seen = []
    m._grad_sync = lambda s, b, e: seen.append((s, b, e))
    crit(m(data), target).backward()
    m._grad_sync = None
    assert [s for s, _, _ in seen] == list(range(18))
    assert nerr(m.flat_grads, g1) < 1e-5


def _train_steps(dtype, env, steps=3, N=8, S=64):
    """`steps` SGD steps of a freshly built model whose executor is created under the environment `env`;
    returns (per-step logits, per-step flat gradients, final flat parameters), all on the CPU."""
    import os

    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.optim import SGD

    from sota_imagenet_amd import native

    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        native.lib().mi355_reload_knobs()   # (library switches are cached: MI355_POOL_KEYS, ...; executor switches are read at context creation)
        m, _ = build(dtype)
        crit = CrossEntropyLoss(smoothing=0.1).cuda()
        opt = SGD([{"params": list(m.parameters())}], lr=0.05, momentum=0.9, weight_decay=3e-5)
        opt.attach_model(m)
        m.train()
        outs, grads = [], []
        for i in range(steps):
            data, target = synthetic_batch(N, S, seed=11, index=i)
            out = m(data.cuda())
            loss = crit(out, target.cuda())
            opt.zero_grad()
            loss.backward()
            outs.append(out.detach().float().cpu())
            grads.append(m.flat_grads.detach().clone().cpu())
            opt.step()
        return outs, grads, m.flat_params.detach().clone().cpu()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        native.lib().mi355_reload_knobs()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_side_stream_is_bitwise_neutral_and_runs_are_reproducible(dev, dtype):
    """The weight-gradient / downsample side stream only re-orders independent kernels: logits, every gradient and the
    updated parameters must be BIT-identical with it on and off (a missing event dependency shows up here), and two runs
    with it on must be bit-identical to each other (no atomics, fixed summation orders)."""
    a = _train_steps(dtype, {"MI355_WGRAD_STREAM": "1"})
    b = _train_steps(dtype, {"MI355_WGRAD_STREAM": "0"})
    c = _train_steps(dtype, {"MI355_WGRAD_STREAM": "1"})
    for i, (x, y, z) in enumerate(zip(a[0], b[0], c[0])):
        assert torch.equal(x, y) and torch.equal(x, z), f"logits of step {i}"
    for i, (x, y, z) in enumerate(zip(a[1], b[1], c[1])):
        assert torch.equal(x, y), f"gradients of step {i}: side stream on vs off"
        assert torch.equal(x, z), f"gradients of step {i}: run to run"
    assert torch.equal(a[2], b[2]) and torch.equal(a[2], c[2])


def test_stem_pool_on_packed_keys_is_bitwise_the_compare_select_kernel(dev):
    """the stem's BN + ReLU + 3x3/2 max pool on packed (value << 16 | 15 - tap) keys (misc.hip bn_relu_maxpool3_kernel: integer maxima instead of a compare
    and two selects per window element) against the compare / select form (MI355_POOL_KEYS=0): the pooled values, the argmax codes and the ReLU bits
    feed everything downstream and the stem's backward, so three SGD steps must agree bit for bit in logits, every gradient and the parameters"""
    a = _train_steps("bf16", {"MI355_POOL_KEYS": "1"})
    b = _train_steps("bf16", {"MI355_POOL_KEYS": "0"})
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), f"logits of step {i}"
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"gradients of step {i}"
    assert torch.equal(a[2], b[2])


def test_fused_bn_backward_sums_match_standalone_reduce(dev):
    """bf16: BN-backward sums accumulated in the dgrad epilogue (default) vs the standalone reduce kernels — different
    summation order, same quantities.  A re-ordered fp32 sum moves a few bf16 roundings of dy, and backward through a
    randomly initialised ResNet-50 amplifies any such perturbation (see the module docstring), so the comparison is made
    per backward segment: the first segments (fc, layer4.2 — reached through at most three fused layers) must agree to
    1e-4, and the drift may only grow gradually from there; a wrong mask or layer pairing is O(1) at the first block."""
    from sota_imagenet_amd.models import resnet50

    f = _train_steps("bf16", {"MI355_FUSE_BN_BWD": "1"}, steps=1)
    u = _train_steps("bf16", {"MI355_FUSE_BN_BWD": "0"}, steps=1)
    assert torch.equal(f[0][0], u[0][0])  # the forward pass is identical
    segs = resnet50(dtype="bf16").grad_segments
    errs = [l2err(f[1][0][b:e], u[1][0][b:e]) for b, e in segs]
    assert errs[0] == 0.0, "fc gradients do not depend on any BN backward"
    assert errs[1] < 1e-4, f"layer4.2: {errs[1]:.3e}"
    assert max(errs[:4]) < 2e-2, f"layer4: {errs[:4]}"  # measured 2e-6, 8e-4, 4e-3: bf16 rounding flips, amplified
    assert max(errs) < 0.3, f"per-segment drift {['%.1e' % x for x in errs]}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stem_backward_from_the_pooled_gradient_matches_pool_backward_kernel(dev, dtype):
    """The stem's BN backward gathers the max pool's backward on the fly from the pooled gradient (default) vs the stand-alone
    pool-backward kernel + plain BN backward (MI355_STEM_FUSED=0): the same per-pixel gradient values (the gather rounds the
    window sum as the kernel stored it), per-channel sums taken in a different order.  Nothing above the stem may change at all;
    the stem's own gradients (conv1.weight, bn1.weight / bias: the last backward segment) agree to summation-order noise."""
    from sota_imagenet_amd.models import resnet50

    f = _train_steps(dtype, {"MI355_STEM_FUSED": "1"}, steps=1)
    u = _train_steps(dtype, {"MI355_STEM_FUSED": "0"}, steps=1)
    assert torch.equal(f[0][0], u[0][0])
    segs = resnet50(dtype=dtype).grad_segments
    for b, e in segs[:-1]:
        assert torch.equal(f[1][0][b:e], u[1][0][b:e])
    b, e = segs[-1]
    assert f[1][0][b:e].abs().max() > 0
    err = l2err(f[1][0][b:e], u[1][0][b:e])
    assert err < (1e-5 if dtype == "fp32" else 2e-3), f"stem segment: {err:.3e}"


@pytest.mark.parametrize("forced", ["1", "3"])
@pytest.mark.parametrize("fuse", ["0", "1"])
def test_256_wide_conv_tiles_in_backward_match_128_wide(dev, fuse, forced, monkeypatch):
    """The 256x256 igemm tile is chosen by a rule that only fires at training-size batches.  Forward coverage is
    test_teacher_forced_layers[bf16-big]; here the SAME forward (128-wide) is followed by a backward with the 256-wide
    tile ("1": 256x256; "3": 256x128, 8 waves, 3-stage ring) forced on every dgrad whose channel count allows (with and
    without the BN-backward epilogue) and by one with 128-wide tiles.  A dgrad output element sums its k-steps in the same order in both; only the grouping of the
    fused BN sums differs, so the gradients must agree tightly at the top of the network and drift only by bf16 rounding
    flips further down."""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    monkeypatch.setenv("MI355_FUSE_BN_BWD", fuse)
    grads = []
    for big in (forced, "0"):
        monkeypatch.setenv("MI355_IGEMM_BIG", "0")
        m, _ = build("bf16")
        m.train()
        data, target = synthetic_batch(8, 64, seed=11, index=0)
        loss = CrossEntropyLoss(smoothing=0.1).cuda()(m(data.cuda()), target.cuda())
        monkeypatch.setenv("MI355_IGEMM_BIG", big)
        loss.backward()
        torch.cuda.synchronize()
        grads.append(m.flat_grads.detach().clone().cpu())
        segs = m.grad_segments
    errs = [l2err(grads[0][b:e], grads[1][b:e]) for b, e in segs]
    # fc: exact; layer4.2: exact without the fused sums, ~2e-6 with them (its bn1/bn2 sums are grouped differently)
    assert errs[0] == 0.0 and errs[1] < 1e-5, f"fc / layer4.2: {errs[:2]}"
    assert errs[2] < 5e-3, f"layer4.1: {errs[2]:.3e}"
    assert max(errs) < 0.3, f"per-segment drift {['%.1e' % x for x in errs]}"


@pytest.mark.parametrize("tile", IGEMM8_TILES)
@pytest.mark.parametrize("fuse", ["0", "1"])
def test_igemm8_tiles_in_backward_match_128_wide(dev, fuse, tile, monkeypatch):
    """The same for the 8-wave ping-pong kernel (conv_igemm8.hip): identical forward, then a backward with `tile` forced on
    every dgrad whose shape allows (plain, + shortcut addend under the ReLU mask, + BN-backward sums) against one with
    the 4-wave 128-wide tiles.  Both sum a dgrad element's k-steps in one fixed order each (different between the two:
    MFMA shape and, with the k suffix, tap order), so fc is exact and the top block agrees to fp32 rounding of the sums."""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    monkeypatch.setenv("MI355_FUSE_BN_BWD", fuse)
    monkeypatch.setenv("MI355_IGEMM_BIG", "0")
    grads = []
    for t in (tile, "0"):
        monkeypatch.setenv("MI355_IGEMM8", "0")
        m, _ = build("bf16")
        m.train()
        data, target = synthetic_batch(8, 64, seed=11, index=0)
        loss = CrossEntropyLoss(smoothing=0.1).cuda()(m(data.cuda()), target.cuda())
        monkeypatch.setenv("MI355_IGEMM8", t)
        loss.backward()
        torch.cuda.synchronize()
        grads.append(m.flat_grads.detach().clone().cpu())
        segs = m.grad_segments
    errs = [l2err(grads[0][b:e], grads[1][b:e]) for b, e in segs]
    assert errs[0] == 0.0 and errs[1] < 2e-3, f"fc / layer4.2: {errs[:2]}"
    assert max(errs[:4]) < 2e-2, f"layer4: {errs[:4]}"
    assert max(errs) < 0.3, f"per-segment drift {['%.1e' % x for x in errs]}"


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_baseline_batch_rule_selected_variants(dev, dtype, monkeypatch):
    """BASELINE.json's batch (N = 256, 224 px), default environment: the kernel variants the launch rules pick only at
    training size (bf16: the 8-wave 224x256 / 256x128 tiles, the 4-wave 256x256 / 256x128-3-stage / 128x64 tiles;
    fp32: the stream-K tail; split-K plans of the weight gradients).
      forward   teacher forced: conv outputs of layers that hit each variant, recomputed by the oracle from the executor's
                own input on a subset of the images (a conv is per-image); BN statistics over the whole batch
      loss      step-0 loss against the torch-CPU oracle's forward of the same batch
      backward  the same backward with every rule switched to the small tiles (checked against the oracle at small N by
                the tests above): fc exact, top block tight, gradual drift below"""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    tol = 2e-5 if dtype == "fp32" else 2e-2
    N, S = 256, 224
    key = (N, S, S)
    m, sd = build(dtype)
    data, target = synthetic_batch(N, S, seed=0, index=0)
    m.train()
    crit = CrossEntropyLoss(smoothing=0.1).cuda()
    out = m(data.cuda())
    loss = crit(out, target.cuda())
    loss.backward()
    torch.cuda.synchronize()
    g_rule = m.flat_grads.detach().clone().cpu()
    if dtype == "bf16":
        # WHICH kernel every convolution of the step went to: the executor's own record against the committed table (a regression in
        # a selection rule — a row capacity, a divisibility test — would leave every number below green and cost a millisecond)
        want = {}
        for ln in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_table_bs256_bf16.txt")):
            name, *kv = ln.split()
            want[name] = dict(x.split("=", 1) for x in kv)
        got = m.kernel_table(key)
        diff = {k: (got.get(k), want[k]) for k in want if got.get(k) != want[k]}
        assert not diff and set(got) == set(want), f"kernel selection changed (`python tools/kernel_table.py --write` on the GPU box writes gpurun_out/kernel_table_bs256_bf16.txt: copy it to tests/golden/): {diff}"
    P = {k: v.float() for k, v in sd.items()}
    T = lambda name: m.debug_tensor(key, name)
    q = lambda t: t.to(tdt).float()
    img = [0, 1, 100, 255]
    # (conv, its input tensor, stride, pad): 3x3 of every stage (layer1: 128x64 tile; layer2: 128x128; layer3: 224x256;
    # layer4: 256x128 fat), long 1x1s (layer3/4 conv1, conv3: 224x256), a stride-2 3x3 and a stride-2 downsample
    checks = [("layer1.1.conv2", "layer1.1.a1", 1, 1), ("layer2.2.conv2", "layer2.2.a1", 1, 1), ("layer3.3.conv2", "layer3.3.a1", 1, 1),
              ("layer4.1.conv2", "layer4.1.a1", 1, 1), ("layer3.2.conv1", "layer3.1.out", 1, 0), ("layer3.4.conv3", "layer3.4.a2", 1, 0),
              ("layer4.2.conv1", "layer4.1.out", 1, 0), ("layer4.2.conv3", "layer4.2.a2", 1, 0), ("layer3.0.conv2", "layer3.0.a1", 2, 1),
              ("layer4.0.downsample.0", "layer3.5.out", 2, 0), ("layer2.0.conv1", "layer1.2.out", 1, 0)]
    for conv, src, stride, pad in checks:
        x = T(src)[img].float().cpu()
        y = T(conv + ".y").float().cpu()
        w = q(R.oihw_to_krsc(P[conv + ".weight"]))
        assert nerr(y[img], R.conv2d_fwd(x, w, stride, pad)) < tol, conv
        bn = conv.replace("conv", "bn") if "downsample" not in conv else conv.replace("downsample.0", "downsample.1")
        y2 = y.reshape(-1, y.shape[-1]).double()
        mean, var = y2.mean(0), y2.var(0, unbiased=False)
        assert nerr(T(bn + ".save_mean").cpu(), mean.float()) < 1e-4, bn
        assert nerr(T(bn + ".save_invstd").cpu(), (var + 1e-5).rsqrt().float()) < 1e-4, bn
    # step-0 loss against the oracle's own forward (fp32: tight; bf16: the stored-activation rounding, 2e-2 as elsewhere)
    ref = O.make_reference(sd)
    ref.train()
    with torch.no_grad():
        loss_ref = O.smooth_ce(ref(data), target, 0.1).item()
    assert abs(loss.item() - loss_ref) < (1e-4 if dtype == "fp32" else 2e-2) * loss_ref, (loss.item(), loss_ref)
    # backward: rule-selected variants against the small tiles.  bf16: the tile rules are read per launch, so the SAME
    # model repeats the forward (rule tiles, identical saved activations) and only the backward switches.  fp32: stream-K
    # is a property of the executor, so a second model runs the whole step without it (forward differs by fp32 summation
    # order only; bounds as in test_fp32_stream_k_tail_matches_whole_tiles).
    if dtype == "bf16":
        m.mark_grads_clean()
        loss2 = crit(m(data.cuda()), target.cuda())
        assert loss2.item() == loss.item()
        monkeypatch.setenv("MI355_IGEMM8", "0")
        monkeypatch.setenv("MI355_IGEMM_BIG", "0")
        loss2.backward()
        torch.cuda.synchronize()
        g_small = m.flat_grads.detach().clone().cpu()
        top, l4 = 2e-3, 2e-2
    else:
        monkeypatch.setenv("MI355_STREAM_K", "0")
        m2, _ = build(dtype)
        m2.train()
        loss2 = crit(m2(data.cuda()), target.cuda())
        loss2.backward()
        torch.cuda.synchronize()
        assert abs(loss2.item() - loss.item()) < 1e-5 * abs(loss.item())
        g_small = m2.flat_grads.detach().clone().cpu()
        top, l4 = 1e-4, 5e-2
    errs = [l2err(g_rule[b:e], g_small[b:e]) for b, e in m.grad_segments]
    assert errs[0] < top and max(errs[:4]) < l4, f"fc / layer4: {errs[:4]}"
    assert max(errs) < 0.3, f"per-segment drift {['%.1e' % x for x in errs]}"


def _segmented_backward(m, loss, key, record=None, replay=None):
    """loss.backward() as one native call per segment (the data-parallel hook's path); after segment k the gradient the next segment
    starts from is copied into `record`, or replaced by replay[k] (mi355_resnet50_force_grad)"""
    nseg = len(m.grad_segments)

    def hook(k, b, e):
        if k >= nseg - 1:
            return
        if record is not None:
            record.append(m.debug_tensor(key, "grad.cur"))
        if replay is not None:
            m.force_grad(key, replay[k])

    m._grad_sync, m._grad_sync_points = hook, None
    try:
        loss.backward()
        torch.cuda.synchronize()
    finally:
        m._grad_sync = None


def test_backward_of_the_baseline_batch_teacher_forced_segment_by_segment(dev, monkeypatch):
    """BASELINE.json's batch, bf16: the backward of the default kernel selection (generated po / pk / pw / dconv / wg kernels, 8-wave
    tiles) against the backward of the round-3 implicit-GEMM kernels with the small tiles — fed the SAME incoming gradient segment by
    segment (arm A's, replayed into arm B before each block), so a segment's gradients differ by that segment's own kernels only and the
    band does not have to absorb sixteen blocks of drift: every segment within 2e-3 (measured 1e-4 at most; the free-running comparison
    allows 0.3 at the stem).
    The replaced tensor's BN-backward sums are re-reduced from it (bn_reduce), so bn3 of every block is also the check of the fused
    epilogue sums against the stand-alone reduction."""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    N, S = 256, 224
    key = (N, S, S)
    m, _ = build("bf16")
    data, target = synthetic_batch(N, S, seed=3, index=0)
    m.train()
    crit = CrossEntropyLoss(smoothing=0.1).cuda()
    rec = []
    _segmented_backward(m, crit(m(data.cuda()), target.cuda()), key, record=rec)
    g_a = m.flat_grads.detach().clone()
    assert len(rec) == len(m.grad_segments) - 1 and rec[0].shape == (N, 7, 7, 2048) and rec[-1].shape == (N, 56, 56, 64)
    # the same split backward again, nothing replaced: the same bits (splitting the native call changes no kernel)
    m.mark_grads_clean()
    _segmented_backward(m, crit(m(data.cuda()), target.cuda()), key)
    assert torch.equal(m.flat_grads, g_a)
    # arm B: every generated family and the large tiles off for the backward; the forward (and so every saved activation) is arm A's
    m.mark_grads_clean()
    loss = crit(m(data.cuda()), target.cuda())
    for k, v in (("MI355_DCONV", "0"), ("MI355_IGEMM8", "0"), ("MI355_IGEMM_BIG", "0")):
        monkeypatch.setenv(k, v)  # (the fixture re-reads the library's switches)
    _segmented_backward(m, loss, key, replay=rec)
    g_b = m.flat_grads.detach().clone()
    table = m.kernel_table(key)
    assert all(v["dgrad"].startswith(("igemm<", "-")) and v["wgrad"].startswith("wgrad<") for v in table.values()), table
    errs = [l2err(g_a[b:e].cpu(), g_b[b:e].cpu()) for b, e in m.grad_segments]
    print("teacher-forced per-segment errors:", ["%.1e" % x for x in errs])
    assert errs[0] == 0.0, errs[0]
    assert max(errs) < 2e-3, f"per-segment error under teacher forcing {['%.1e' % x for x in errs]}"


def test_an_executor_switch_outside_its_domain_fails_the_creation(dev, monkeypatch):
    """the executor's environment switches (MI355_WGRAD_STREAM, MI355_STREAM_K, MI355_FUSE_BN_BWD, MI355_STEM_FUSED, MI355_DS_COMPACT, the MI355_FP8_* ones) have
    closed domains, read once at context creation: a mistyped value is an error with the switch's name, not a silent default"""
    from sota_imagenet_amd.models import resnet50

    m = resnet50(dtype="bf16").to(dev)
    x = torch.zeros(2, 3, 64, 64, device=dev)
    monkeypatch.setenv("MI355_WGRAD_STREAM", "off")
    with pytest.raises(RuntimeError, match="MI355_WGRAD_STREAM=off"):
        m.eval()(x)
    monkeypatch.setenv("MI355_WGRAD_STREAM", "0")
    assert m.eval()(x).shape == (2, 1000)


@pytest.mark.parametrize("S", [160, 224, 320])
def test_config5_batch_512_progressive_sizes(dev, S):
    """BASELINE.json configs[4]'s per-GPU shapes: batch 512 at the progressive-resize sizes 160 / 224 / 320 px, bf16, default
    launch rules (the largest tensors of the path: 1.68 GB activations at 320 px, just inside the 2 GiB buffer-descriptor
    range the kernels index with).  Teacher-forced like the N = 256 test: conv outputs of one layer per stage re-derived by the
    oracle from the executor's own inputs on a few images (first, middle, last — the last row tiles are the ragged ones),
    whole-batch BN statistics, a finite step-0 loss near ln(1000), finite gradients of every segment."""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    N = 512
    key = (N, S, S)
    m, sd = build("bf16")
    data, target = synthetic_batch(N, S, seed=2, index=S)
    m.train()
    loss = CrossEntropyLoss(smoothing=0.1).cuda()(m(data.cuda()), target.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - 6.9078) < 1.0, loss.item()
    g = m.flat_grads.detach()
    assert torch.isfinite(g).all()
    for b, e in m.grad_segments:
        assert g[b:e].abs().max().item() > 0, (b, e)
    P = {k: v.float() for k, v in sd.items()}
    T = lambda name: m.debug_tensor(key, name)
    img = [0, 255, 511]
    for conv, src, stride, pad in [("layer1.2.conv2", "layer1.2.a1", 1, 1), ("layer2.1.conv3", "layer2.1.a2", 1, 0), ("layer3.0.conv2", "layer3.0.a1", 2, 1),
                                   ("layer3.5.conv1", "layer3.4.out", 1, 0), ("layer4.2.conv2", "layer4.2.a1", 1, 1)]:
        x = T(src)[img].float().cpu()
        y = T(conv + ".y")
        w = R.oihw_to_krsc(P[conv + ".weight"]).bfloat16().float()
        assert nerr(y[img].float().cpu(), R.conv2d_fwd(x, w, stride, pad)) < 2e-2, conv
        y2 = y.reshape(-1, y.shape[-1]).double()
        bn = conv.replace("conv", "bn")
        assert nerr(T(bn + ".save_mean").cpu(), y2.mean(0).float().cpu()) < 1e-4, bn
        assert nerr(T(bn + ".save_invstd").cpu(), (y2.var(0, unbiased=False) + 1e-5).rsqrt().float().cpu()) < 1e-4, bn


def test_fp32_stream_k_tail_matches_whole_tiles(dev):
    """fp32 igemm cuts the row tiles of a partial last round along K across workgroups (stream-K) — only when a launch has
    >= 128 tiles, i.e. not at the small shapes of the other tests.  N=64 at 224 px puts the layer-3/4 convs (98 / 25 row
    tiles) into that regime.  Same forward + backward with it on and off: only the order in which a tile's k-steps are
    summed changes (fp32 rounding): logits agree to 1e-3 (measured ~1e-5); gradients drift the way any fp32 rounding
    change does in this ill-conditioned setting (ReLU masks of near-zero activations flip: measured 6e-6 at fc, 7e-3 ...
    1e-2 over layer 4 — torch's own fp32-vs-fp64 distance is 1.5e-2, module docstring).  A lost or doubled partial tile
    is an O(1) error of a whole conv output and would break the logits bound by orders of magnitude."""
    a = _train_steps("fp32", {"MI355_STREAM_K": "1"}, steps=1, N=64, S=224)
    b = _train_steps("fp32", {"MI355_STREAM_K": "0"}, steps=1, N=64, S=224)
    assert l2err(a[0][0], b[0][0]) < 1e-3, "logits"
    from sota_imagenet_amd.models import resnet50

    segs = resnet50(dtype="fp32").grad_segments
    errs = [l2err(a[1][0][s:e], b[1][0][s:e]) for s, e in segs]
    assert errs[0] < 1e-4 and max(errs[:4]) < 5e-2, f"fc / layer4: {errs[:4]}"
    assert max(errs) < 0.3, f"per-segment drift {['%.1e' % x for x in errs]}"
    # and the run-to-run reproducibility claim holds with the hand-offs in play
    c = _train_steps("fp32", {"MI355_STREAM_K": "1"}, steps=1, N=64, S=224)
    assert torch.equal(a[0][0], c[0][0]) and torch.equal(a[1][0], c[1][0])


def test_stream_k_timeout_is_reported(dev, monkeypatch):
    """a stream-K hand-off that times out leaves a wrong tile behind; the kernel's error word must surface as an error of
    the context (MI355_E_STATE -> RuntimeError), not as silently wrong fp32 results.  MI355_SK_DEBUG=mute (read once per
    process, hence the subprocess) makes every contributor withhold its flag, so every owner runs into the spin bound."""
    import os
    import subprocess
    import sys

    code = r"""
import torch
from sota_imagenet_amd.models import resnet50
from sota_imagenet_amd.losses import CrossEntropyLoss
from sota_imagenet_amd.synth import synthetic_batch
m = resnet50(dtype="fp32").cuda()
m.train()
data, target = synthetic_batch(64, 224, seed=1, index=0, device="cuda")
loss = CrossEntropyLoss(smoothing=0.1)(m(data), target)   # layer-3/4 convs: partial last rounds, cut along K
torch.cuda.synchronize()
try:
    m(data)
    print("NO ERROR")
except RuntimeError as e:
    print("RAISED", "stream-K" in str(e))
"""
    env = dict(os.environ, MI355_SK_DEBUG="mute", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert "RAISED True" in out.stdout, (out.stdout[-500:], out.stderr[-1500:])
