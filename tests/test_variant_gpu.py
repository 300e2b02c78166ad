"""BResNet-50 variant blocks (BASELINE configs[3]; csrc/variant.hip, bresnet.py) on the GPU against the torch-CPU oracle
(oracle/ops_ref.py per op, oracle/bresnet50_ref.py whole model).  Tolerances as in test_ops_gpu.py: normalised max error
fp32 2e-5 (1e-4 where a backward sums many terms), bf16 2e-2.

The per-op tests here are the first look at each kernel.  tests/test_variant_ops_gpu.py pins the same kernels against fp64 references
(tests/variant_common.py) where they can go wrong unnoticed here: the segmented row walk and the tie rule of the max pool with its argmax codes, ECA
at every kernel width on data with pooled means of order 1, the accumulate mode of the weight gradients, the null-pointer forms of residual_act,
single values of the keep_scale stream, a launch past the grid cap."""
import pytest
import torch

from oracle import bresnet50_ref as B
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}


def nerr(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def rnd(shape, seed, dtype, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(dtype).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 8, 8, 64), (3, 14, 6, 128), (1, 2, 2, 64)])
def test_pools(dev, dtype, shape):
    from sota_imagenet_amd import ops

    x = rnd(shape, 1, dtype)
    xd = x.to(dev, dtype)
    for name, fwd, bwd, ref in (("blurpool", ops.blurpool_fwd, ops.blurpool_bwd, R.blurpool), ("avgpool2", ops.avgpool2_fwd, ops.avgpool2_bwd, R.avgpool2)):
        y_ref = ref(x)
        dy = rnd(tuple(y_ref.shape), 2, dtype)
        assert nerr(fwd(xd), y_ref) < TOL[dtype], name
        (dx_ref,) = R.grads(ref, [x], dy)
        assert nerr(bwd(dy.to(dev, dtype), shape), dx_ref) < TOL[dtype], name + " bwd"
    xr = torch.relu(x)  # ties inside windows
    y, idx = ops.maxpool3s1_fwd(xr.to(dev, dtype))
    assert nerr(y, R.maxpool3s1(xr)) == 0.0
    dy = rnd(shape, 3, dtype)
    dx = ops.maxpool3s1_bwd(dy.to(dev, dtype), idx)
    assert abs(dx.float().sum().item() - dy.sum().item()) < 1e-2 * dy.abs().sum().item()  # every gradient lands exactly once
    xu = rnd(shape, 4, dtype) + torch.arange(shape[1] * shape[2]).view(1, shape[1], shape[2], 1) * 1e-2  # no ties: unique argmax
    xu = xu.to(dtype).float()
    y, idx = ops.maxpool3s1_fwd(xu.to(dev, dtype))
    (dx_ref,) = R.grads(R.maxpool3s1, [xu], dy)
    assert nerr(ops.maxpool3s1_bwd(dy.to(dev, dtype), idx), dx_ref) < TOL[dtype]


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, (32, 64, 20, 64)), (torch.bfloat16, (32, 64, 16, 64)), (torch.float32, (16, 64, 22, 128))])
def test_maxpool3s1_row_walking_kernels(dev, dtype, shape):
    """the stem-sized launches of the 3x3 / stride-1 max pool take the row-walking kernels (three loads per pixel from a rotating register window; widths with
    W % 3 = 2, 1, 1): values equal to torch's max pool, ties (ReLU zeros) routed to exactly one position, and on tie-free data the gradient torch routes"""
    from sota_imagenet_amd import ops

    F = torch.nn.functional
    x = torch.relu(rnd(shape, 5, dtype)).to(dev, dtype)
    y, idx = ops.maxpool3s1_fwd(x)
    assert torch.equal(y.float(), F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1))
    dy = rnd(shape, 6, dtype).to(dev, dtype)
    dx = ops.maxpool3s1_bwd(dy, idx)
    assert abs(dx.double().sum().item() - dy.double().sum().item()) < 1e-3 * dy.double().abs().sum().item()
    xu = (rnd(shape, 7, torch.float32) + torch.arange(shape[1] * shape[2]).view(1, shape[1], shape[2], 1) * 1e-2).to(dtype).to(dev)
    y, idx = ops.maxpool3s1_fwd(xu)
    xt = xu.float().permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(xt, 3, 1, 1).backward(dy.float().permute(0, 3, 1, 2))
    assert nerr(ops.maxpool3s1_bwd(dy, idx), xt.grad.permute(0, 2, 3, 1)) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [3, 5])
def test_eca(dev, dtype, k):
    from sota_imagenet_amd import ops

    x = rnd((3, 7, 7, 256), 5, dtype)
    w = rnd((k,), 6, torch.float32, 0.8)
    dy = rnd((3, 7, 7, 256), 7, dtype)
    y, pooled, gate = ops.eca_fwd(x.to(dev, dtype), w.to(dev))
    assert nerr(y, R.eca(x, w)) < TOL[dtype]
    dx_ref, dw_ref = R.grads(R.eca, [x, w], dy)
    dx, dw = ops.eca_bwd(dy.to(dev, dtype), x.to(dev, dtype), w.to(dev), pooled, gate)
    assert nerr(dx, dx_ref) < max(TOL[dtype], 1e-4) and nerr(dw, dw_ref) < max(TOL[dtype], 1e-4)


def test_weight_std(dev):
    from sota_imagenet_amd import ops

    for shape in [(64, 3, 3, 32), (256, 1, 1, 64), (512, 3, 3, 512)]:
        w = rnd(shape, 8, torch.float32, 0.3) + 0.05
        g = rnd(shape, 9, torch.float32)
        w_hat, invstd = ops.weight_std_fwd(w.to(dev))
        assert nerr(w_hat, R.weight_std(w)) < 2e-5
        (dw_ref,) = R.grads(R.weight_std, [w], g)
        assert nerr(ops.weight_std_bwd(g.to(dev), w_hat, invstd), dw_ref) < 1e-4


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_residual_act_and_leaky_bn(dev, dtype, act):
    from sota_imagenet_amd import ops

    shape = (4, 6, 6, 128)
    b, s, dout = rnd(shape, 10, dtype), rnd(shape, 11, dtype), rnd(shape, 12, dtype)
    keep = torch.tensor([0.0, 1.25, 1.25, 0.0])
    out = ops.residual_act_fwd(b.to(dev, dtype), s.to(dev, dtype), keep.to(dev), act)
    ref = R.residual_act(b, keep, s, act)
    assert nerr(out, ref) < TOL[dtype]
    db_ref, ds_ref = R.grads(lambda u, v: R.residual_act(u, keep, v, act), [b, s], dout)
    db, ds = ops.residual_act_bwd(dout.to(dev, dtype), ref.to(dev, dtype), keep.to(dev), act)
    assert nerr(db, db_ref) < TOL[dtype] and nerr(ds, ds_ref) < TOL[dtype]
    # ABN: batch norm + activation code (leaky ReLU = the norm_act of the BResNet-50 recipe)
    x = rnd(shape, 13, dtype, 2.0) + 0.3
    g, be = rnd((128,), 14, torch.float32, 0.5) + 1.5, rnd((128,), 15, torch.float32)
    rm, rv = torch.zeros(128), torch.ones(128)
    o_ref, rm_ref, rv_ref = R.bn_act_train(x, g, be, rm, rv, None, act)
    rmd, rvd = rm.to(dev), rv.to(dev)
    o, mean, invstd = ops.bn_fwd_train(x.to(dev, dtype), g.to(dev), be.to(dev), rmd, rvd, relu=act)
    assert nerr(o, o_ref) < TOL[dtype] and nerr(rvd, rv_ref) < (1e-4 if dtype == torch.float32 else 2e-3)
    dx_ref, dg_ref, db_ref = R.grads(lambda u, v, w: R.bn_act_train(u, v, w, rm, rv, None, act)[0], [x, g, be], dout)
    dx, dg, dbe, _ = ops.bn_bwd(dout.to(dev, dtype), o_ref.to(dev, dtype), x.to(dev, dtype), g.to(dev), mean, invstd, relu=act)
    assert nerr(dx, dx_ref) < max(TOL[dtype], 1e-4) and nerr(dg, dg_ref) < max(TOL[dtype], 1e-4) and nerr(dbe, db_ref) < max(TOL[dtype], 1e-4)


def test_keep_scale_statistics(dev):
    from sota_imagenet_amd import ops

    k = ops.keep_scale(200000, 0.2, 3, 5, dev)
    vals = set(torch.unique(k).cpu().tolist())
    assert vals <= {0.0, 1.25} and abs((k > 0).float().mean().item() - 0.8) < 5e-3 and abs(k.mean().item() - 1.0) < 1e-2
    assert torch.equal(k, ops.keep_scale(200000, 0.2, 3, 5, dev)) and not torch.equal(k, ops.keep_scale(200000, 0.2, 3, 6, dev))


def _models(dtype):
    from sota_imagenet_amd.models import resnet50

    m = resnet50(stem_type="deep", antialias=True, attn_type="eca", norm_layer="inplaceabn", norm_act="leaky_relu", drop_rate=0.2,
                 drop_connect_rate=0.2, weight_standardization=True, dtype=dtype)
    ref = B.BResNet50Ref(standardize=True)
    ref.load_state_dict({k: v.detach().clone().contiguous() for k, v in m.state_dict().items()})
    return m.cuda(), ref


def _masks(N, seed):
    g = torch.Generator().manual_seed(seed)
    dc = [None] + [((torch.rand(N, generator=g) >= 0.2 * i / 16).float() / (1 - 0.2 * i / 16)) for i in range(1, 16)]
    do = (torch.rand(N, 2048, generator=g) >= 0.2).float() / 0.8
    return {"dc": dc, "do": do}


def test_bresnet50_fp32_matches_oracle(dev):
    """whole model, training mode, given drop-connect / dropout masks: logits within 1e-3 rel (the north_star bar), loss,
    running statistics, and gradients judged against an fp64 run with the oracle's own fp32 distance as yardstick"""
    from sota_imagenet_amd.synth import synthetic_batch

    N, S = 4, 64
    m, ref = _models("fp32")
    data, target = synthetic_batch(N, S, seed=0, index=1)
    masks = _masks(N, 1)
    m.masks = {"dc": [None if k is None else k.to(dev) for k in masks["dc"]], "do": masks["do"].to(dev)}
    m.train(), ref.train()
    out = m(data.cuda())
    loss = R.smooth_ce(out, target.cuda(), 0.1)
    loss.backward()
    o32 = ref(data, masks)
    l32 = R.smooth_ce(o32, target, 0.1)
    l32.backward()
    ref64 = B.BResNet50Ref(standardize=True).double()
    ref64.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()}, strict=True)
    ref64.load_state_dict({k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in ref.state_dict().items()})
    assert nerr(out, o32) < 1e-3, "logits"
    assert abs(loss.item() - l32.item()) < 1e-4 * l32.item()
    assert nerr(m.bn1.running_var, ref.bn1.running_var) < 1e-4
    gn = torch.cat([p.grad.detach().float().cpu().flatten() for p in m.parameters()])
    gr = torch.cat([p.grad.detach().flatten() for p in ref.parameters()])
    rel = ((gn - gr).norm() / gr.norm()).item()
    assert rel < 2e-2, f"gradients vs the fp32 oracle: rel L2 {rel:.3e}"
    # per tensor in the L2 norm: at 2 x 2 pixels x 4 images one leaky-ReLU sign that two fp32 summation orders decide differently moves single elements by
    # O(1) of the tensor's maximum (seen: 0.27 at one element of layer4.2.conv3.weight after the first conv changed its summation order) and the norm by 1e-3
    for name in ("fc.weight", "layer4.2.se_module.conv.weight", "layer4.2.conv3.weight", "conv1.0.weight"):
        a, b = dict(m.named_parameters())[name].grad.detach().float().cpu(), dict(ref.named_parameters())[name].grad
        assert ((a - b).norm() / b.norm()).item() < 5e-2, name


def test_bresnet50_bf16_trains(dev):
    """bf16 compute, on-device drop-connect / dropout sampling, two SGD steps with the native optimizer; eval mode runs"""
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.optim import SGD
    from sota_imagenet_amd.synth import synthetic_batch

    m, ref = _models("bf16")
    opt = SGD([{"params": list(m.parameters())}], lr=0.01, momentum=0.9, weight_decay=3e-5)
    crit = CrossEntropyLoss(smoothing=0.1)
    m.train()
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    for i in range(2):
        data, target = synthetic_batch(4, 64, seed=0, index=i, device="cuda")
        loss = crit(m(data), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert torch.isfinite(loss)
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert not torch.equal(before["layer3.1.conv2.weight"], dict(m.named_parameters())["layer3.1.conv2.weight"].detach())
    # bf16 logits track the fp32 oracle of the same parameters (training-mode statistics, no drop masks)
    ref.load_state_dict({k: v.detach().cpu().clone().contiguous() for k, v in m.state_dict().items()})
    m.masks = {"dc": [None] * 16, "do": None}
    ref.train()
    data, _ = synthetic_batch(4, 64, seed=0, index=7)
    with torch.no_grad():
        a, b = m(data.cuda()).float().cpu(), ref(data)
    assert ((a - b).norm() / b.norm()).item() < 0.25  # measured 0.11: 53 bf16-rounded activations deep (cf. 0.33 of the baseline net)
    m.eval()  # running statistics, identity drop paths
    with torch.no_grad():
        e = m(data.cuda())
    assert e.shape == (4, 1000) and torch.isfinite(e).all()


def test_static_executor_samples_drop_connect_and_dropout(dev):
    """training through autograd (the Runner's path): the executor draws drop-connect / dropout itself.  Two training forwards of one
    batch differ (the generator position advances), the position is reproducible (set_drop_position), (run seed, rank) selects the
    stream (reseed), rates of 0 give bit-equal logits, and the per-op graph — which draws the same keep_scale vectors from Python —
    lands on the same logits."""
    from sota_imagenet_amd.bresnet import BResNet50, BResNet50Graph
    from sota_imagenet_amd.synth import synthetic_batch

    N, S = 8, 64
    kw = dict(dtype="fp32", drop_rate=0.2, drop_connect_rate=0.2, weight_standardization=False)
    m, g = BResNet50(**kw), BResNet50Graph(**kw)
    g.load_state_dict({k: v.detach().clone().contiguous() for k, v in m.state_dict().items()})
    m, g = m.cuda().train(), g.cuda().train()
    data, _ = synthetic_batch(N, S, seed=0, index=1, device="cuda")
    for mod in (m, g):
        mod.reseed(7, 0)
        mod.set_drop_position(3, 0)
    a0 = m(data).detach().clone()
    assert m._step == (3 << 32) + 1
    a1 = m(data).detach().clone()
    assert m._step == (3 << 32) + 2
    assert not torch.equal(a0, a1), "drop-connect / dropout were not sampled"
    assert ((a0 - a1).norm() / a0.norm()).item() > 1e-2
    g0 = g(data).detach()
    assert nerr(a0, g0) < 1e-4, f"executor vs per-op graph under the same generator position: {nerr(a0, g0):.2e}"
    m.set_drop_position(3, 0)  # same position, same masks (batch statistics do not depend on the running buffers)
    assert torch.equal(m(data).detach(), a0)
    m.reseed(7, 1)  # another rank: another stream
    m.set_drop_position(3, 0)
    assert not torch.equal(m(data).detach(), a0)
    with torch.no_grad():  # train mode without autograd: batch statistics, no drops, the position stays
        before = m._step
        n0, n1 = m(data).clone(), m(data).clone()
    assert torch.equal(n0, n1) and m._step == before
    z = BResNet50(dtype="fp32").cuda().train()
    z0, z1 = z(data).detach().clone(), z(data).detach().clone()
    assert torch.equal(z0, z1)
    s = BResNet50(dtype="fp32", drop_rate=0.2, seed=5)  # an explicit seed stays
    s.reseed(7, 1)
    assert s.seed == 5


def test_runner_positions_the_drop_generator(dev):
    """fit_wrapper.Runner gives the model its (run seed, rank) stream and the (epoch, step) position: epoch 1 of a resumed run does not
    replay the masks of epoch 0"""
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.fit_wrapper import Runner
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.optim import SGD
    from sota_imagenet_amd.data import SyntheticLoader

    m = BResNet50(dtype="bf16", drop_rate=0.2, drop_connect_rate=0.2).cuda()
    opt = SGD([{"params": list(m.parameters())}], lr=0.0, momentum=0.0, weight_decay=0.0)
    r = Runner(m, opt, CrossEntropyLoss(smoothing=0.1))
    r.state.random_seed = 11
    loader = SyntheticLoader(dict(batch_size=4, image_size=64, num_classes=1000), size=8, seed=0, device="cuda", pool=2)
    r.fit(loader, steps_per_epoch=2, epochs=2, start_epoch=1)
    assert m.seed == (11 * 1000003 + 54321) & 0x7FFFFFFF
    assert m._step == (1 << 32) + 2


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("wstd", [True, False])
def test_static_executor_matches_the_per_op_graph(dev, dtype, wstd, monkeypatch):
    """csrc/bresnet_exec.cpp runs the operator sequence of bresnet.BResNet50Graph (one C-ABI call per op from Python) — same kernels,
    same order — from C++.  With the shortcut-gradient add as its own launch (MI355_BRESNET_FUSED_ADD=0; default: in conv1's dgrad
    epilogue) and the ECA / residual tail op by op (MI355_BRESNET_FUSED_ECA=0; default: one fused pass each way) everything up to the
    pooled features is the same arithmetic: running statistics must be BIT-identical.  The FC is
    fc_kernel here and torch's GEMM there, so logits and gradients agree to fp32 GEMM rounding / its bf16 amplification."""
    from sota_imagenet_amd.bresnet import BResNet50, BResNet50Graph
    from sota_imagenet_amd.synth import synthetic_batch

    monkeypatch.setenv("MI355_BRESNET_FUSED_ADD", "0")
    monkeypatch.setenv("MI355_BRESNET_FUSED_ECA", "0")
    monkeypatch.setenv("MI355_BRESNET_STEM_IM2COL", "0")  # (the graph's first conv is the 3x3 over the padded input: the patch form sums in another order)
    N, S = 4, 64
    kw = dict(dtype=dtype, drop_rate=0.2, drop_connect_rate=0.2, weight_standardization=wstd)
    m, g = BResNet50(**kw), BResNet50Graph(**kw)
    g.load_state_dict({k: v.detach().clone().contiguous() for k, v in m.state_dict().items()})
    m, g = m.cuda(), g.cuda()
    data, target = synthetic_batch(N, S, seed=0, index=2, device="cuda")
    masks = _masks(N, 3)
    mk = {"dc": [None if k is None else k.to(dev) for k in masks["dc"]], "do": masks["do"].to(dev)}
    m.masks, g.masks = mk, mk
    m.train(), g.train()
    om, og = m(data), g(data)
    assert nerr(om, og) < 1e-5 if dtype == "fp32" else nerr(om, og) < 1e-4, f"logits {nerr(om, og):.2e}"
    for name in ("conv1.1.running_mean", "bn1.running_var", "layer2.0.downsample.1.running_var", "layer4.2.bn3.running_mean"):
        assert torch.equal(m.state_dict()[name], g.state_dict()[name]), name
    R.smooth_ce(om, target, 0.1).backward()
    R.smooth_ce(og, target, 0.1).backward()
    gm, gg = dict(m.named_parameters()), dict(g.named_parameters())
    rel = lambda a, b: ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-20)).item()
    tot = rel(torch.cat([p.grad.flatten() for p in gm.values()]), torch.cat([gg[k].grad.flatten() for k in gm]))
    assert tot < (1e-4 if dtype == "fp32" else 3e-2), f"all gradients: rel L2 {tot:.2e}"
    for name in ("fc.weight", "fc.bias", "layer4.2.se_module.conv.weight", "layer4.2.conv3.weight", "layer2.0.downsample.0.weight", "layer1.0.bn1.weight",
                 "conv1.0.weight", "conv1.1.weight", "conv1.2.weight", "bn1.bias"):
        r = rel(gm[name].grad, gg[name].grad)
        # bf16: the two heads differ in the last fp32 bits (fc_kernel / torch GEMM), so whether ONE element of the pooled gradient rounds
        # to the neighbouring bf16 value is chance (about two of its 8192 elements sit that close to a rounding boundary), and a single
        # flip at the top grows layer by layer on the way down (measured: 5e-6 at layer4.2 -> 2e-2 at layer1 -> 0.13 at the stem's bias
        # with a flip, exactly 0 everywhere without one; tools/dbg_bres.py).  The bound is the drift bound of the ResNet-50 tests.
        assert r < (1e-3 if dtype == "fp32" else 0.3), f"{name}: {r:.2e}"
    # a second backward into the same flat array accumulates (accumulate_steps > 1)
    g1 = m.flat_grads.clone()
    R.smooth_ce(m(data), target, 0.1).backward()
    assert rel(m.flat_grads, 2 * g1) < (1e-5 if dtype == "fp32" else 2e-2)


def test_static_executor_at_the_baseline_batch(dev, monkeypatch):
    """BASELINE configs[3] at its own size — bs 256, 224 px, bf16: the launch rules pick other tiles / kernels there than at the toy sizes
    of the oracle tests (8-wave tiles, split-K plans, the 112 x 112 stem tensors).  The static executor and the per-op graph must still
    run the same arithmetic: BIT-identical running statistics after a training forward at every depth of the net (the statistics of
    layer 4 have seen every kernel before them), logits equal up to the FC GEMM, a loss near ln 1000, finite gradients that agree."""
    from sota_imagenet_amd.bresnet import BResNet50, BResNet50Graph
    from sota_imagenet_amd.synth import synthetic_batch

    monkeypatch.setenv("MI355_BRESNET_FUSED_ECA", "0")  # (the fused tail skips one bf16 rounding of the gated tensor: not the graph's bits)
    monkeypatch.setenv("MI355_BRESNET_STEM_IM2COL", "0")  # (the first conv as a 1x1 over its patches sums in another order: not the graph's bits either)
    N, S = 256, 224
    kw = dict(dtype="bf16", drop_rate=0.0, drop_connect_rate=0.0, weight_standardization=True)
    m, g = BResNet50(**kw), BResNet50Graph(**kw)
    g.load_state_dict({k: v.detach().clone().contiguous() for k, v in m.state_dict().items()})
    m, g = m.cuda(), g.cuda()
    data, target = synthetic_batch(N, S, seed=0, index=0, device="cuda")
    m.train(), g.train()
    om = m(data)
    lm = R.smooth_ce(om, target, 0.1)
    lm.backward()
    og = g(data)
    lg = R.smooth_ce(og, target, 0.1)
    lg.backward()
    for name in ("conv1.1.running_var", "conv1.3.running_mean", "bn1.running_var", "layer1.0.bn2.running_var", "layer2.0.downsample.1.running_mean",
                 "layer3.5.bn3.running_var", "layer4.0.bn2.running_var", "layer4.2.bn3.running_mean"):
        assert torch.equal(m.state_dict()[name], g.state_dict()[name]), name
    assert nerr(om, og) < 1e-4 and abs(lm.item() - 6.9078) < 0.2 and abs(lm.item() - lg.item()) < 1e-4
    gm, gg = dict(m.named_parameters()), dict(g.named_parameters())
    assert torch.isfinite(m.flat_grads).all()
    for name in ("fc.weight", "layer4.2.conv3.weight", "layer3.0.conv2.weight", "layer1.0.conv1.weight", "conv1.0.weight"):
        a, b = gm[name].grad.float(), gg[name].grad.float()
        assert ((a - b).norm() / b.norm()).item() < 0.1, name  # (fused shortcut add + the FC kernels: bf16 roundings, amplified backwards)
    del g
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bn3_backward_sums_from_the_eca_pass_match_the_reduction_pass(dev, dtype, monkeypatch):
    """default: the BatchNorm-backward sums of bn3 come out of the fused ECA backward's per-image sums (no pass over the tensors:
    sum dz3 = sum_n keep gate a + HW dpool, ...); MI355_BRESNET_ECA_SUMS=0: the reduction pass that forms dz3 on the fly.  Same arithmetic up to
    the summation order (fp32) and the bf16 rounding of dz3 the reduction pass applies before summing."""
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.synth import synthetic_batch

    N, S = 8, 64
    data, target = synthetic_batch(N, S, seed=0, index=3, device="cuda")
    grads = []
    for sw in ("1", "0"):
        monkeypatch.setenv("MI355_BRESNET_ECA_SUMS", sw)
        m = BResNet50(dtype=dtype, drop_rate=0.0, drop_connect_rate=0.2, weight_standardization=True, seed=4).cuda()
        m.train()
        R.smooth_ce(m(data), target, 0.1).backward()
        torch.cuda.synchronize()
        grads.append(m.flat_grads.detach().clone())
        segs = m._segments
    errs = [((grads[0][b:e] - grads[1][b:e]).norm() / grads[1][b:e].norm().clamp_min(1e-30)).item() for b, e in segs]
    assert max(errs) < (1e-4 if dtype == "fp32" else 5e-2), ["%.1e" % x for x in errs]
    assert not torch.equal(grads[0], grads[1]) or dtype == "fp32"


def test_bn1_bn2_backward_sums_from_the_data_gradient_epilogues_match_the_reduction_passes(dev, monkeypatch):
    """default: the backward sums of bn1 / bn2 (and of the deep stem's BatchNorms) ride in the epilogue of the data gradient that produces their
    activation gradient (`*_s3` kernels: the leaky-ReLU mask, tests/test_dconv_gpu.py pins each per op); MI355_BRESNET_FUSE_BN_BWD=0: the reduction
    passes.  Same quantities in another summation order: the first backward segments agree to fp32 rounding, later ones within the amplification
    a re-ordered sum meets in a randomly initialised network (the ResNet-50 counterpart: test_fused_bn_backward_sums_match_standalone_reduce)."""
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.synth import synthetic_batch

    N, S = 8, 224   # (the generated kernels serve the 224 px shapes)
    data, target = synthetic_batch(N, S, seed=0, index=3, device="cuda")
    grads = []
    for sw in ("1", "0"):
        monkeypatch.setenv("MI355_BRESNET_FUSE_BN_BWD", sw)
        m = BResNet50(dtype="bf16", drop_rate=0.0, drop_connect_rate=0.2, weight_standardization=True, seed=4).cuda()
        m.train()
        R.smooth_ce(m(data), target, 0.1).backward()
        torch.cuda.synchronize()
        grads.append(m.flat_grads.detach().clone())
        segs = m._segments
    errs = [((grads[0][b:e] - grads[1][b:e]).norm() / grads[1][b:e].norm().clamp_min(1e-30)).item() for b, e in segs]
    assert errs[0] == 0.0, "the head's gradients depend on no BatchNorm backward"
    assert errs[1] < 1e-3 and max(errs) < 5e-2, ["%.1e" % x for x in errs]   # measured at N = 16: 1.5e-5, 1e-3 ... 1.6e-2 at the stem
    assert not torch.equal(grads[0], grads[1]), "the fused epilogues did not run"


def _bres_backward(env, monkeypatch, data, target, record=False, replay=None, dtype="bf16"):
    """one training forward + backward of a freshly built BResNet-50 executor under the environment `env`; with record: the gradients every block's
    backward started from; with replay: those gradients forced (mi355_bresnet50_grad_hooks).  Returns (flat gradients, segments, recorded)."""
    from sota_imagenet_amd.bresnet import BResNet50

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = BResNet50(dtype=dtype, drop_rate=0.0, drop_connect_rate=0.2, weight_standardization=True, seed=4).cuda()
    m.train()
    loss = R.smooth_ce(m(data), target, 0.1)
    key = (data.shape[0], data.shape[2], data.shape[3])
    rec = None
    if record or replay is not None:
        names = ["layer%d.%d.out" % (li + 1, bi) for li, nb in enumerate((3, 4, 6, 3)) for bi in range(nb)]
        rec = [torch.empty_like(m.debug_tensor(key, n)) for n in names] if record else None
        m.grad_hooks(record=rec, replay=replay)
    loss.backward()
    torch.cuda.synchronize()
    return m.flat_grads.detach().clone(), m._segments, rec


def test_default_backward_teacher_forced_per_segment_against_the_unfused_forms(dev, monkeypatch):
    """the DEFAULT BResNet-50 backward (im2col stem, fused ECA tail with its sums, bn1 / bn2 sums in the data gradients' epilogues, batched
    weight preparation) against the executor with those forms switched off, segment by segment under teacher forcing: run A records the gradient
    every block's backward starts from, run B is fed exactly those (mi355_bresnet50_grad_hooks), so a segment's parameter gradients differ only by that
    segment's own arithmetic — a TIGHT bound per segment instead of the 5e-2 a free-running comparison needs."""
    from sota_imagenet_amd.synth import synthetic_batch

    N, S = 8, 224
    data, target = synthetic_batch(N, S, seed=0, index=5, device="cuda")
    ga, segs, rec = _bres_backward({}, monkeypatch, data, target, record=True)
    off = {"MI355_BRESNET_FUSE_BN_BWD": "0", "MI355_BRESNET_ECA_SUMS": "0", "MI355_BRESNET_BATCH_PREP": "0", "MI355_BRESNET_FUSED_ADD": "0"}
    gb, _, _ = _bres_backward(off, monkeypatch, data, target, replay=rec)
    errs = [((ga[b:e] - gb[b:e]).norm() / gb[b:e].norm().clamp_min(1e-30)).item() for b, e in segs]
    # segment 0 = the head, 1 .. 16 = the blocks (last first), 17 = the stem (fed by block 0's own input gradient: not forced, so it carries one block's difference)
    print("teacher-forced per-segment differences:", ["%.1e" % x for x in errs])
    assert errs[0] == 0.0
    assert max(errs[1:17]) < 4e-3, ["%.1e" % x for x in errs]   # measured 0.8e-3 .. 2.5e-3 (bf16 roundings inside one block); free-running: up to 1.8e-2
    assert errs[17] < 1e-2, errs[17]                             # measured 4.5e-3
    # and forcing is not vacuous: free-running, the same two settings drift apart towards the stem
    gc, _, _ = _bres_backward(off, monkeypatch, data, target)
    free = [((ga[b:e] - gc[b:e]).norm() / gc[b:e].norm().clamp_min(1e-30)).item() for b, e in segs]
    print("free-running:", ["%.1e" % x for x in free])
    assert max(free[8:17]) > 2 * max(errs[8:17]), (free, errs)


def test_static_executor_at_the_baseline_batch_default_fused_tail_against_the_oracle(dev):
    """BASELINE configs[3] at its own size (bs 256, 224 px, bf16) in the DEFAULT environment — the fused ECA x drop-connect x shortcut x
    leaky-ReLU pass with bn3 / the downsample BN applied inside it (MI355_BRESNET_FUSED_ECA, MI355_BRESNET_LAZY_BN at their defaults),
    drop-connect sampled on the device — teacher-forced against the oracle (oracle/bresnet50_ref.py's definitions, oracle/ops_ref.py's
    convolution) on a few images: six convolutions of the kinds the launch rules treat differently there (zero-padded 32-channel stem conv,
    3x3 of layers 1 and 4, conv3 behind the blur pool, the striding block's downsample conv behind its average pool, a long 1x1), each
    re-derived from the executor's own input and the oracle's standardised weights, with whole-batch BN statistics; and the fused tail of a
    striding block and of an identity block re-derived from the executor's conv outputs, statistics, gate inputs and keep scales."""
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.synth import synthetic_batch

    N, S = 256, 224
    key = (N, S, S)
    m = BResNet50(dtype="bf16", drop_rate=0.2, drop_connect_rate=0.2, weight_standardization=True, seed=5).cuda()
    data, target = synthetic_batch(N, S, seed=0, index=0, device="cuda")
    m.train()
    loss = R.smooth_ce(m(data), target, 0.1)
    assert abs(loss.item() - 6.9078) < 0.3
    P = {k: v.detach().float().cpu() for k, v in m.state_dict().items()}
    T = lambda name: m.debug_tensor(key, name)
    img = [0, 100, 255]
    q = lambda t: t.bfloat16().float()
    stats = {}

    def bn_stats(conv, bn):
        y = T(conv + ".y")
        y2 = y.reshape(-1, y.shape[-1]).double()
        mean, invstd = T(bn + ".save_mean"), T(bn + ".save_invstd")
        C = P[bn + ".weight"].numel()
        assert nerr(mean[:C], y2.mean(0).float()[:C]) < 1e-4, bn
        assert nerr(invstd[:C], (y2.var(0, unbiased=False) + 1e-5).rsqrt().float()[:C]) < 1e-4, bn
        stats[bn] = (mean[:C].cpu(), invstd[:C].cpu())
        return y

    # (conv, its BN, the tensor it reads, real input channels)
    for conv, bn, src in [("conv1.2", "conv1.3", "conv1.1.out"), ("layer1.0.conv2", "layer1.0.bn2", "layer1.0.bn1.out"),
                          ("layer2.0.conv3", "layer2.0.bn3", "layer2.0.a2b"), ("layer2.0.downsample.0", "layer2.0.downsample.1", "layer2.0.scin"),
                          ("layer3.2.conv1", "layer3.2.bn1", "layer3.1.out"), ("layer3.2.conv3", "layer3.2.bn3", "layer3.2.bn2.out"),
                          ("layer4.1.conv2", "layer4.1.bn2", "layer4.1.bn1.out")]:
        w = P[conv + ".weight"]
        Co, Ci, K = w.shape[0], w.shape[1], w.shape[2]
        y = bn_stats(conv, bn)[img].float().cpu()
        x = T(src)[img].float().cpu()
        assert x[..., Ci:].abs().max().item() == 0 if x.shape[-1] > Ci else True, src  # (padded channels carry zeros)
        ref = R.conv2d_fwd(x[..., :Ci], q(R.oihw_to_krsc(B.ws(w))), 1, K // 2)
        assert nerr(y[..., :Co], ref) < 2e-2, conv
        if y.shape[-1] > Co:
            assert y[..., Co:].abs().max().item() == 0, conv

    # the first stem convolution (default: a 1x1 convolution over the 27-value patches the input conversion writes) against the oracle's 3x3 / stride-2
    # convolution of the bf16-rounded input
    y0 = bn_stats("conv1.0", "conv1.1")[img].float().cpu()
    x0 = q(data[img].cpu().permute(0, 2, 3, 1))
    assert nerr(y0[..., :32], R.conv2d_fwd(x0, q(R.oihw_to_krsc(B.ws(P["conv1.0.weight"]))), 2, 1)) < 2e-2 and y0[..., 32:].abs().max().item() == 0

    def normalised(y, bn):
        mean, invstd = stats[bn]
        return (y - mean) * invstd * P[bn + ".weight"] + P[bn + ".bias"]

    for blk, prev in (("layer2.0", None), ("layer3.2", "layer3.1")):
        z = normalised(T(blk + ".conv3.y")[img].float().cpu(), blk + ".bn3")        # [n][H][W][C]
        cw = P[blk + ".se_module.conv.weight"].reshape(1, 1, 3)
        gate = torch.sigmoid(torch.nn.functional.conv1d(z.mean((1, 2))[:, None, :], cw, padding=1))[:, 0]
        assert nerr(T(blk + ".gate")[img], gate) < 1e-3, blk
        keep = T(blk + ".keep")[img].cpu()
        assert set(torch.unique(T(blk + ".keep")).cpu().tolist()) <= {0.0, keep.max().item()} and keep.max().item() > 1.0
        sc = T(prev + ".out")[img].float().cpu() if prev else normalised(T(blk + ".downsample.0.y")[img].float().cpu(), blk + ".downsample.1")
        ref = torch.nn.functional.leaky_relu(z * gate[:, None, None, :] * keep[:, None, None, None] + sc, B.LEAKY)
        assert nerr(T(blk + ".out")[img], ref) < 2e-2, blk
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(m.flat_grads).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_epilogue_statistics_feed_the_next_batchnorm(dev, dtype):
    """ops.conv2d_fwd(stats=True) returns (y, partial rows); ops.bn_fwd_train(y, ..., stats=partial) takes the sums the conv
    epilogue left (no reduction pass) and must give what the standalone path gives on the same tensor.  The rows are an
    explicit value: a BatchNorm that is not handed them reduces its own input, whatever ran before."""
    from sota_imagenet_amd import ops

    N, H, W, Cin, Cout = 8, 14, 14, 64, 128
    x = rnd((N, H, W, Cin), 3, dtype).to(dev, dtype)
    w = rnd((Cout, 3, 3, Cin), 4, dtype, 0.05).to(dev, dtype)
    g = (rnd((Cout,), 5, torch.float32) + 1.5).to(dev)
    b = rnd((Cout,), 6, torch.float32).to(dev)
    outs = []
    for stats in (False, True):
        rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
        y, st = ops.conv2d_fwd(x, w, 1, 1, stats=True) if stats else (ops.conv2d_fwd(x, w, 1, 1), None)
        assert (st is not None) == stats and (st is None or (st.dim() == 3 and st.shape[1:] == (2, Cout)))
        out, mean, invstd = ops.bn_fwd_train(y, g, b, rm, rv, relu=True, stats=st)
        outs.append((y, out, mean, invstd, rm, rv))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, c in zip(outs[0][1:], outs[1][1:]):
        assert nerr(c, a) < (1e-5 if dtype == torch.float32 else 1e-2)
    # no hidden hand-off: the SAME storage modified in place after the conv, normalised without the rows, uses its own sums
    y, st = ops.conv2d_fwd(x, w, 1, 1, stats=True)
    y.mul_(2).add_(1)
    rm, rv = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
    _, mean2, _ = ops.bn_fwd_train(y, g, b, rm, rv, relu=False)
    assert nerr(mean2, y.float().reshape(-1, Cout).mean(0)) < 1e-3
    with pytest.raises(ValueError):
        ops.bn_fwd_train(y, g, b, rm, rv, relu=False, stats=st[:, :, : Cout // 2].contiguous())
