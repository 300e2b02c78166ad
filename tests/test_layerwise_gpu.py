"""Native NovogradApex / MyNovograd / AdamLayerwise / MyAdai (csrc/optim_lw.hip, optim._Layerwise) on the MI355X against trajectories recorded
from the reference's own classes (tests/golden/layerwise_ref_trajectories.npz, written by tests/golden/make_layerwise_golden.py on the CPU).

Yardstick, stored in the fixture and never computed from the code under test: after every step and for every tensor, the native parameters may
be no further from the reference's float64 run than FACTOR = 1.5 times the distance of the reference's own float32 run from it, plus a floor of
4 * 2^-24 (two float32 ulps) of the largest parameter magnitude — the rule of test_madgrad_adais_gpu.py.  At model scale, where no recorded
trajectory exists, the same rule is applied with the float32 run of the restated rules (tests/layerwise_common.py) as the yardstick."""
import copy
import glob
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

from layerwise_common import CASES, FACTOR, U, Fixture, Restated
from plan_common import layout as _layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _flat_params(sizes, shapes, values, dev, order=None, separate=False):
    """parameters as views of one flat parameter / gradient buffer (zero gaps in p, NaN in every gap of g), or each in its own allocation"""
    offs, n = _layout(sizes, order)
    fp, fg = torch.zeros(n, device=dev), torch.full((n,), NAN, device=dev)
    ps = []
    for i, (o, s, shape) in enumerate(zip(offs, sizes, shapes)):
        if separate:
            p = torch.nn.Parameter(values[i].to(dev).clone().view(shape))
            p.grad = torch.zeros(s, device=dev).view(shape)
        else:
            fp[o:o + s] = values[i].to(dev)
            p = torch.nn.Parameter(fp[o:o + s].view(shape))
            p.grad = fg[o:o + s].view(shape)
        ps.append(p)
    return ps, fp, fg, offs


def _fixture_problem(fx, dev, p_flat0=None, separate=False):
    order = [i for idx in fx.groups for i in idx]
    ps, fp, fg, offs = _flat_params(fx.sizes, fx.shapes, fx.split(fx.p0 if p_flat0 is None else p_flat0), dev, order, separate)
    groups = [{"params": [ps[i] for i in fx.groups[0]]}, {"params": [ps[i] for i in fx.groups[1]], "weight_decay": 0}]
    return ps, groups, fp, fg, offs


def _make(fx, groups, lr):
    from sota_imagenet_amd import optim

    return getattr(optim, fx.cls)(groups, lr=lr, **fx.hyper)


def _set_grads(ps, grads, mult=1.0):
    for p, g in zip(ps, grads):
        p.grad.copy_((g * mult).view(p.shape))


def _gather(ps):
    return torch.cat([p.detach().reshape(-1) for p in ps])


def _gaps(ps, fp):
    mask = torch.ones_like(fp, dtype=torch.bool)
    for p in ps:
        o = (p.data_ptr() - fp.data_ptr()) // 4
        mask[o:o + p.numel()] = False
    return mask


def _run(fx, dev, grad_scale=1.0, steps=6, separate=False):
    ps, groups, fp, fg, offs = _fixture_problem(fx, dev, separate=separate)
    opt = _make(fx, groups, fx.lrs[0])
    opt.grad_scale = grad_scale
    traj = []
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = fx.lrs[k]
        _set_grads(ps, fx.split(fx.grads[k]), 1.0 / grad_scale)  # (exact: a power of two)
        opt.step()
        traj.append(_gather(ps).clone())
    torch.cuda.synchronize()
    return traj, opt, ps, fp, fg


@pytest.mark.parametrize("case", CASES)
def test_steps_follow_the_reference_trajectory(dev, case):
    """six steps on the fixture's inputs, gradients and lr ramp, every step and tensor against the stored yardstick; the same again with
    grad_scale = 0.5 on doubled gradients (figures: DESIGN.md section 11).  The gaps of the flat buffers are never touched: zero in p,
    NaN in g."""
    fx = Fixture(case)
    worst = 0.0
    for gs in (1.0, 0.5):
        traj, opt, ps, fp, fg = _run(fx, dev, grad_scale=gs)
        for k, got in enumerate(traj):
            worst = max(worst, fx.check(k, got, f"{case} grad_scale={gs}"))
        gaps = _gaps(ps, fp)
        assert gaps.any() and (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all() and torch.isfinite(fp).all()
        assert all(opt.state[p]["step"] == 6 and type(opt.state[p]["step"]) is int for p in ps)
    print(f"{case}: worst native / reference-fp32 error ratio {worst:.2f}")
    assert (traj[-1].cpu() - fx.p0).abs().max().item() > 1e-3
    if fx.cls == "MyAdai":  # the momentum coefficient of the last step, per tensor, against the recorded one
        order = [i for idx in fx.groups for i in idx]
        got = opt._coef[:, 1].double().cpu().numpy()
        assert np.abs(got - fx.beta1[5][order]).max() <= 4 * U


@pytest.mark.parametrize("source", ["gradient", "parameter"])
def test_per_tensor_sums_equal_the_float64_sums(dev, source):
    """tensors of 1, 5, 63, 64, 65, W-1, W, W+1 and 3W+5 elements (one item with a scalar tail only, whole items, an item boundary inside a
    tensor) in one 64-aligned flat buffer with NaN in every gap of the gradient buffer: the statistic of stage (b), per tensor, equals
    the float64 sum of squares on the CPU to 1e-12 relative, for the gradient (AdamLayerwise, grad_scale 0.5) and the parameter (MyNovograd)"""
    from sota_imagenet_amd import ops, optim

    W = ops.lw_item_elems()
    sizes = [1, 5, 63, 64, 65, W - 1, W, W + 1, 3 * W + 5]
    gen = torch.Generator().manual_seed(11)
    vals = [torch.randn(s, generator=gen) * (10.0 ** (i % 3 - 1)) for i, s in enumerate(sizes)]
    grads = [torch.randn(s, generator=gen) * (10.0 ** ((i + 1) % 3 - 2)) for i, s in enumerate(sizes)]
    ps, fp, fg, offs = _flat_params(sizes, [(s,) for s in sizes], vals, dev)
    _set_grads(ps, grads)
    if source == "gradient":
        opt, scale, src = optim.AdamLayerwise(ps, lr=1e-3, betas=(0.9, 0.99)), 0.5, grads
    else:
        opt, scale, src = optim.MyNovograd(ps, lr=1e-3), 1.0, vals
    opt.grad_scale = 0.5
    opt.step()
    torch.cuda.synchronize()
    got = opt._sums.cpu()
    want = torch.stack([(t * scale).double().pow(2).sum() for t in src])
    rel = ((got - want).abs() / want).max().item()
    print(f"{source}: per-tensor sums, worst relative error {rel:.3e}; items {opt._items.shape[0]}")
    assert rel <= 1e-12
    assert opt._items.shape[0] == sum(-(-s // W) for s in sizes) == opt._partial.numel()
    for t in (opt._sums, opt._partial, opt._coef, opt._v, fp, *[opt.state[p][opt._m_key] for p in ps]):
        assert torch.isfinite(t).all()
    gaps = _gaps(ps, fp)
    assert (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all()
    assert all((p.detach().cpu().reshape(-1) != v).any() for p, v in zip(ps[2:], vals[2:]))  # every tensor was updated


@pytest.mark.parametrize("case", ["nov_recipe", "mynov_recipe", "adamlw_alt", "myadai_recipe"])
def test_placement_and_replay_are_bitwise(dev, case):
    """the same tensors in separately allocated storages (one stage-(a) and one stage-(c) launch per storage pair) give the parameters of
    the flat-buffer run bit for bit, and a second flat-buffer run from the same state repeats them bit for bit"""
    fx = Fixture(case)
    flat_a, opt_a, *_ = _run(fx, dev, steps=3)
    flat_b, *_ = _run(fx, dev, steps=3)
    sep, opt_s, *_ = _run(fx, dev, steps=3, separate=True)
    assert len(opt_a._segs) == 1 and len(opt_s._segs) == 5
    for k in range(3):
        assert torch.equal(flat_a[k], flat_b[k]) and torch.equal(flat_a[k], sep[k])


def _grads_for(m, seed, scale=1e-2):
    """one flat gradient for every parameter of a flat model, NaN in the padding"""
    g = torch.full_like(m.flat_grads, NAN)
    for i, (name, p) in enumerate(m.named_parameters()):
        off = (p.data_ptr() - m.flat_params.data_ptr()) // 4
        gen = torch.Generator().manual_seed(seed * 1000 + i)
        g[off: off + p.numel()] = (torch.randn((p.numel(),), generator=gen) * scale).to(g.device)
    return g


def _flat_steps(m, opt, seeds, lr):
    for s in seeds:
        m.flat_grads.copy_(_grads_for(m, s))
        for g in opt.param_groups:
            g["lr"] = lr
        opt.zero_grad()
        opt.step()
    torch.cuda.synchronize()


KINDS = {
    "nov": ("NovogradApex", dict(betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01), 1e-2),
    "mynov": ("MyNovograd", dict(betas=(0.9, 0.99), weight_decay=0.002), 1e-2),
    "adamlw": ("AdamLayerwise", dict(betas=(0.9, 0.995), weight_decay=2e-2), 1e-3),
    "myadai": ("MyAdai", dict(betas=(0.1, 0.99), weight_decay=3e-5, sgd_mom=True, stable_wd=True), 1e-2),
}


def _model_opt(kind, groups_of=None):
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.models import resnet50

    cls, kw, lr = KINDS[kind]
    m = resnet50(dtype="fp32").cuda()
    groups = groups_of(m) if groups_of else [{"params": list(m.parameters())}]
    opt = getattr(optim, cls)(groups, lr=lr, **kw)
    opt.attach_model(m)
    return m, opt


def _padding_mask(m):
    mask = torch.ones(m.flat_params.numel(), dtype=torch.bool, device=m.flat_params.device)
    for p in m.parameters():
        off = (p.data_ptr() - m.flat_params.data_ptr()) // 4
        mask[off: off + p.numel()] = False
    return mask


def _count_launches(monkeypatch):
    from sota_imagenet_amd import ops

    calls = []
    for name in ("lw_sumsq", "lw_coef", "lw_update"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(fn, name))
    return calls


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_step_at_model_scale(dev, monkeypatch, kind):
    """one step on a real resnet50 flat array (161 tensors, alignment gaps, FC padding; NaN in the gradient's padding) against the float64
    restatement on the CPU, tensor by tensor, with the restatement's own float32 run as the yardstick; 3 launches, 1 + 2 + 2 with
    filter_from_wd; the parameter padding stays zero"""
    cls, kw, lr = KINDS[kind]
    m, opt = _model_opt(kind)
    params = list(m.parameters())
    assert len(params) == 161
    p0 = [p.detach().cpu().clone() for p in params]
    calls = _count_launches(monkeypatch)
    _flat_steps(m, opt, [31], lr)
    assert calls == ["lw_sumsq", "lw_coef", "lw_update"]
    mask = _padding_mask(m)
    assert mask.any() and (m.flat_params[mask] == 0).all() and torch.isnan(m.flat_grads[mask]).all() and torch.isfinite(m.flat_params).all()
    grads = [p.grad.detach().cpu().clone() for p in params]
    wd = kw["weight_decay"]
    r64 = Restated(cls, kw, p0, [0] * 161, [wd], torch.float64)
    r32 = Restated(cls, kw, p0, [0] * 161, [wd], torch.float32)
    r64.step(grads, [lr])
    r32.step(grads, [lr])
    worst, moved = 0.0, 0
    for i, p in enumerate(params):
        ref = r64.p[i]
        err = (p.detach().cpu().double() - ref).abs().max().item()
        yard = (r32.p[i].double() - ref).abs().max().item()
        floor = 4 * U * ref.abs().max().item()
        worst = max(worst, err / max(yard, floor))
        moved += int((p.detach().cpu() != p0[i]).any())
        assert err <= FACTOR * yard + floor, f"{kind} tensor {i} {tuple(p.shape)}: native {err:.3e} vs restated fp32 {yard:.3e} (floor {floor:.2e})"
    print(f"{kind}: worst native error / max(restated-fp32 error, floor) over 161 tensors {worst:.2f}")
    assert moved == 161
    # the recipe's two groups
    sys.path.insert(0, ROOT)
    import train

    m2, opt2 = _model_opt(kind, lambda mm: train.filter_from_weight_decay(mm, ["bn", "bias"]))
    del calls[:]
    _flat_steps(m2, opt2, [32], lr)
    assert calls == ["lw_sumsq", "lw_coef", "lw_coef", "lw_update", "lw_update"]
    assert (m2.flat_params[_padding_mask(m2)] == 0).all() and torch.isfinite(m2.flat_params).all()
    assert all(opt2.state[p]["step"] == 1 for p in m2.parameters())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_model_ema_inside_the_step_kernel_matches_the_callback(dev, kind):
    """ModelEma (train.py:111-112) under the layer-wise optimizers: the average advanced by the update kernel (attach_ema) equals the
    callback's own lerp after every batch, and the parameters are the same bits either way"""
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.synth import synthetic_batch

    class Loader:
        batch_size = 4

        def __len__(self):
            return 3

        def __iter__(self):
            return iter([synthetic_batch(4, 64, seed=6, index=i, device="cuda") for i in range(3)])

    res = []
    lr = KINDS[kind][2] * 0.1
    for fused in (True, False):
        m, opt = _model_opt(kind)
        ema = fw.ModelEma(m, 0.9)
        if not fused:
            ema.on_begin = lambda: None
        runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[fw.PhasesScheduler([dict(ep=(0, 1), lr=(lr, 2 * lr))]), ema])
        runner.fit(Loader(), val_loader=Loader(), epochs=1)
        assert ema._fused == fused and not ema._swapped
        res.append((m.flat_params.clone(), ema.ema[0].clone(), ema.ema[1].clone()))
    (p_a, e_a, b_a), (p_b, e_b, b_b) = res
    assert torch.equal(p_a, p_b) and torch.equal(b_a, b_b)
    assert not torch.equal(e_a, p_a) and torch.isfinite(e_a).all()
    assert ((e_a - e_b).abs().max() / e_b.abs().max()).item() < 1e-6


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_resume_continues_bitwise(dev, kind):
    """train.py:140-146 resume: two steps, state_dict into a new optimizer, two more = four uninterrupted steps bit for bit (the float32
    second-moment slot and the step counts travel in the state; MyAdai's float travels as a float)"""
    cls, kw, lr = KINDS[kind]
    m, opt = _model_opt(kind)
    _flat_steps(m, opt, [1, 2], lr)
    ck = {"state_dict": copy.deepcopy(m.state_dict()), "optimizer": copy.deepcopy(opt.state_dict())}
    st0 = ck["optimizer"]["state"][0]
    p_first = next(iter(m.parameters()))
    if cls == "MyAdai":
        assert set(st0) == {"step", "exp_avg", "exp_avg_sq"} and type(st0["exp_avg_sq"]) is float
    else:
        assert set(st0) == {"step", opt._m_key, opt._v_key}
        v = st0[opt._v_key]
        assert v.shape == p_first.shape and v.is_contiguous() and (v == v.reshape(-1)[0]).all()  # dense, as the reference keeps it
        assert opt.state[p_first][opt._v_key].stride() == (0,) * p_first.dim()                   # one slot on the device
    assert st0["step"] == 2
    _flat_steps(m, opt, [3, 4], lr)
    want = m.flat_params.clone()
    m2, opt2 = _model_opt(kind)
    m2.load_state_dict(ck["state_dict"])
    opt2.load_state_dict(ck["optimizer"])
    _flat_steps(m2, opt2, [3, 4], lr)
    assert torch.equal(m2.flat_params, want)
    assert all(opt2.state[p]["step"] == 4 for p in m2.parameters())
    m3, opt3 = _model_opt(kind)  # without the optimizer state the steps differ
    m3.load_state_dict(ck["state_dict"])
    _flat_steps(m3, opt3, [3, 4], lr)
    assert not torch.equal(m3.flat_params, want)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_has_the_references_layout_and_loads_its_state(dev, case):
    """our state_dict() carries exactly the key set and tensor shapes the reference's did (recorded in the fixture); the reference's
    float64 state after five steps (dense second moment) loads, and the sixth step lands on the reference's sixth step; a second moment
    that does not hold one value is refused at load"""
    fx = Fixture(case)
    _, opt, ps, _, _ = _run(fx, dev)
    sd = opt.state_dict()
    order = [i for idx in fx.groups for i in idx]  # state_dict index -> fixture tensor
    assert sorted(sd["state"]) == list(range(len(order)))
    for j, i in enumerate(order):
        st = sd["state"][j]
        assert sorted(st) == fx.state_keys and st["step"] == 6
        for key, shapes in fx.state_shapes.items():
            assert list(st[key].shape) == shapes[i] and st[key].dtype == torch.float32 and st[key].is_contiguous()
    ps2, groups2, fp2, fg2, _ = _fixture_problem(fx, dev, p_flat0=fx.p64[4].float())
    opt2 = _make(fx, groups2, fx.lrs[5])
    state = {}
    for j, i in enumerate(order):
        state[j] = {key: fx.split(t)[i].view(fx.shapes[i]).clone() for key, t in fx.state5.items()}
        state[j]["step"] = 5
        if fx.cls == "MyAdai":
            state[j]["exp_avg_sq"] = float(fx.v0[i])
    pg = copy.deepcopy(opt2.state_dict()["param_groups"])
    opt2.load_state_dict({"state": copy.deepcopy(state), "param_groups": pg})
    for g in opt2.param_groups:
        g["lr"] = fx.lrs[5]
    _set_grads(ps2, fx.split(fx.grads[5]))
    opt2.step()
    torch.cuda.synchronize()
    fx.check(5, _gather(ps2), f"{case} step 6 from the reference's state")
    assert all(opt2.state[p]["step"] == 6 for p in ps2)
    if fx.cls != "MyAdai":
        key = opt2._v_key
        state[0][key].view(-1)[-1] *= 2
        with pytest.raises(ValueError, match="one value"):
            opt2.load_state_dict({"state": state, "param_groups": pg})


SMOKE = [("nov_test", "NovogradApex", {"step", "exp_avg", "exp_avg_sq"}), ("my-nov_test", "MyNovograd", {"step", "ema_grad", "ema_norm"}),
         ("nov-adam_test", "AdamLayerwise", {"step", "exp_avg", "exp_avg_sq"}), ("adai_2_test", "MyAdai", {"step", "exp_avg", "exp_avg_sq"})]


@pytest.mark.parametrize("name,cls_name,keys", SMOKE)
def test_train_py_runs_the_smoke_config(dev, tmp_path, monkeypatch, name, cls_name, keys):
    """train.py on the four smoke configs: the native class is built and planned, the losses are finite, the checkpoint carries the
    reference's state layout and evaluates after a resume"""
    sys.path.insert(0, ROOT)
    import train

    from sota_imagenet_amd import optim

    cls = getattr(optim, cls_name)
    made = []
    build = cls._build_plans

    def spy(self):
        made.append(self)
        return build(self)

    monkeypatch.setattr(cls, "_build_plans", spy)
    logdir = os.path.relpath(str(tmp_path), ROOT)
    val_loss, metrics = train.main([f"+hydra_exp={name}", f"log.dir={logdir}", "run.fp16=false", "random_seed=0", "data.pool=2",
                                    "log.save_optim=true"])
    assert made and all(type(o) is cls for o in made)
    assert math.isfinite(val_loss) and 0.0 <= metrics["Acc@1"].avg <= 100.0
    run = glob.glob(os.path.join(str(tmp_path), f"*_{name}", "*"))[0]
    logs = open(os.path.join(run, "logs.txt")).read()
    losses = [float(x) for x in re.findall(r"Train loss: ([0-9.]+)", logs)]
    print(name, "train losses:", losses)
    assert losses and all(math.isfinite(x) for x in losses)
    ck = torch.load(os.path.join(run, "model.chpn"), map_location="cpu")
    per_param = list(ck["optimizer"]["state"].values())
    assert len(per_param) == 161 and all(set(s) == keys and s["step"] > 0 for s in per_param)
    loss2, m2 = train.main([f"+hydra_exp={name}", f"log.dir={logdir}", f"run.resume={os.path.join(run, 'model.chpn')}", "run.evaluate=true",
                            "data.pool=2"])
    assert math.isfinite(loss2) and 0.0 <= m2["Acc@1"].avg <= 100.0
