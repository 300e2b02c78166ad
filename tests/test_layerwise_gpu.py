"""Native NovogradApex / MyNovograd / AdamLayerwise / MyAdai (csrc/optim_lw.hip, optim._Layerwise) on the MI355X against trajectories recorded
from the reference's own classes (tests/golden/layerwise_ref_trajectories.npz, written by tests/golden/make_layerwise_golden.py on the CPU).

Yardstick, stored in the fixture and never computed from the code under test: after every step and for every tensor, the native parameters may
be no further from the reference's float64 run than FACTOR = 1.5 times the distance of the reference's own float32 run from it, plus a floor of
4 * 2^-24 (two float32 ulps) of the largest parameter magnitude — the rule of this family, stated once in tests/optim_harness.py
(within_yardstick).  At model scale, where no recorded trajectory exists, the same rule is applied with the float32 run of the restated rules
(tests/layerwise_common.py) as the yardstick."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

import optim_harness as H
from layerwise_common import CASES, Fixture, Restated
from optim_harness import U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(fx, dev, grad_scale=1.0, steps=6, separate=False):
    ps, groups, fp, fg, offs = H.fixture_problem(fx, dev, separate=separate)
    opt = H.make_opt(fx, groups, fx.lrs[0])
    opt.grad_scale = grad_scale
    traj = []
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = fx.lrs[k]
        H.set_grads(ps, fx.split(fx.grads[k]), 1.0 / grad_scale)  # (exact: a power of two)
        opt.step()
        traj.append(H.gather(ps).clone())
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
        gaps = H.gaps(ps, fp)
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
    ps, fp, fg, offs = H.flat_params(sizes, [(s,) for s in sizes], vals, dev)
    H.set_grads(ps, grads)
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
    gaps = H.gaps(ps, fp)
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


KINDS = {
    "nov": ("NovogradApex", dict(betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01), 1e-2),
    "mynov": ("MyNovograd", dict(betas=(0.9, 0.99), weight_decay=0.002), 1e-2),
    "adamlw": ("AdamLayerwise", dict(betas=(0.9, 0.995), weight_decay=2e-2), 1e-3),
    "myadai": ("MyAdai", dict(betas=(0.1, 0.99), weight_decay=3e-5, sgd_mom=True, stable_wd=True), 1e-2),
}


def _model_opt(kind, groups_of=None):
    return H.model_opt(*KINDS[kind], groups_of)


STAGES = ["lw_sumsq", "lw_coef", "lw_update"]


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
    calls = H.count_launches(monkeypatch, STAGES)
    H.flat_steps(m, opt, [31], lr)
    assert calls == ["lw_sumsq", "lw_coef", "lw_update"]
    mask = H.padding_mask(m)
    assert mask.any() and (m.flat_params[mask] == 0).all() and torch.isnan(m.flat_grads[mask]).all() and torch.isfinite(m.flat_params).all()
    grads = [p.grad.detach().cpu().clone() for p in params]
    wd = kw["weight_decay"]
    r64 = Restated(cls, kw, p0, [0] * 161, [wd], torch.float64)
    r32 = Restated(cls, kw, p0, [0] * 161, [wd], torch.float32)
    r64.step(grads, [lr])
    r32.step(grads, [lr])
    worst, moved = 0.0, 0
    for i, p in enumerate(params):
        yard = (r32.p[i].double() - r64.p[i]).abs().max().item()
        worst = max(worst, H.within_yardstick(p, r64.p[i], yard, f"{kind} tensor {i} {tuple(p.shape)}", floor_in_ratio=True, yard_name="restated fp32"))
        moved += int((p.detach().cpu() != p0[i]).any())
    print(f"{kind}: worst native error / max(restated-fp32 error, floor) over 161 tensors {worst:.2f}")
    assert moved == 161
    # the recipe's two groups
    sys.path.insert(0, ROOT)
    import train

    m2, opt2 = _model_opt(kind, lambda mm: train.filter_from_weight_decay(mm, ["bn", "bias"]))
    del calls[:]
    H.flat_steps(m2, opt2, [32], lr)
    assert calls == ["lw_sumsq", "lw_coef", "lw_coef", "lw_update", "lw_update"]
    assert (m2.flat_params[H.padding_mask(m2)] == 0).all() and torch.isfinite(m2.flat_params).all()
    assert all(opt2.state[p]["step"] == 1 for p in m2.parameters())


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_model_ema_inside_the_step_kernel_matches_the_callback(dev, kind):
    """ModelEma (train.py:111-112) under the layer-wise optimizers: the average advanced by the update kernel (attach_ema) equals the
    callback's own lerp after every batch, and the parameters are the same bits either way"""
    H.ema_matches_callback(lambda: _model_opt(kind), KINDS[kind][2] * 0.1)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_resume_continues_bitwise(dev, kind):
    """train.py:140-146 resume: two steps, state_dict into a new optimizer, two more = four uninterrupted steps bit for bit (the float32
    second-moment slot and the step counts travel in the state; MyAdai's float travels as a float)"""
    cls, kw, lr = KINDS[kind]
    m, opt = _model_opt(kind)
    H.flat_steps(m, opt, [1, 2], lr)
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
    H.flat_steps(m, opt, [3, 4], lr)
    want = m.flat_params.clone()
    m2, opt2 = _model_opt(kind)
    m2.load_state_dict(ck["state_dict"])
    opt2.load_state_dict(ck["optimizer"])
    H.flat_steps(m2, opt2, [3, 4], lr)
    assert torch.equal(m2.flat_params, want)
    assert all(opt2.state[p]["step"] == 4 for p in m2.parameters())
    m3, opt3 = _model_opt(kind)  # without the optimizer state the steps differ
    m3.load_state_dict(ck["state_dict"])
    H.flat_steps(m3, opt3, [3, 4], lr)
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
    ps2, groups2, fp2, fg2, _ = H.fixture_problem(fx, dev, p_flat0=fx.p64[4].float())
    opt2 = H.make_opt(fx, groups2, fx.lrs[5])
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
    H.set_grads(ps2, fx.split(fx.grads[5]))
    opt2.step()
    torch.cuda.synchronize()
    fx.check(5, H.gather(ps2), f"{case} step 6 from the reference's state")
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
    from sota_imagenet_amd import optim

    cls = getattr(optim, cls_name)
    made = []
    build = cls._build_plans

    def spy(self):
        made.append(self)
        return build(self)

    monkeypatch.setattr(cls, "_build_plans", spy)
    _, _, run, losses = H.run_smoke_config(name, tmp_path, ["run.fp16=false", "random_seed=0", "data.pool=2", "log.save_optim=true"],
                                           resume_eval=True)
    assert made and all(type(o) is cls for o in made)
    print(name, "train losses:", losses)
    assert losses and all(math.isfinite(x) for x in losses)
    ck = torch.load(os.path.join(run, "model.chpn"), map_location="cpu")
    per_param = list(ck["optimizer"]["state"].values())
    assert len(per_param) == 161 and all(set(s) == keys and s["step"] > 0 for s in per_param)
