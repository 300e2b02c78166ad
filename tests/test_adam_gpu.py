"""Native Adam / AdamW (csrc/optim.hip, optim.Adam / optim.AdamW) on the MI355X against torch's own optimizers on the CPU.

Yardstick: the native result may be no further from a float64 run of torch.optim.Adam / AdamW(foreach=False) than twice the
distance of the same torch optimizer in float32 on the CPU (one intra-op thread), plus a floor of 1e-7 * lr for the parameters
and one fp32 rounding of the largest value per step for the moments — the form of test_resnet_gpu's fp32 gradient yardstick."""
import copy
import functools
import math
import os
import sys

import pytest
import torch

import optim_harness as H
from optim_harness import U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_grads_for = functools.partial(H.grads_for, pad=0.0)  # zero in the padding: what a backward leaves there
_flat_steps = functools.partial(H.flat_steps, lr=1e-3, pad=0.0)


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def maxerr(a, ref):
    return (a.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item()


def torch_cls(decoupled):
    return torch.optim.AdamW if decoupled else torch.optim.Adam


def torch_run(p0s, grads, lrs, dtype, decoupled, groups_wd, eps, betas=(0.9, 0.999)):
    """torch's single-tensor optimizer on the CPU: p0s = list of initial tensors (one group per entry of groups_wd, a list of
    index lists), grads[k] = list of per-tensor gradients of step k.  Returns (params, optimizer)."""
    ps = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in p0s]
    opt = torch_cls(decoupled)([{"params": [ps[i] for i in idx], "weight_decay": wd} for idx, wd in groups_wd], lr=lrs[0],
                               betas=betas, eps=eps, foreach=False)
    for k, gs in enumerate(grads):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        for p, g in zip(ps, gs):
            p.grad = g.to(dtype).clone()
        opt.step()
    return ps, opt


@pytest.mark.parametrize("decoupled", [True, False])
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_adam_step_matches_torch(dev, decoupled, eps, grad_scale):
    """ops.adam_step over n = 100 003 (the f32x4 loop + the scalar tail), five steps with a different lr each"""
    from sota_imagenet_amd import ops

    n, wd, betas = 100003, 5e-2, (0.9, 0.999)
    lrs = [1e-3, 3e-3, 5e-4, 2e-3, 1e-3]
    p0 = rnd((n,), 81)
    grads = [rnd((n,), 82 + k, 10.0 ** (k % 3 - 1)) for k in range(5)]
    scaled = [[g * grad_scale] for g in grads]  # what the native kernel sees after its grad_scale multiply (exact: powers of 2)
    (r64,), o64 = torch_run([p0], scaled, lrs, torch.float64, decoupled, [([0], wd)], eps, betas)
    (r32,), o32 = torch_run([p0], scaled, lrs, torch.float32, decoupled, [([0], wd)], eps, betas)
    p = p0.to(dev).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k, g in enumerate(grads):
        ops.adam_step(p, g.to(dev), m, v, k, lrs[k], betas, eps, wd, decoupled=decoupled, grad_scale=grad_scale)
    torch.cuda.synchronize()
    s64, s32 = o64.state[r64], o32.state[r32]
    got, yard = maxerr(p, r64), maxerr(r32, r64)
    assert got <= 2 * yard + 1e-7 * min(lrs), f"p: native {got:.3e} vs torch fp32 {yard:.3e}"
    for name, t in (("exp_avg", m), ("exp_avg_sq", v)):
        ref = s64[name]
        got, yard = maxerr(t, ref), maxerr(s32[name], ref)
        assert got <= 2 * yard + 5 * U * ref.abs().max().item(), f"{name}: native {got:.3e} vs torch fp32 {yard:.3e}"
    # the step really moved p by ~lr per step (not a no-op that the yardstick would also accept)
    assert maxerr(p, p0) > 1e-3


def test_adam_step_with_the_moving_average_in_the_same_pass(dev):
    """mi355_adam_step_ema: p, m, v bit for bit as the plain step, the average = ModelEma's lerp after each step"""
    from sota_imagenet_amd import ops

    n = 100003
    p0 = rnd((n,), 91).to(dev)
    grads = [rnd((n,), 92 + k).to(dev) for k in range(3)]
    for decoupled in (True, False):
        p, pe = p0.clone(), p0.clone()
        m, v, me, ve = (torch.zeros_like(p0) for _ in range(4))
        ema, ema_ref = p0.clone(), p0.clone()
        for k, g in enumerate(grads):
            ops.adam_step(p, g, m, v, k, 1e-3, eps=1e-8, weight_decay=5e-2, decoupled=decoupled)
            ema_ref.lerp_(p, 1.0 - 0.99)
            ops.adam_step(pe, g, me, ve, k, 1e-3, eps=1e-8, weight_decay=5e-2, decoupled=decoupled, ema=ema, ema_decay=0.99)
        assert torch.equal(p, pe) and torch.equal(m, me) and torch.equal(v, ve)
        assert ((ema - ema_ref).abs().max() / ema_ref.abs().max()).item() < 1e-6 and not torch.equal(ema, pe)


def _sgd_plan_ranges(m, groups):
    from sota_imagenet_amd.optim import SGD

    s = SGD(groups, lr=0.0)
    s.attach_model(m)
    return [[(r[2], r[3]) for r in s._merged_ranges() if r[5] == gi] for gi in range(len(groups))]


def test_adamw_model_level_teacher_forced(dev):
    """resnet50 fp32, the recipe's two param groups (train.filter_from_weight_decay), one frozen parameter: the same flat gradients
    into native AdamW and into torch's AdamW on the CPU (fp64 / fp32) for three steps"""
    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.optim import AdamW

    sys.path.insert(0, ROOT)
    import train

    m = resnet50(dtype="fp32").cuda()
    named = dict(m.named_parameters())
    frozen = named["layer3.2.bn2.weight"]
    frozen.requires_grad_(False)
    frozen_before = frozen.detach().clone()
    groups = train.filter_from_weight_decay(m, ["bn", "bias"])
    names = {id(p): n for n, p in named.items()}
    order = [p for g in groups for p in g["params"]]
    p0s = [p.detach().cpu().clone() for p in order]
    wd, lrs = 5e-2, [1e-3, 2e-3, 1.5e-3]
    opt = AdamW(groups, lr=lrs[0], weight_decay=wd)
    opt.attach_model(m)
    flat_grads = [_grads_for(m, 40 + k) for k in range(3)]
    for k in range(3):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        m.flat_grads.copy_(flat_grads[k])
        opt.zero_grad()
        opt.step()
    torch.cuda.synchronize()

    def per_param(flat):
        return [torch.as_strided(flat, p.shape, p.stride(), (p.data_ptr() - m.flat_params.data_ptr()) // 4).cpu() for p in order]

    grads = [per_param(fg) for fg in flat_grads]
    n0 = len(groups[0]["params"])
    gw = [(list(range(n0)), wd), (list(range(n0, len(order))), 0.0)]
    r64, o64 = torch_run(p0s, grads, lrs, torch.float64, True, gw, 1e-8)
    r32, o32 = torch_run(p0s, grads, lrs, torch.float32, True, gw, 1e-8)
    for p, a, b in zip(order, r64, r32):
        got, yard = maxerr(p, a), maxerr(b, a)
        floor = 1e-7 * min(lrs) + 3 * U * a.abs().max().item()
        assert got <= 2 * yard + floor, f"{names[id(p)]}: native {got:.3e} vs torch fp32 {yard:.3e}"
        st, s64 = opt.state[p], o64.state[a]
        assert int(st["step"].item()) == 3 and st["step"].dtype == torch.float32 and st["step"].device.type == "cpu"
        for key in ("exp_avg", "exp_avg_sq"):
            assert maxerr(st[key], s64[key]) <= 2 * maxerr(o32.state[b][key], s64[key]) + 5 * U * s64[key].abs().max().item()
    # the wd-0 group gets no decay: bn1.weight moves by the Adam update alone (the decayed run lands far from it)
    i = next(k for k, q in enumerate(order) if q is named["bn1.weight"])
    decayed = torch_run([p0s[i]], [[g[i]] for g in grads], lrs, torch.float64, True, [([0], wd)], 1e-8)[0][0]
    assert maxerr(decayed, r64[i]) > 10 * maxerr(order[i], r64[i])
    assert torch.equal(frozen.detach(), frozen_before)
    # launches = the ranges of SGD's planner on the same groups (the two groups interleave in the flat array, the frozen
    # tensor is a barrier); a single group over the whole model is ONE launch
    assert [len(segs) for segs in opt._plans] == [len(r) for r in _sgd_plan_ranges(m, groups)]
    m2 = resnet50(dtype="fp32").cuda()
    o2 = AdamW(m2.parameters(), lr=1e-3)
    o2.attach_model(m2)
    o2.step()
    assert [len(segs) for segs in o2._plans] == [1]


def test_adamw_resume_continues_bitwise(dev):
    """train.py:140-146 resume under AdamW: after load_state_dict the next step equals the uninterrupted run bit for bit"""
    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.optim import AdamW

    def make():
        m = resnet50(dtype="fp32").cuda()
        opt = AdamW(m.parameters(), lr=1e-3, weight_decay=5e-2)
        opt.attach_model(m)
        return m, opt

    m, opt = make()
    _flat_steps(m, opt, [1, 2])
    ck = {"state_dict": copy.deepcopy(m.state_dict()), "optimizer": copy.deepcopy(opt.state_dict())}
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    _flat_steps(m, opt, [3])
    want = m.flat_params.clone()
    m2, opt2 = make()
    m2.load_state_dict(ck["state_dict"])
    opt2.load_state_dict(ck["optimizer"])
    _flat_steps(m2, opt2, [3])
    assert torch.equal(m2.flat_params, want)
    assert all(int(opt2.state[p]["step"].item()) == 3 for p in m2.parameters())
    m3, opt3 = make()  # without the optimizer state the step differs
    m3.load_state_dict(ck["state_dict"])
    _flat_steps(m3, opt3, [3])
    assert not torch.equal(m3.flat_params, want)


def test_adamw_state_dict_moves_both_ways_with_torch(dev):
    """a native state_dict() loads into torch.optim.AdamW and torch's into the native class; one more step then agrees.
    Step counts that differ between parameters split the native launch ranges."""
    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.optim import AdamW

    sys.path.insert(0, ROOT)
    import train

    def pair():
        m = resnet50(dtype="fp32").cuda()
        return m, train.filter_from_weight_decay(m, ["bn", "bias"])

    def close(a, b):
        return ((a - b).abs().max() / b.abs().max()).item() < 1e-6

    # native -> torch
    m, groups = pair()
    nat = AdamW(groups, lr=1e-3, weight_decay=5e-2)
    nat.attach_model(m)
    _flat_steps(m, nat, [5, 6])
    mt, gt = pair()
    mt.load_state_dict(m.state_dict())
    ref = torch.optim.AdamW(gt, lr=1e-3, weight_decay=5e-2, foreach=False)
    ref.load_state_dict(copy.deepcopy(nat.state_dict()))
    _flat_steps(m, nat, [7])
    mt.flat_grads.copy_(_grads_for(mt, 7))
    ref.step()
    assert close(m.flat_params, mt.flat_params)
    assert all(int(ref.state[p]["step"].item()) == 3 for g in gt for p in g["params"])
    # torch -> native
    mt, gt = pair()
    ref = torch.optim.AdamW(gt, lr=1e-3, weight_decay=5e-2, foreach=False)
    _flat_steps(mt, ref, [8, 9])
    mn, gn = pair()
    mn.load_state_dict(mt.state_dict())
    nat = AdamW(gn, lr=1e-3, weight_decay=5e-2)
    nat.attach_model(mn)
    sd = copy.deepcopy(ref.state_dict())
    nat.load_state_dict(sd)
    mt.flat_grads.copy_(_grads_for(mt, 10))
    ref.step()
    _flat_steps(mn, nat, [10])
    assert close(mn.flat_params, mt.flat_params)
    for p, q in zip([p for g in gn for p in g["params"]], [p for g in gt for p in g["params"]]):
        assert close(nat.state[p]["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
    # a state with unequal step counts (one group: the whole model is one range): the range splits around the odd parameter,
    # and each part keeps its own bias correction
    mt = resnet50(dtype="fp32").cuda()
    ref = torch.optim.AdamW(mt.parameters(), lr=1e-3, weight_decay=5e-2, foreach=False)
    _flat_steps(mt, ref, [12, 13])
    sd = copy.deepcopy(ref.state_dict())
    sd["state"][5]["step"] = torch.tensor(7.0)
    ref.load_state_dict(copy.deepcopy(sd))
    mn = resnet50(dtype="fp32").cuda()
    mn.load_state_dict(mt.state_dict())
    nat = AdamW(mn.parameters(), lr=1e-3, weight_decay=5e-2)
    nat.attach_model(mn)
    nat.load_state_dict(copy.deepcopy(sd))
    mt.flat_grads.copy_(_grads_for(mt, 14))
    ref.step()
    _flat_steps(mn, nat, [14])
    assert close(mn.flat_params, mt.flat_params)
    ps = list(mn.parameters())
    assert int(nat.state[ps[5]]["step"].item()) == 8 and int(nat.state[ps[4]]["step"].item()) == 3
    assert len(nat._plans[0]) == 3


def test_model_ema_inside_the_adamw_kernel_matches_the_callback(dev):
    """ModelEma (train.py:111-112) under the native AdamW: the average advanced by the step kernel (attach_ema) equals the
    callback's own lerp after every batch"""
    H.ema_matches_callback(lambda: H.model_opt("AdamW", dict(weight_decay=5e-2), 0.0), 1e-3)


def test_train_py_runs_the_adamw_smoke_config(dev, tmp_path, monkeypatch):
    from sota_imagenet_amd import optim

    made = []
    build = optim.Adam._build_plans

    def spy(self):
        made.append(self)
        return build(self)

    monkeypatch.setattr(optim.Adam, "_build_plans", spy)
    _, _, run, losses = H.run_smoke_config("adamw_test", tmp_path, ["run.fp16=false", "random_seed=0", "data.pool=2", "log.save_optim=true"],
                                           resume_eval=True)
    assert made and all(type(o) is optim.AdamW for o in made)
    assert losses and all(math.isfinite(x) for x in losses)
    ck = torch.load(os.path.join(run, "model.chpn"), map_location="cpu")
    st = ck["optimizer"]["state"]
    assert st and all({"step", "exp_avg", "exp_avg_sq"} <= set(s) for s in st.values())
    assert ck["optimizer"]["param_groups"][0]["decoupled_weight_decay"] is True
