"""Native MADGRAD / AdaiS (csrc/optim.hip, optim.MADGRAD / optim.AdaiS) on the MI355X against trajectories recorded from the reference's
own program (tests/golden/optim_ref_trajectories.npz, written by tests/golden/make_optim_golden.py on the CPU).

Yardstick, stored in the fixture and never computed from the code under test: after every step and for every tensor, the native
parameters may be no further from the reference's float64 run than FACTOR times the distance of the reference's own float32 run from
it, plus a floor of 4 * 2^-24 (two float32 ulps) of the largest parameter magnitude.  FACTOR = 1.5 is the project's factor
(test_resnet_gpu.py::test_fp32_forward_backward_matches_cpu).  Measured on the MI355X: the device's cbrtf and division needed no more —
the worst native / reference-float32 ratios are 2.42, 1.68 (MADGRAD) and 1.22, 1.18 (AdaiS), and every ratio above 1.5 is an error
below the floor itself (<= 8.4e-8 against 9.8e-8)."""
import copy
import functools
import math
import os
import sys

import pytest
import torch

import optim_harness as H
from madgrad_adais_common import CASES, Fixture
from optim_harness import U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat_problem(fx, dev, p_flat0=None):
    """the fixture's tensors in the layout of the flat models, group by group, so that each group is one range with bridged gaps: zero in
    the gaps of the gradient too, which these launches sweep"""
    return H.fixture_problem(fx, dev, p_flat0, grad_fill=0.0)


def _run(fx, dev, grad_scale=1.0, steps=6):
    ps, groups, fp, fg, offs = _flat_problem(fx, dev)
    opt = H.make_opt(fx, groups, fx.lrs[0])
    opt.grad_scale = grad_scale
    traj, means = [], []
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = fx.lrs[k]
        H.set_grads(ps, fx.split(fx.grads[k]), 1.0 / grad_scale)  # (exact: a power of two)
        opt.step()
        traj.append(H.gather(ps).clone())
        if fx.cls == "AdaiS":
            means.append(opt.exp_avg_sq_hat_mean.clone())
    torch.cuda.synchronize()
    return traj, means, opt, ps, fp


@pytest.mark.parametrize("case", CASES)
def test_steps_follow_the_reference_trajectory(dev, case):
    """six steps on the fixture's inputs, gradients and lr ramp, every step and tensor against the stored yardstick; the same again with
    grad_scale = 0.5 on doubled gradients (figures: the module docstring)"""
    fx = Fixture(case)
    worst = 0.0
    for gs in (1.0, 0.5):
        traj, _, opt, ps, fp = _run(fx, dev, grad_scale=gs)
        for k, got in enumerate(traj):
            worst = max(worst, fx.check(k, got, f"{case} grad_scale={gs}"))
        # the alignment gaps of the flat buffer were bridged into the launches and stayed zero
        mask = H.gaps(ps, fp)
        assert mask.any() and (fp[mask] == 0).all() and [len(segs) for segs in opt._plans] == [1, 1]
    print(f"{case}: worst native / reference-fp32 error ratio {worst:.2f}")
    # the steps really moved the parameters (a no-op would sit far from the trajectory, but make it explicit)
    assert (traj[-1].cpu() - fx.p0).abs().max().item() > 1e-3


@pytest.mark.parametrize("case", ["adais_recipe", "adais_alt"])
def test_adais_mean_matches_the_reference_and_replays_bitwise(dev, case):
    """the device-resident mean of every step against the fixture's float64 mean, within FACTOR times the reference float32 run's own
    relative error plus two float32 ulps; a second run from the same state gives the same bits, parameters included"""
    fx = Fixture(case)
    traj_a, means_a, *_ = _run(fx, dev)
    traj_b, means_b, *_ = _run(fx, dev)
    for k in range(6):
        got = float(means_a[k].item())
        rel = abs(got - fx.mean64[k]) / fx.mean64[k]
        yard = abs(fx.mean32[k] - fx.mean64[k]) / fx.mean64[k]
        print(f"{case} step {k + 1}: mean {got:.9g} (reference fp64 {fx.mean64[k]:.12g})  rel {rel:.3e}  reference fp32 rel {yard:.3e}")
        assert rel <= H.bound(yard, 1.0)
        assert torch.equal(means_a[k], means_b[k]) and torch.equal(traj_a[k], traj_b[k])


KINDS = {"madgrad": ("MADGRAD", dict(momentum=0.9, weight_decay=1e-4), 1e-3), "adais": ("AdaiS", dict(betas=(0.1, 0.99), weight_decay=1e-3), 1e-2)}
LR = {kind: lr for kind, (_, _, lr) in KINDS.items()}


def _model_opt(kind, groups_of=None):
    return H.model_opt(*KINDS[kind], groups_of)


_flat_steps = functools.partial(H.flat_steps, pad=0.0)  # zero in the padding: what a backward leaves there


@pytest.mark.parametrize("kind", ["madgrad", "adais"])
def test_padding_stays_zero_and_the_step_is_the_planned_launches(dev, kind):
    """a real resnet50 flat array (alignment gaps, FC row padding) under attach_model: ONE range, so 1 launch for MADGRAD and 1 + 1 + 1
    for AdaiS; after three steps the padding of p and of every state array is exactly 0, and the AdaiS mean (16384 partial sums)
    equals the mean over the real elements only"""
    m, opt = _model_opt(kind)
    mask = H.padding_mask(m)
    assert mask.any()
    _flat_steps(m, opt, [21, 22, 23], LR[kind])
    segs = [seg for segs in opt._plans for seg in segs]
    assert [len(s) for s in opt._plans] == [1]
    launches = len(segs) if kind == "madgrad" else len(segs) + 1 + len(segs)
    assert launches == (1 if kind == "madgrad" else 3)
    seg = segs[0]
    b = (seg[0].data_ptr() - m.flat_params.data_ptr()) // 4
    pad = mask[b: b + seg[0].numel()]
    assert pad.any() and (seg[0][pad] == 0).all() and torch.isfinite(seg[0]).all()
    states = seg[2:5]  # MADGRAD: grad_sum_sq, s, x0;  AdaiS: exp_avg, exp_avg_sq, beta1_prod
    for t in states:
        assert t.numel() == seg[0].numel() and (t[pad] == 0).all() and (t[~pad] != 0).any() and torch.isfinite(t).all()
    assert (m.flat_params[mask] == 0).all()
    if kind == "adais":
        n_real = int((~mask).sum().item())
        assert opt._param_size == n_real == sum(p.numel() for p in m.parameters())
        bc2 = 1 - 0.99 ** 3
        want = ((seg[3][~pad] / bc2).double().sum() / n_real).item()
        got = float(opt.exp_avg_sq_hat_mean.item())
        assert abs(got - want) <= 4 * U * want, (got, want)
        assert all(opt.state[p]["step"] == 3 and type(opt.state[p]["step"]) is int for p in m.parameters())
    else:
        assert opt.state["k"].dtype == torch.long and opt.state["k"].tolist() == [3] and opt.state["k"].device.type == "cpu"
    # the recipe's two groups (filter_from_wd): the ranges of SGD's planner on the same groups, and AdaiS still takes ONE mean
    sys.path.insert(0, ROOT)
    import train

    from sota_imagenet_amd.optim import SGD

    m2, opt2 = _model_opt(kind, lambda mm: train.filter_from_weight_decay(mm, ["bn", "bias"]))
    _flat_steps(m2, opt2, [24], LR[kind])
    s = SGD(train.filter_from_weight_decay(m2, ["bn", "bias"]), lr=0.0)
    s.attach_model(m2)
    assert [len(x) for x in opt2._plans] == [sum(1 for r in s._merged_ranges() if r[5] == gi) for gi in range(2)]
    assert (m2.flat_params[H.padding_mask(m2)] == 0).all() and torch.isfinite(m2.flat_params).all()
    if kind == "adais":
        v = torch.cat([opt2.state[p]["exp_avg_sq"].reshape(-1) for p in m2.parameters()])
        want = ((v / (1 - 0.99)).double().sum() / v.numel()).item()
        assert abs(float(opt2.exp_avg_sq_hat_mean.item()) - want) <= 4 * U * want


@pytest.mark.parametrize("kind", ["madgrad", "adais"])
def test_model_ema_inside_the_step_kernel_matches_the_callback(dev, kind):
    """ModelEma (train.py:111-112) under the native MADGRAD / AdaiS: the average advanced by the step kernel (attach_ema) equals the
    callback's own lerp after every batch, and the parameters are the same bits either way"""
    H.ema_matches_callback(lambda: _model_opt(kind), LR[kind])


@pytest.mark.parametrize("kind", ["madgrad", "adais"])
def test_resume_continues_bitwise(dev, kind):
    """train.py:140-146 resume: three steps, state_dict into a new optimizer, three more = six uninterrupted steps bit for bit
    (MADGRAD's k and x0, AdaiS's beta1_prod and step counts travel in the state)"""
    m, opt = _model_opt(kind)
    _flat_steps(m, opt, [1, 2, 3], LR[kind])
    ck = {"state_dict": copy.deepcopy(m.state_dict()), "optimizer": copy.deepcopy(opt.state_dict())}
    want_keys = {"grad_sum_sq", "s", "x0"} if kind == "madgrad" else {"step", "exp_avg", "exp_avg_sq", "beta1_prod"}
    assert set(ck["optimizer"]["state"][0]) == want_keys
    if kind == "madgrad":
        assert ck["optimizer"]["state"]["k"].tolist() == [3]
    _flat_steps(m, opt, [4, 5, 6], LR[kind])
    want = m.flat_params.clone()
    m2, opt2 = _model_opt(kind)
    m2.load_state_dict(ck["state_dict"])
    opt2.load_state_dict(ck["optimizer"])
    _flat_steps(m2, opt2, [4, 5, 6], LR[kind])
    assert torch.equal(m2.flat_params, want)
    if kind == "madgrad":
        assert opt2.state["k"].tolist() == [6]
    else:
        assert all(opt2.state[p]["step"] == 6 for p in m2.parameters())
    m3, opt3 = _model_opt(kind)  # without the optimizer state the steps differ
    m3.load_state_dict(ck["state_dict"])
    _flat_steps(m3, opt3, [4, 5, 6], LR[kind])
    assert not torch.equal(m3.flat_params, want)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_has_the_references_layout_and_loads_its_state(dev, case):
    """our state_dict() carries exactly the key set and tensor shapes the reference's did (recorded in the fixture); a state built from
    the reference's float64 state after five steps loads, and the sixth step lands on the reference's sixth step"""
    fx = Fixture(case)
    _, _, opt, ps, _ = _run(fx, dev)
    sd = opt.state_dict()
    order = [i for idx in fx.groups for i in idx]  # state_dict index -> fixture tensor
    assert sorted(k for k in sd["state"] if k != "k") == list(range(len(order)))
    for j, i in enumerate(order):
        st = sd["state"][j]
        assert sorted(st) == fx.state_keys
        for key, shapes in fx.state_shapes.items():
            assert list(st[key].shape) == shapes[i] and st[key].dtype == torch.float32
    if fx.cls == "MADGRAD":
        assert sd["state"]["k"].dtype == torch.long and sd["state"]["k"].tolist() == [6]
        assert set(sd["param_groups"][0]) == {"lr", "eps", "momentum", "weight_decay", "params"}
    else:
        assert "k" not in sd["state"] and all(sd["state"][j]["step"] == 6 for j in range(len(order)))
        assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "params"}
    # reference state after step 5 -> native, then step 6
    ps2, groups2, fp2, fg2, offs2 = _flat_problem(fx, dev, p_flat0=fx.p64[4].float())
    opt2 = H.make_opt(fx, groups2, fx.lrs[5])
    state = {}
    for j, i in enumerate(order):
        state[j] = {key: fx.split(t)[i].view(fx.shapes[i]).clone() for key, t in fx.state5.items()}
        if fx.cls == "AdaiS":
            state[j]["step"] = 5
    if fx.cls == "MADGRAD":
        state["k"] = torch.tensor([5], dtype=torch.long)
    pg = copy.deepcopy(opt2.state_dict()["param_groups"])
    opt2.load_state_dict({"state": state, "param_groups": pg})
    for g in opt2.param_groups:
        g["lr"] = fx.lrs[5]
    H.set_grads(ps2, fx.split(fx.grads[5]))
    opt2.step()
    torch.cuda.synchronize()
    fx.check(5, H.gather(ps2), f"{case} step 6 from the reference's state")


@pytest.mark.parametrize("name,cls_name,keys", [("madgrad_test", "MADGRAD", {"grad_sum_sq", "s", "x0"}),
                                                ("adais_test", "AdaiS", {"step", "exp_avg", "exp_avg_sq", "beta1_prod"})])
def test_train_py_runs_the_smoke_config(dev, tmp_path, monkeypatch, name, cls_name, keys):
    """train.py on madgrad_test.yaml / adais_test.yaml: the native class is built and planned, the loss is finite and decreasing or
    stable (the last epoch's training loss at most 10 % above the first's: a diverging step rule multiplies it), the checkpoint carries
    the reference's state layout and evaluates after a resume"""
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
    assert losses and all(math.isfinite(x) for x in losses) and losses[-1] <= 1.1 * losses[0]
    ck = torch.load(os.path.join(run, "model.chpn"), map_location="cpu")
    st = ck["optimizer"]["state"]
    per_param = [s for k, s in st.items() if k != "k"]
    assert per_param and all(set(s) == keys for s in per_param)
    if cls_name == "MADGRAD":
        assert int(st["k"].item()) > 0
