"""MADGRAD / AdaiS on the host: the reference's optimizer targets resolve to the native classes, the new configs compose, the C-ABI
entries refuse bad arguments before any launch, the constructors keep the reference's domains, and the two update rules as this
project documents them (include/mi355rn.h) reproduce — restated here in float64 torch — the trajectories that the
reference's own program recorded in tests/golden/optim_ref_trajectories.npz (tests/golden/make_optim_golden.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from madgrad_adais_common import CASES, GOLDEN, Fixture
from sota_imagenet_amd import config as C
from sota_imagenet_amd import native


def test_madgrad_adais_targets_resolve_to_the_native_classes():
    from sota_imagenet_amd import optim

    for target in ("src.optimizers.MADGRAD", "sota_imagenet.optimizers.MADGRAD"):
        assert C.resolve_target(target) is optim.MADGRAD
    for target in ("src.optimizers.AdaiS", "sota_imagenet.optimizers.AdaiS"):
        assert C.resolve_target(target) is optim.AdaiS
    assert issubclass(optim.MADGRAD, optim._FlatOptimizer) and issubclass(optim.AdaiS, optim._FlatOptimizer)
    # not in the reference tree or deliberately left out: stay unaliased
    assert "src.optimizers.MyAdai" not in C.TARGET_ALIASES and "pytorch_tools.optim.AdamP" not in C.TARGET_ALIASES


def test_madgrad_adais_configs_compose_and_instantiate():
    from sota_imagenet_amd import optim

    ps = [{"params": [torch.nn.Parameter(torch.zeros(4))]}]
    cfg = C.compose(None, ["+hydra_exp=r50_madgrad"])
    assert cfg.optim._target_ == "src.optimizers.MADGRAD" and cfg.optim.lr == 0 and cfg.optim.weight_decay == 1e-4
    assert cfg.loader.batch_size == 192 and cfg.loader.color_twist_prob == 0.3 and cfg.run.ema_decay == 0.9993
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 5, [0.0001, 0.002], "linear"), (5, 90, [0.002, 0], "cos")]
    assert cfg.criterion.smoothing == 0.1 and cfg.loader.image_size == 224
    o = C.call(cfg.optim, ps)
    assert type(o) is optim.MADGRAD and o.defaults == dict(lr=0, eps=1e-6, momentum=0.9, weight_decay=1e-4)

    cfg = C.compose(None, ["+hydra_exp=r50_adais"])
    assert cfg.optim._target_ == "src.optimizers.AdaiS" and cfg.optim.betas == [0.1, 0.99] and cfg.optim.weight_decay == 1e-3
    assert cfg.loader.batch_size == 192 and cfg.loader.color_twist_prob == 0.3 and cfg.run.ema_decay == 0.9993
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 5, [0.0001, 0.1], "linear"), (5, 90, [0.1, 0], "cos")]
    o = C.call(cfg.optim, ps)
    assert type(o) is optim.AdaiS and o.defaults["eps"] == 1e-3 and o.ema_norm_init == 1e-3
    for name, cls in (("madgrad_test", optim.MADGRAD), ("adais_test", optim.AdaiS)):
        cfg = C.compose(None, [f"+hydra_exp={name}"])
        assert cfg.log.exp_name == name and cfg.debug is True and "momentum" not in C.to_plain(cfg.optim)
        assert type(C.call(cfg.optim, ps)) is cls
    # the recipes' extra callbacks are left out: the default no-op callbacks stay
    for name in ("r50_madgrad", "r50_adais"):
        cbs = C.compose(None, [f"+hydra_exp={name}"]).run.extra_callbacks
        assert all(cb["_target_"] == "pytorch_tools.fit_wrapper.callbacks.Callback" for cb in cbs)


P = ctypes.c_void_p


def _madgrad(L, p=4096, g=4096, q=4096, s=4096, x0=4096, ema=None, lr=1e-3, mom=0.9, wd=0.0, eps=1e-6, k=0, ema_decay=0.99):
    # n = 0: even a call that passed validation would touch no memory (these addresses are never dereferenced)
    args = [P(p), P(g), P(q), P(s), P(x0)]
    tail = [0, lr, mom, wd, eps, k, 1.0]
    if ema is None:
        return L.mi355_madgrad_step(*args, *tail, None)
    return L.mi355_madgrad_step_ema(*args, P(ema), *tail, ema_decay, None)


def test_madgrad_bad_arguments_return_status_not_crash():
    L = native.lib()
    assert _madgrad(L, p=4096 + 4) == -1 and "aligned" in native.last_error()
    assert _madgrad(L, x0=4096 + 8) == -1 and "aligned" in native.last_error()
    assert _madgrad(L, ema=4096 + 8) == -1 and "aligned" in native.last_error()
    assert _madgrad(L, s=0) == -1 and "null" in native.last_error()
    assert _madgrad(L, mom=1.0) == -1 and "momentum" in native.last_error()
    assert _madgrad(L, mom=-0.1) == -1 and "momentum" in native.last_error()
    assert _madgrad(L, eps=-1e-6) == -1 and "eps" in native.last_error()
    assert _madgrad(L, lr=float("nan")) == -1 and "lr" in native.last_error()
    assert _madgrad(L, lr=float("inf")) == -1 and "lr" in native.last_error()
    assert _madgrad(L, wd=-1.0) == -1 and "weight_decay" in native.last_error()
    assert _madgrad(L, k=-1) == -1 and "k=" in native.last_error()
    assert _madgrad(L, ema=4096, ema_decay=2.0) == -1 and "ema_decay" in native.last_error()
    rc = L.mi355_madgrad_step_ema(P(4096), P(4096), P(4096), P(4096), P(4096), None, 0, 1e-3, 0.9, 0.0, 1e-6, 0, 1.0, 0.9, None)
    assert rc == -1 and "null ema" in native.last_error()


def _adais_step(L, p=4096, g=4096, m=4096, v=4096, bp=4096, mean=4096, ema=None, lr=1e-3, b0=0.1, b2=0.99, eps=1e-3, wd=1e-3, step=1,
                ema_decay=0.99):
    args = [P(p), P(g), P(m), P(v), P(bp), P(mean)]
    tail = [0, lr, b0, b2, eps, wd, step, 1.0]
    if ema is None:
        return L.mi355_adais_step(*args, *tail, None)
    return L.mi355_adais_step_ema(*args, P(ema), *tail, ema_decay, None)


def test_adais_bad_arguments_return_status_not_crash():
    L = native.lib()
    # (a) moments
    assert L.mi355_adais_moments(P(4096), P(4096 + 4), 0, 0.99, 1, 1.0, P(4096), None) == -1 and "aligned" in native.last_error()
    assert L.mi355_adais_moments(P(4096), P(4096), 0, 0.99, 1, 1.0, P(4096 + 4), None) == -1 and "aligned" in native.last_error()
    assert L.mi355_adais_moments(None, P(4096), 0, 0.99, 1, 1.0, P(4096), None) == -1 and "null" in native.last_error()
    assert L.mi355_adais_moments(P(4096), P(4096), 0, 0.99, 1, 1.0, None, None) == -1 and "null" in native.last_error()
    assert L.mi355_adais_moments(P(4096), P(4096), 0, 1.0, 1, 1.0, P(4096), None) == -1 and "beta2" in native.last_error()
    assert L.mi355_adais_moments(P(4096), P(4096), 0, 0.99, 0, 1.0, P(4096), None) == -1 and "step" in native.last_error()
    # (b) mean
    assert L.mi355_adais_mean(None, 8, 1, P(4096), None) == -1 and "null" in native.last_error()
    assert L.mi355_adais_mean(P(4096), 8, 1, None, None) == -1 and "null" in native.last_error()
    assert L.mi355_adais_mean(P(4096), 0, 1, P(4096), None) == -1 and "count" in native.last_error()
    assert L.mi355_adais_mean(P(4096), 12, 1, P(4096), None) == -1 and "whole number" in native.last_error()
    assert L.mi355_adais_mean(P(4096), 8, 0, P(4096), None) == -1 and "param_size" in native.last_error()
    assert L.mi355_adais_mean(P(4096 + 4), 8, 1, P(4096), None) == -1 and "misaligned" in native.last_error()
    # (c) step
    assert _adais_step(L, p=4096 + 4) == -1 and "aligned" in native.last_error()
    assert _adais_step(L, ema=4096 + 8) == -1 and "aligned" in native.last_error()
    assert _adais_step(L, mean=0) == -1 and "null" in native.last_error()
    assert _adais_step(L, bp=0) == -1 and "null" in native.last_error()
    assert _adais_step(L, b2=1.0) == -1 and "beta2" in native.last_error()
    assert _adais_step(L, b2=-0.5) == -1 and "beta2" in native.last_error()
    assert _adais_step(L, b0=-0.1) == -1 and "beta0" in native.last_error()
    assert _adais_step(L, eps=-1e-3) == -1 and "eps" in native.last_error()
    assert _adais_step(L, lr=float("inf")) == -1 and "lr" in native.last_error()
    assert _adais_step(L, step=0) == -1 and "step" in native.last_error()
    assert _adais_step(L, ema=4096, ema_decay=-1.0) == -1 and "ema_decay" in native.last_error()
    rc = L.mi355_adais_step_ema(P(4096), P(4096), P(4096), P(4096), P(4096), P(4096), None, 0, 1e-3, 0.1, 0.99, 1e-3, 0.0, 1, 1.0, 0.9, None)
    assert rc == -1 and "null ema" in native.last_error()
    # the workspace size is a function of n alone: one double per workgroup of 256 float4 (the scalar tail rides in workgroup 0), capped
    assert L.mi355_adais_workspace_bytes(5) == 8 and L.mi355_adais_workspace_bytes(1024 * 10 + 3) == 8 * 10
    assert L.mi355_adais_workspace_bytes(1024 * 10 + 4) == 8 * 11
    assert L.mi355_adais_workspace_bytes(25557032) == L.mi355_adais_workspace_bytes(10 ** 9) == 8 * 16384


def test_constructor_domains_are_the_references():
    from sota_imagenet_amd import optim

    ps = [torch.nn.Parameter(torch.zeros(4))]
    m = optim.MADGRAD(ps)
    assert m.defaults == dict(lr=1e-2, eps=1e-6, momentum=0.9, weight_decay=0)
    optim.MADGRAD(ps, lr=0)  # the stated deviation: the recipe constructs with the base config's lr 0
    for bad in (dict(momentum=1), dict(momentum=-0.1), dict(lr=-1e-3), dict(weight_decay=-1e-4), dict(eps=-1e-6)):
        with pytest.raises(ValueError):
            optim.MADGRAD(ps, **bad)
    optim.MADGRAD(ps, momentum=0, eps=0)
    a = optim.AdaiS(ps)
    assert a.defaults == dict(lr=0, betas=(0.1, 0.99), eps=1e-3, weight_decay=0) and a.ema_norm_init == 1e-3
    for bad in (dict(lr=-1.0), dict(eps=-1e-3), dict(betas=(-0.1, 0.99)), dict(betas=(0.1, 1.0)), dict(betas=(0.1, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            optim.AdaiS(ps, **bad)
    optim.AdaiS(ps, betas=(1.5, 0.0), eps=0)  # beta0 has no upper bound in the reference


# ---- the documented rules, restated in float64, against the reference's recorded float64 trajectories ----------------------------
def _madgrad_rule(p, g, st, k, lr, momentum, weight_decay, eps):
    lamb = (lr + eps) * (k + 1) ** 0.5
    st["gss"] = st["gss"] + lamb * g * g
    rms = st["gss"].pow(1 / 3) + eps
    st["s"] = st["s"] + lamb * g
    z = st["x0"] - st["s"] / rms
    p = p * momentum + (1 - momentum) * z
    return p * (1 - weight_decay)


def _adais_moments_rule(g, st, step, beta2):
    st["v"] = st["v"] * beta2 + (1 - beta2) * g * g
    return st["v"] / (1 - beta2 ** step)


def _adais_step_rule(p, g, st, vhat, mean, lr, beta0, eps, weight_decay):
    if weight_decay != 0:
        p = p * (1 - lr * weight_decay)
    beta1 = (1 - vhat / mean * beta0).clamp(0.0, 1 - eps)
    st["b1prod"] = st["b1prod"] * beta1
    st["m"] = st["m"] * beta1 + (1 - beta1) * g
    return p - lr * st["m"] / (1 - st["b1prod"])


@pytest.mark.parametrize("case", CASES)
def test_documented_rules_reproduce_the_reference_fp64_trajectory(case):
    fx = Fixture(case)
    hyper, n = fx.hyper, len(fx.shapes)
    wd_of = {i: (hyper["weight_decay"] if gi == 0 else 0.0) for gi, idx in enumerate(fx.groups) for i in idx}
    p = [t.double() for t in fx.split(fx.p0)]
    grads = fx.grads.double()
    if fx.cls == "MADGRAD":
        st = [dict(gss=torch.zeros_like(q), s=torch.zeros_like(q), x0=q.clone()) for q in p]
    else:
        st = [dict(v=torch.full_like(q, hyper.get("ema_norm_init", 1e-3)), m=torch.zeros_like(q), b1prod=torch.ones_like(q)) for q in p]
    for k in range(grads.shape[0]):
        gs = fx.split(grads[k])
        if fx.cls == "MADGRAD":
            p = [_madgrad_rule(p[i], gs[i], st[i], k, fx.lrs[k], hyper["momentum"], wd_of[i], hyper["eps"]) for i in range(n)]
        else:
            beta0, beta2 = hyper["betas"]
            vhat = [_adais_moments_rule(gs[i], st[i], k + 1, beta2) for i in range(n)]
            mean = sum(h.sum() for h in vhat) / sum(fx.sizes)
            assert abs(float(mean) - float(fx.mean64[k])) <= 1e-12 * abs(float(mean))
            p = [_adais_step_rule(p[i], gs[i], st[i], vhat[i], mean, fx.lrs[k], beta0, hyper["eps"], wd_of[i]) for i in range(n)]
        got = torch.cat(p)
        rel = ((got - fx.p64[k]).abs().max() / fx.p64[k].abs().max()).item()
        assert rel <= 1e-12, f"{case} step {k + 1}: {rel:.3e}"
    # the trajectory moves (a no-op rule would not pass by accident) and the recorded float32 run is a usable yardstick
    assert (fx.p64[-1] - fx.p0.double()).abs().max().item() > 1e-3
    assert (fx.yard > 0).all() and fx.yard.max() < 1e-4


def test_fixture_records_both_ends_of_the_adais_clamp():
    z = np.load(GOLDEN)
    for case in ("adais_recipe", "adais_alt"):
        clamp = z[f"{case}/clamp"]
        assert clamp.shape == (6, 2) and (clamp > 0.005).all() and (clamp.sum(1) < 0.5).all()
    assert os.path.getsize(GOLDEN) < 768 * 1024
