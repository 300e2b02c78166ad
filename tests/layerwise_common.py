"""What tests/test_layerwise_host.py and tests/test_layerwise_gpu.py share: the fixture recorded from the reference's own MyNovograd, NovogradApex,
AdamLayerwise and MyAdai (tests/golden/layerwise_ref_trajectories.npz, written by tests/golden/make_layerwise_golden.py) and the four update rules
as this project documents them (include/mi355rn.h), restated in torch on the CPU in a chosen dtype."""
import importlib.util
import os

import numpy as np
import torch

from optim_harness import TrajectoryFixture

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "layerwise_ref_trajectories.npz")
CASES = ["nov_recipe", "mynov_recipe", "adamlw_recipe", "myadai_recipe", "adamlw_alt", "nov_alt", "myadai_alt"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_layerwise_golden", os.path.join(HERE, "golden", "make_layerwise_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_PROBLEM = None


def problem_grads():
    """[6, n] float32: the gradients of the fixture's problem, rebuilt from their seeds (the file does not store them)"""
    global _PROBLEM
    if _PROBLEM is None:
        gen = _generator()
        p0, grads = gen.problem()
        _PROBLEM = (gen.flat(p0), torch.stack([gen.flat(g) for g in grads]))
    return _PROBLEM[1]


class Fixture(TrajectoryFixture):
    """the gradients are rebuilt from their seeds; MyAdai's momentum coefficients and second moments where the case records them"""

    GOLDEN = GOLDEN

    def __init__(self, case):
        super().__init__(case)
        self.grads = problem_grads()
        assert torch.equal(self.p0, _PROBLEM[0])  # the seeds rebuild the recorded inputs bit for bit
        self.beta1 = self.rec("beta1") if self.has("beta1") else None
        self.v0 = self.rec("v0") if self.has("v0") else None


class Restated:
    """the four rules, per tensor, in `dtype` on the CPU.  params: list of tensors; group_of[i]: the param group of tensor i; wds: weight decay
    per group; hyper: the constructor's keyword arguments (the class defaults are filled in here as the reference has them)."""

    DEFAULTS = {
        "NovogradApex": dict(betas=(0.95, 0), eps=1e-8, ema_norm_init=1e-3, wd_eps=None),
        "AdamLayerwise": dict(betas=(0.95, 0), eps=1e-6, ema_norm_init=1e-3, stable_wd=False),
        "MyNovograd": dict(betas=(0.9, 0.99), eps=1e-8, ema_norm_init=1e-3),
        "MyAdai": dict(betas=(0.1, 0.99), eps=1e-3, ema_norm_init=1e-3, sgd_mom=False, sqrt_mom=False, stable_wd=False),
    }

    def __init__(self, cls, hyper, params, group_of, wds, dtype):
        self.cls, self.h = cls, dict(self.DEFAULTS[cls], **{k: v for k, v in hyper.items() if k != "weight_decay"})
        self.p = [t.detach().to("cpu", dtype).clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.group_of, self.wds, self.dtype = group_of, wds, dtype
        if cls == "MyAdai":
            self.v = [self.h["ema_norm_init"]] * len(self.p)  # Python floats, never updated
        else:
            self.v = [torch.tensor(self.h["ema_norm_init"], dtype=dtype) for _ in self.p]
        self.steps = 0
        self.beta1 = []

    def step(self, grads, lrs):
        """grads: list of tensors (already multiplied by grad_scale); lrs: lr per group"""
        h = self.h
        b1, b2 = h["betas"]
        if self.cls == "MyAdai":
            mean = h["ema_norm_init"] if self.steps == 0 else sum(self.v) / len(self.v)
            self.beta1.append([])
        for i, g in enumerate(grads):
            g = g.detach().to("cpu", self.dtype)
            p, m, lr, wd = self.p[i], self.m[i], lrs[self.group_of[i]], self.wds[self.group_of[i]]
            if self.cls in ("NovogradApex", "AdamLayerwise"):
                stat = g.pow(2).mean() if self.cls == "AdamLayerwise" else g.pow(2).sum()
                self.v[i] = self.v[i] * b2 + (1 - b2) * stat
                den = self.v[i].sqrt() + h["eps"]
                m = m * b1 + (1 - b1) * (g / den)
                p = p + (-lr) * m
                if h.get("wd_eps") is not None:
                    p = p - (lr * wd) * ((p.abs() - h["wd_eps"]).clamp_min(0) * p.sign())
                elif h.get("stable_wd"):
                    p = p * (1 - lr * wd / den)
                else:
                    p = p * (1 - lr * wd)
            elif self.cls == "MyNovograd":
                self.v[i] = self.v[i] * b2 + (1 - b2) * p.pow(2).sum()  # of the PARAMETER: as the class has it
                den = self.v[i].sqrt() + h["eps"]
                m = m * b1 + (1 - b1) * g
                p = p + (-lr) * (m / den)
                p = p * (1 - lr * wd)
            else:
                vt = self.v[i] * b2 + g.pow(2).mean().item() * (1 - b2)  # not written back
                r = vt / mean
                bt = float(np.clip(1 - (np.sqrt(r) if h["sqrt_mom"] else r) * b1, 0, 1 - h["eps"]))
                self.beta1[-1].append(bt)
                m = m * bt + (1 if h["sgd_mom"] else 1 - bt) * g
                p = p + (-lr) * m
                p = p * ((1 - lr * wd / (1 - bt)) if h["stable_wd"] else (1 - lr * wd))
            self.p[i], self.m[i] = p, m
        self.steps += 1

    def flat(self):
        return torch.cat([t.reshape(-1) for t in self.p])


def restate_fixture(fx, dtype, steps=6):
    """[steps, n]: the restated trajectory on the fixture's problem"""
    group_of = [0 if i in fx.groups[0] else 1 for i in range(len(fx.shapes))]
    wds = [fx.hyper.get("weight_decay", Restated.DEFAULTS[fx.cls].get("weight_decay", 1e-2 if fx.cls == "MyNovograd" else 0)), 0]
    r = Restated(fx.cls, fx.hyper, [t.view(s) for t, s in zip(fx.split(fx.p0), fx.shapes)], group_of, wds, dtype)
    out = []
    for k in range(steps):
        r.step([t.view(s) for t, s in zip(fx.split(fx.grads[k]), fx.shapes)], [fx.lrs[k], fx.lrs[k]])
        out.append(r.flat().clone())
    return torch.stack(out), r
