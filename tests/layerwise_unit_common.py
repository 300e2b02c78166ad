"""What tests/test_layerwise_unit_host.py and tests/test_layerwise_unit_gpu.py share: the fixture recorded from the reference's own MyNovograd and
NovogradApex with unitwise_norm=True (tests/golden/layerwise_unit_ref_trajectories.npz, written by tests/golden/make_layerwise_unit_golden.py) and
the unit-wise rule as this project documents it (include/mi355rn.h), restated in torch on the CPU in a chosen dtype."""
import os

import torch

from layerwise_common import HERE, Fixture

GOLDEN = os.path.join(HERE, "golden", "layerwise_unit_ref_trajectories.npz")
CASES = ["mynov_unit_recipe", "nov_unit", "nov_unit_alt"]
V_KEY = {"MyNovograd": "ema_norm", "NovogradApex": "exp_avg_sq"}
M_KEY = {"MyNovograd": "ema_grad", "NovogradApex": "exp_avg"}


class UnitFixture(Fixture):
    """layerwise_common.Fixture over the unit-wise file, with the float32 second moment after step 5 and its spread"""

    GOLDEN = GOLDEN

    def __init__(self, case):
        super().__init__(case)
        self.v32_5, self.spread, self.vs_layerwise = torch.from_numpy(self.rec("v32_5")), self.rec("spread"), float(self.rec("vs_layerwise"))
        self.v_key, self.m_key = V_KEY[self.cls], M_KEY[self.cls]


def slot_rows(t):
    """[slots, unit_len] view of a tensor: one row per index of dim 0, or one row in all for ndim <= 1"""
    return t.reshape(t.shape[0] if t.dim() > 1 else 1, -1)


def slot_norms(t):
    """the reference's unitwise_norm without the expand: sqrt of the sum of squares per slot, [slots]"""
    return slot_rows(t).pow(2).sum(1).sqrt()


def per_elem(stat, like):
    """one value per slot, broadcast to the elements of `like`"""
    return stat.reshape((-1,) + (1,) * (like.dim() - 1)).expand_as(like) if like.dim() > 1 else stat.reshape(()).expand_as(like)


def f32(x):
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32)


class UnitRestated:
    """MyNovograd / NovogradApex with unitwise_norm=True, per tensor, on the CPU.  dtype float64: the rule in exact-ish arithmetic.  dtype float32
    with native=True: the arithmetic the kernels document — the statistic and the second moment in double rounded once to the float32 v, the
    coefficients formed in double and rounded once, every element operation a float32 operation of its own — and, with `den` given to step(),
    the update alone."""

    def __init__(self, cls, hyper, params, group_of, wds, dtype, native=False):
        self.cls, self.dtype, self.native = cls, dtype, native
        d = dict(betas=(0.9, 0.99) if cls == "MyNovograd" else (0.95, 0), eps=1e-8, ema_norm_init=1e-3, wd_eps=None)
        self.h = dict(d, **{k: v for k, v in hyper.items() if k not in ("weight_decay", "unitwise_norm")})
        self.p = [t.detach().to("cpu", dtype).clone() for t in params]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.full((slot_rows(t).shape[0],), self.h["ema_norm_init"], dtype=dtype) for t in self.p]
        self.group_of, self.wds = group_of, wds
        self.ema = None

    def step(self, grads, lrs, den=None, grad_scale=1.0, ema_decay=None):
        b1, b2 = self.h["betas"]
        for i, g in enumerate(grads):
            g = g.detach().to("cpu", self.dtype)
            if self.native:
                g = g * f32(grad_scale)
            p, m, lr, wd = self.p[i], self.m[i], lrs[self.group_of[i]], self.wds[self.group_of[i]]
            x = p if self.cls == "MyNovograd" else g
            if den is not None:
                dn = den[i].to("cpu", self.dtype)
            elif self.native:
                v = (self.v[i].double() * b2 + (1 - b2) * slot_norms(x.double())).to(self.dtype)
                self.v[i] = v
                dn = (v.double().sqrt() + self.h["eps"]).to(self.dtype)
            else:
                self.v[i] = self.v[i] * b2 + (1 - b2) * slot_norms(x)
                dn = self.v[i].sqrt() + self.h["eps"]
            dn = per_elem(dn, p)
            soft = self.h.get("wd_eps") is not None
            c1, gw, nlr, wdf = b1, 1 - b1, -lr, (lr * wd if soft else 1 - lr * wd)
            if self.native:
                c1, gw, nlr, wdf = f32(c1), f32(gw), f32(nlr), f32(wdf)
            if self.cls == "NovogradApex":
                m = m * c1 + gw * (g / dn)
                p = p + nlr * m
                if soft:
                    we = f32(self.h["wd_eps"]) if self.native else self.h["wd_eps"]
                    p = p - wdf * torch.copysign((p.abs() - we).clamp_min(0), p)
                else:
                    p = p * wdf
            else:
                m = m * c1 + gw * g
                p = p + nlr * (m / dn)
                p = p * wdf
            self.p[i], self.m[i] = p, m
            if ema_decay is not None:
                w = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(ema_decay), dtype=torch.float32)
                self.ema[i] = self.ema[i] + w * (p - self.ema[i])

    def flat(self):
        return torch.cat([t.reshape(-1) for t in self.p])


def restate_fixture(fx, dtype, steps=6, native=False):
    """[steps, n]: the restated trajectory on the fixture's problem"""
    group_of = [0 if i in fx.groups[0] else 1 for i in range(len(fx.shapes))]
    wds = [fx.hyper.get("weight_decay", 1e-2 if fx.cls == "MyNovograd" else 0), 0]
    r = UnitRestated(fx.cls, fx.hyper, [t.view(s) for t, s in zip(fx.split(fx.p0), fx.shapes)], group_of, wds, dtype, native)
    out = []
    for k in range(steps):
        r.step([t.view(s) for t, s in zip(fx.split(fx.grads[k]), fx.shapes)], [fx.lrs[k], fx.lrs[k]])
        out.append(r.flat().clone())
    return torch.stack(out), r
