"""What tests/test_adamp_host.py and tests/test_adamp_gpu.py share: the fixture tests/golden/adamp_ref_trajectories.npz and the AdamP rule restated
in torch on the CPU in a chosen dtype.

Provenance: the `adamp` package is not available to this project.  The rule is the published adamp.AdamP.step (package 0.3.0) written down from
memory of the public package in tests/golden/make_adamp_golden.py (adamp_tensor_step, which the plain restatement here calls); parity of the
native AdamP is against that restatement and is unpinned against the package itself.  With native=True the restatement uses the arithmetic that
include/mi355rn.h and csrc/optim_adamp.hip document for the kernels: float32 element operations, one rounding each, coefficients formed in double
and rounded once, the sums of the decision in double, s = sum(p*u)/d."""
import importlib.util
import math
import os

import torch

from optim_harness import TrajectoryFixture

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "adamp_ref_trajectories.npz")
CASES = ["adamp_recipe51", "adamp_alt"]


def recorder():
    spec = importlib.util.spec_from_file_location("make_adamp_golden", os.path.join(HERE, "golden", "make_adamp_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = recorder()
DEFAULTS = GEN.DEFAULTS


class Fixture(TrajectoryFixture):
    """four steps; param groups, inputs and gradients per case; the yardstick is the restatement's float32 run; state4: its float32 moments"""

    GOLDEN = GOLDEN
    YARD_NAME = "restated fp32"

    def __init__(self, case):
        super().__init__(case)
        self.shapes = [tuple(s) for s in self.shapes]
        if "betas" in self.hyper:
            self.hyper["betas"] = tuple(self.hyper["betas"])
        self.wds, self.grads = [float(x) for x in self.rec("wds")], torch.from_numpy(self.rec("grads"))
        self.modes, self.margins, self.effect = self.rec("modes"), self.rec("margins"), self.rec("effect")
        self.state4 = self.states("state4")
        self.group_of = [next(gi for gi, idx in enumerate(self.groups) if i in idx) for i in range(len(self.shapes))]
        self.order = [i for idx in self.groups for i in idx]  # param-group order -> fixture tensor

    def split(self, flat):
        return [t.view(shape) for t, shape in zip(super().split(flat), self.shapes)]

    def tensor_label(self, i):
        return f"tensor {i} {self.shapes[i]}"


def f32(x):
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32)


def slot_rows(t):
    """[slots, unit_len] view of a tensor: one row per index of dim 0, or one row in all for ndim <= 1"""
    return t.reshape(t.shape[0] if t.dim() > 1 else 1, -1)


def per_elem(stat, like):
    """one value per slot, broadcast to the elements of `like`"""
    return stat.reshape((-1,) + (1,) * (like.dim() - 1)).expand_as(like) if like.dim() > 1 else stat.reshape(()).expand_as(like)


def native_direction(p, g, m, v, h, step, grad_scale=1.0):
    """(ge, m', v', u) of one tensor in the kernels' float32 arithmetic (adamp_elem of csrc/optim_adamp.hip)"""
    b1, b2 = h["betas"]
    ge = g * f32(grad_scale)
    b1f, gwf, b2f, g2f = f32(b1), f32(1 - b1), f32(b2), f32(1 - b2)
    sq2f, epsf = f32(math.sqrt(1 - b2 ** step)), f32(h["eps"])
    mn = b1f * m + gwf * ge
    vn = b2f * v + (g2f * ge) * ge
    # the kernels' sqrtf is correctly rounded; torch's float32 sqrt on the CPU is not everywhere (it differs from the rounded float64 root in
    # about one element of 200), so the root is taken in float64 and rounded once — which for a square root equals the correctly rounded float32
    den = vn.double().sqrt().float() / sq2f + epsf
    u = (b1f * mn + gwf * ge) / den if h["nesterov"] else mn / den
    return ge, mn, vn, u


def native_decision(p, ge, u, h, lr, wd):
    """(mode, d [slots], s [slots], wdf) of one tensor as stage (b) documents it: sums in double, (d, s) and wdf rounded once to float32"""
    eps, rows = h["eps"], slot_rows(p).shape[0]
    mode, d, s = 0, torch.ones(rows, dtype=torch.float64), torch.zeros(rows, dtype=torch.float64)
    if p.dim() > 1:
        P, G, Uu = slot_rows(p).double(), slot_rows(ge).double(), slot_rows(u).double()
        Sgg, Spp, Sgp, Spu = (G * G).sum(1), (P * P).sum(1), (G * P).sum(1), (P * Uu).sum(1)

        def cos(gg, pp, gp):
            return gp.abs() / (gg.sqrt().clamp_min(eps) * pp.sqrt().clamp_min(eps))

        if cos(Sgg, Spp, Sgp).max().item() < h["delta"] / math.sqrt(P.shape[1]):
            mode, d = 1, Spp.sqrt() + eps
            s = Spu / d
        elif cos(Sgg.sum(), Spp.sum(), Sgp.sum()).item() < h["delta"] / math.sqrt(P.numel()):
            mode = 2
            d = (Spp.sum().sqrt() + eps).expand(rows)
            s = Spu.sum().expand(rows) / d
    wdf = f32(1 - lr * wd * (h["wd_ratio"] if mode else 1.0)) if wd > 0 else f32(1.0)
    return mode, d.float(), s.float(), wdf


class Restated:
    """AdamP per tensor on the CPU.  native=False: adamp_tensor_step of the recorder in `dtype`.  native=True (float32): the kernels' documented
    arithmetic; with coef / wdf handed to step() — per tensor the device's (d, s) per slot and its decay factor — the update of stage (c) alone."""

    def __init__(self, hyper, params, group_of, wds, dtype, native=False):
        self.h = dict(DEFAULTS, **hyper)
        self.dtype, self.native = dtype, native
        self.p = [t.detach().to("cpu", dtype).clone() for t in params]
        self.st = [dict(step=0, exp_avg=torch.zeros_like(t), exp_avg_sq=torch.zeros_like(t)) for t in self.p]
        self.group_of, self.wds = group_of, wds
        self.ema, self.modes = None, []

    def step(self, grads, lrs, grad_scale=1.0, coef=None, wdf=None, ema_decay=None):
        self.modes = []
        for i, g in enumerate(grads):
            g = g.detach().to("cpu", self.dtype)
            lr, wd, st = lrs[self.group_of[i]], self.wds[self.group_of[i]], self.st[i]
            if not self.native:
                self.p[i], md, _ = GEN.adamp_tensor_step(self.p[i], g * grad_scale, st, self.h, lr, wd)
                self.modes.append(md)
                continue
            p = self.p[i]
            st["step"] += 1
            ge, mn, vn, u = native_direction(p, g, st["exp_avg"], st["exp_avg_sq"], self.h, st["step"], grad_scale)
            if coef is None:
                md, d, s, w = native_decision(p, ge, u, self.h, lr, wd)
            else:
                md, d, s, w = None, coef[i][:, 0].cpu(), coef[i][:, 1].cpu(), wdf[i].cpu()
            self.modes.append(md)
            d, s = per_elem(d, p), per_elem(s, p)
            pn = p / d
            u = u - pn * s
            p = p * w
            p = p + f32(-lr / (1 - self.h["betas"][0] ** st["step"])) * u
            self.p[i], st["exp_avg"], st["exp_avg_sq"] = p, mn, vn
            if ema_decay is not None:
                w1 = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(float(ema_decay), dtype=torch.float32)
                self.ema[i] = self.ema[i] + w1 * (p - self.ema[i])

    def flat(self):
        return torch.cat([t.reshape(-1) for t in self.p])
