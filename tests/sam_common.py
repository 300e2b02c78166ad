"""What tests/test_sam_host.py and tests/test_sam_gpu.py share: the fixture recorded from the reference's own SAMOriginal callback
(tests/golden/sam_ref_trajectories.npz, written by tests/golden/make_sam_golden.py), the rules of the callback as this project documents them
(include/mi355rn.h) restated in torch on the CPU in a chosen dtype, and the quadratic problem of the fixture."""
import importlib.util
import os

import torch

from optim_harness import TrajectoryFixture, _js

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sam_ref_trajectories.npz")
CASES = ["sgd", "adamlw_recipe", "clamp"]
NORM_FLOOR = 2e-5


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_GEN = {}


def generator(name="make_sam_golden"):
    """tests/golden/<name>.py as a module: the problem (shapes, groups, seeds, the quadratic module) is stated there once"""
    if name not in _GEN:
        _GEN[name] = _load(name)
    return _GEN[name]


class CallbackFixture(TrajectoryFixture):
    """a callback's trajectory: per step the reference's float64 eps, the parameters at the second forward (p + eps) and the parameters after
    the optimizer step, each with the yardstick of the reference's float32 run"""

    GENERATOR = None  # the subclass's recorder, tests/golden/<GENERATOR>.py

    def __init__(self, case):
        super().__init__(case)
        gen = generator(self.GENERATOR)
        assert torch.equal(self.p0, gen.flat(gen.params0()))  # the seeds rebuild the recorded inputs bit for bit
        self.steps, self.kw, self.rho = _js(self.rec("steps")), self.hyper["kw"], self.hyper["rho"]
        self.a = [float(x) for x in self.rec("a")]
        self.forwards = [int(x) for x in self.rec("forwards")]
        self.eps, self.p_step = torch.from_numpy(self.rec("eps")), torch.from_numpy(self.rec("p_step"))
        self.yard = {k: self.rec(f"yard_{k}") for k in ("eps", "pert", "step")}

    def targets(self, k):
        return generator(self.GENERATOR).targets(k)

    def pert(self, k):
        """the float64 run's parameters at the second forward of step k: the parameters before the step plus eps (exact in float64, asserted by
        the generator)"""
        return (self.p0.double() if k == 0 else self.p_step[k - 1]) + self.eps[k]

    def check(self, k, got_flat, what):
        """got_flat: the native values of step k + 1 (what: "eps", "pert" or "step") in the fixture's tensor order, against the float64 run"""
        ref_flat = {"eps": self.eps[k], "pert": self.pert(k), "step": self.p_step[k]}[what]
        return self.check_tensors(got_flat, ref_flat, [float(y) for y in self.yard[what][k]], f"{self.case} {what} step {k + 1}", floor_in_ratio=True)


class Fixture(CallbackFixture):
    GOLDEN = GOLDEN
    GENERATOR = "make_sam_golden"

    def __init__(self, case):
        super().__init__(case)
        self.eta, self.norm = self.hyper["eta"], self.rec("norm")


def sam_norm(ps, gs, eta):
    """max(sqrt(sum over tensors of |w_t|^2), 2e-5): w_t = g * max(|p|, eta) for tensors with more than one dimension, g for the others"""
    tot = sum((g * p.abs().clamp_min(eta) if p.ndim > 1 else g).pow(2).sum() for p, g in zip(ps, gs))
    return tot.sqrt().clamp_min(NORM_FLOOR)


def sam_eps(ps, gs, rho, eta, norm):
    """eps_t = (max(p^2, eta) * g) * (rho / norm) for tensors with more than one dimension, g * (rho / norm) for the others"""
    scale = rho / norm
    return [(p.pow(2).clamp_min(eta) * g) * scale if p.ndim > 1 else g * scale for p, g in zip(ps, gs)]


def _optimizer_step(cls, kw, st, ps, gs, group_of, lr, dtype):
    """torch.optim.SGD with momentum, or AdamLayerwise as layerwise_common.Restated states it; st: the state carried between steps"""
    if cls == "SGD":
        mu, wd = kw["momentum"], kw["weight_decay"]
        first = "m" not in st
        m = st.setdefault("m", [None] * len(ps))
        for i, (p, g) in enumerate(zip(ps, gs)):
            g = g + (wd if group_of[i] == 0 else 0.0) * p
            m[i] = g.clone() if first else m[i] * mu + g
            ps[i] = p - lr * m[i]
        return
    assert cls == "AdamLayerwise"
    from layerwise_common import Restated

    r = st.get("r")
    if r is None:
        r = st["r"] = Restated(cls, kw, ps, group_of, [kw["weight_decay"], 0], dtype)
    r.p = [p.clone() for p in ps]
    r.step(gs, [lr, lr])
    ps[:] = r.p


def restate_fixture(fx, dtype):
    """the documented rules on the fixture's problem in `dtype`: per step (norm or NaN, eps flat, parameters at the second forward flat, parameters
    after the optimizer step flat, forwards made)"""
    ps = [t.to(dtype).view(s).clone() for t, s in zip(fx.split(fx.p0), fx.shapes)]
    group_of = [0 if i in fx.groups[0] else 1 for i in range(len(ps))]
    flat = generator().flat
    st, out = {}, []

    def grads(ps, k):
        return [a * (p - c.to(dtype)) for a, p, c in zip(fx.a, ps, fx.targets(k))]

    for k in range(fx.steps):
        g = grads(ps, k)
        forwards, norm, eps = 1, float("nan"), [torch.zeros_like(p) for p in ps]
        pert = list(ps)
        if st:  # the optimizer has state: every step but the first
            norm = sam_norm(ps, g, fx.eta)
            eps = sam_eps(ps, g, fx.rho, fx.eta, norm)
            pert = [p + e for p, e in zip(ps, eps)]
            g = grads(pert, k)  # the second gradient, at the perturbed parameters
            ps = [p - e for p, e in zip(pert, eps)]
            forwards, norm = 2, float(norm)
        _optimizer_step(fx.cls, fx.kw, st, ps, g, group_of, fx.lrs[k], dtype)
        out.append((norm, flat(eps), flat(pert), flat(ps).clone(), forwards))
    return out
