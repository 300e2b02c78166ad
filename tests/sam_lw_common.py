"""What tests/test_sam_lw_host.py and tests/test_sam_lw_gpu.py share: the fixture recorded from the reference's own SAM callback
(tests/golden/sam_lw_ref_trajectories.npz, written by tests/golden/make_sam_lw_golden.py), the rules of the callback as this project documents
them (include/mi355rn.h) restated in torch on the CPU in a chosen dtype.  (The layout helpers: tests/plan_common.py.)"""
import importlib.util
import json
import os

import numpy as np
import torch

from sam_common import _optimizer_step

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sam_lw_ref_trajectories.npz")
CASES = ["layer_sgd", "unit_sgd", "unit_adamlw"]
U = 2.0 ** -24
FACTOR = 1.5
GN_FLOOR, WN_FLOOR = 1e-5, 1e-3

_GEN = None


def generator():
    """tests/golden/make_sam_lw_golden.py as a module: the problem (shapes, groups, seeds, the quadratic module) is stated there once"""
    global _GEN
    if _GEN is None:
        spec = importlib.util.spec_from_file_location("make_sam_lw_golden", os.path.join(HERE, "golden", "make_sam_lw_golden.py"))
        _GEN = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_GEN)
    return _GEN


def _js(a):
    return json.loads(bytes(a).decode())


class Fixture:
    def __init__(self, case):
        z = np.load(GOLDEN)
        gen = generator()
        self.case = case
        self.shapes, self.groups, self.steps = _js(z["shapes"]), _js(z["groups"]), _js(z["steps"])
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.offs = np.cumsum([0] + self.sizes)
        self.p0 = torch.from_numpy(z["p0"])
        assert torch.equal(self.p0, gen.flat(gen.params0()))  # the seeds rebuild the recorded inputs bit for bit
        h = _js(z[f"{case}/hyper"])
        self.cls, self.kw, self.rho, self.unitwise = h["cls"], h["kw"], h["rho"], h["unitwise"]
        self.a = [float(x) for x in z[f"{case}/a"]]
        self.lrs = [float(x) for x in z[f"{case}/lrs"]]
        self.gn, self.wn = z[f"{case}/gn"], z[f"{case}/wn"]
        self.forwards = [int(x) for x in z[f"{case}/forwards"]]
        self.eps, self.p_step = torch.from_numpy(z[f"{case}/eps"]), torch.from_numpy(z[f"{case}/p_step"])
        self.yard = {k: z[f"{case}/yard_{k}"] for k in ("eps", "pert", "step")}
        self.slot_counts = [s[0] if self.unitwise and len(s) > 1 else 1 for s in self.shapes]  # slots per tensor, in tensor order
        self.slot_offs = np.cumsum([0] + self.slot_counts)

    def targets(self, k):
        return generator().targets(k)

    def split(self, flat):
        return [flat[self.offs[i]:self.offs[i + 1]] for i in range(len(self.shapes))]

    def pert(self, k):
        """the float64 run's parameters at the second forward of step k: the parameters before the step plus eps (exact in float64, asserted by
        the generator)"""
        return (self.p0.double() if k == 0 else self.p_step[k - 1]) + self.eps[k]

    def check(self, k, got_flat, what):
        """got_flat: the native values of step k + 1 (what: "eps", "pert" or "step") in the fixture's tensor order, against the float64 run:
        within 1.5 x the reference's own float32 error + 4 * 2^-24 * max|ref| per tensor (the rule of sam_common.Fixture.check)"""
        ref_flat = {"eps": self.eps[k], "pert": self.pert(k), "step": self.p_step[k]}[what]
        ratios = []
        for i, (got, ref) in enumerate(zip(self.split(got_flat.detach().double().cpu()), self.split(ref_flat))):
            err = (got - ref).abs().max().item()
            yard = float(self.yard[what][k, i])
            floor = 4 * U * ref.abs().max().item()
            ratios.append(err / max(yard, floor))
            print(f"{self.case} {what} step {k + 1} tensor {i}: native {err:.3e}  reference fp32 {yard:.3e}  floor {floor:.2e}")
            assert err <= FACTOR * yard + floor, f"{self.case} {what} step {k + 1} tensor {i}: native {err:.3e} vs reference fp32 {yard:.3e}"
        return max(ratios)


def slot_norms(x, unitwise):
    """||x||_2 per slot, as a vector: one value for the whole tensor, or one per index of dim 0 for a unit-wise tensor with ndim > 1"""
    if unitwise and x.ndim > 1:
        return x.reshape(x.shape[0], -1).pow(2).sum(1).sqrt()
    return x.pow(2).sum().sqrt().reshape(1)


def sam_lw_eps(ps, gs, rho, unitwise):
    """per tensor (eps, gn, wn): gn = max(||g||, 1e-5), wn = max(||p||, 1e-3) per slot, eps = ((wn / gn) * g) * rho"""
    out = []
    for p, g in zip(ps, gs):
        gn, wn = slot_norms(g, unitwise).clamp_min(GN_FLOOR), slot_norms(p, unitwise).clamp_min(WN_FLOOR)
        c = wn / gn
        c = c.reshape([-1] + [1] * (p.ndim - 1)) if c.numel() > 1 else c.reshape(())
        out.append(((c * g) * rho, gn, wn))
    return out


def restate_fixture(fx, dtype):
    """the documented rules on the fixture's problem in `dtype`: per step (gn per slot, wn per slot, eps flat, parameters at the second forward
    flat, parameters after the optimizer step flat, forwards made)"""
    ps = [t.to(dtype).view(s).clone() for t, s in zip(fx.split(fx.p0), fx.shapes)]
    group_of = [0 if i in fx.groups[0] else 1 for i in range(len(ps))]
    flat = generator().flat
    st, out = {}, []

    def grads(ps, k):
        return [a * (p - c.to(dtype)) for a, p, c in zip(fx.a, ps, fx.targets(k))]

    for k in range(fx.steps):
        res = sam_lw_eps(ps, grads(ps, k), fx.rho, fx.unitwise)
        eps = [r[0] for r in res]
        pert = [p + e for p, e in zip(ps, eps)]
        g = grads(pert, k)  # the second gradient, at the perturbed parameters
        ps = [p - e for p, e in zip(pert, eps)]
        _optimizer_step(fx.cls, fx.kw, st, ps, g, group_of, fx.lrs[k], dtype)
        out.append((torch.cat([r[1] for r in res]), torch.cat([r[2] for r in res]), flat(eps), flat(pert), flat(ps).clone(), 2))
    return out
