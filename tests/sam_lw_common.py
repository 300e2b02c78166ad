"""What tests/test_sam_lw_host.py and tests/test_sam_lw_gpu.py share: the fixture recorded from the reference's own SAM callback
(tests/golden/sam_lw_ref_trajectories.npz, written by tests/golden/make_sam_lw_golden.py), the rules of the callback as this project documents
them (include/mi355rn.h) restated in torch on the CPU in a chosen dtype.  (The layout helpers: tests/plan_common.py.)"""
import os

import numpy as np
import torch

import sam_common
from sam_common import HERE, _optimizer_step

GOLDEN = os.path.join(HERE, "golden", "sam_lw_ref_trajectories.npz")
CASES = ["layer_sgd", "unit_sgd", "unit_adamlw"]
GN_FLOOR, WN_FLOOR = 1e-5, 1e-3


def generator():
    """tests/golden/make_sam_lw_golden.py as a module: the problem (shapes, groups, seeds, the quadratic module) is stated there once"""
    return sam_common.generator(Fixture.GENERATOR)


class Fixture(sam_common.CallbackFixture):
    """the norms per slot, and where each tensor's slots lie"""

    GOLDEN = GOLDEN
    GENERATOR = "make_sam_lw_golden"

    def __init__(self, case):
        super().__init__(case)
        self.unitwise, self.gn, self.wn = self.hyper["unitwise"], self.rec("gn"), self.rec("wn")
        self.slot_counts = [s[0] if self.unitwise and len(s) > 1 else 1 for s in self.shapes]  # slots per tensor, in tensor order
        self.slot_offs = np.cumsum([0] + self.slot_counts)


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
