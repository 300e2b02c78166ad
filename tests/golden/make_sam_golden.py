#!/usr/bin/env python3
"""Records tests/golden/sam_ref_trajectories.npz by running the REFERENCE's own SAMOriginal callback (sota_imagenet/callbacks.py of a reference
checkout, loaded by path; none of its text is here) on the CPU with one thread, once in float32 and once in float64.

    python tests/golden/make_sam_golden.py --reference <checkout of the reference>

The reference module imports pytorch_tools and loguru, which need not be installed: stub modules written here (a Callback base, Cutmix / Mixup
classes, a pass-through rank_zero_only, losses.Loss = nn.Module, a logger) are put into sys.modules first.  The callback runs against a fake
runner state holding model, optimizer, criterion, input and a grad scaler whose unscale_ / update / scale do nothing (the bf16 path of this project
has no loss scaling).

The problem: six tensors ([16,3,3,3], [16], [32,16,1,1], [10,37], [5], [41,13,3,3] — the last has 4797 elements: more than one 4096-element work
item, with a tail that is no multiple of 4) in two param groups, the second (the 1-D tensors) with weight_decay 0.  p0 = synth.uniform_tensor in
+-0.5, so both regimes p^2 < eta and p^2 > eta occur (asserted).  The "model" is a module whose loss is sum_t 0.5 * a_t * |p_t - c_t^k|^2 with
targets c_t^k rebuilt from seeds per step and per-tensor weights a_t spread over several decades: the gradient a_t * (p_t - c_t^k) is an exact
elementwise function of the parameters, at the perturbed parameters too.  Four steps on an lr ramp; the first one the callback skips (the
optimizer has no state yet).

Cases: sgd (torch.optim.SGD, momentum 0.9), adamlw_recipe (the reference's own AdamLayerwise with the values of recipe 49), clamp (SGD with a_t
so small that sqrt(S) < 2e-5: the norm sits at its floor, asserted).

Arrays of the file (i = tensor index; flat = the tensors concatenated in index order):
    p0 [n], shapes, groups, steps (json)      inputs (float32); the targets are not stored: targets() of this file rebuilds them from their seeds
    <case>/a [6], <case>/lrs [4], <case>/hyper (json: cls, kw, rho, eta)
    <case>/norm [4]                           the clamped norm of the float64 run (NaN for the skipped step)
    <case>/eps [4, n]                         eps of the float64 run (zeros for the skipped step)
    <case>/p_step [4, n]                      parameters of the float64 run after the optimizer step
                                              (the parameters the second forward saw are not stored: in float64 they are, bit for bit, the
                                              parameters before the step plus eps — asserted here — and pert() of tests/sam_common.py rebuilds them)
    <case>/forwards [4]                       forwards the step made (1 for the skipped step, 2 after it)
    <case>/yard_eps, yard_pert, yard_step [4, 6]   max |float32 run - float64 run| per step and tensor: the reference's own float32 error
"""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from sota_imagenet_amd.synth import uniform_tensor  # noqa: E402

SHAPES = [(16, 3, 3, 3), (16,), (32, 16, 1, 1), (10, 37), (5,), (41, 13, 3, 3)]
GROUPS = [[0, 2, 3, 5], [1, 4]]  # the second group: weight_decay 0 (what train.filter_from_weight_decay makes of 1-D tensors)
STEPS = 4
RHO, ETA = 0.5, 0.01  # the callback's defaults, which recipe 49 uses
A_WEIGHTS = [3.0, 1e-2, 0.3, 30.0, 1e-3, 1.0]
CASES = {
    "sgd": dict(cls="SGD", kw=dict(momentum=0.9, weight_decay=1e-4), a=A_WEIGHTS, lr=(1e-3, 2e-2)),
    "adamlw_recipe": dict(cls="AdamLayerwise", kw=dict(betas=(0.9, 0.995), weight_decay=2e-2), a=A_WEIGHTS, lr=(1e-4, 2e-3)),
    "clamp": dict(cls="SGD", kw=dict(momentum=0.9, weight_decay=1e-4), a=[x * 1e-7 for x in A_WEIGHTS], lr=(1e-3, 2e-2)),
}


def params0():
    return [uniform_tensor(s, 0.5, 7301 + i) for i, s in enumerate(SHAPES)]


def targets(k):
    """c_t^k: the targets of step k (0-based), one per tensor"""
    return [uniform_tensor(s, 0.5, 7400 + 10 * k + i) for i, s in enumerate(SHAPES)]


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def lr_ramp(lo, hi):
    return [lo + (hi - lo) * k / (STEPS - 1) for k in range(STEPS)]


class Quadratic(torch.nn.Module):
    """loss(data) = sum_t 0.5 * a_t * |p_t - data_t|^2 over its parameters; records the parameters every forward saw"""

    def __init__(self, params, a):
        super().__init__()
        self.ps = torch.nn.ParameterList(params)
        self.a = [float(x) for x in a]
        self.seen = []

    def forward(self, data):
        self.seen.append(flat(self.ps).clone())
        return sum(0.5 * a * (p - c).pow(2).sum() for a, p, c in zip(self.a, self.ps, data))


def criterion(output, target):
    return output


def install_stubs():
    """the modules the reference's callbacks.py imports, as far as its class definitions need them"""

    class Callback:
        def __init__(self):
            self.state = None

        def set_state(self, state):
            self.state = state

    class Cutmix(Callback):
        pass

    class Mixup(Callback):
        pass

    class Logger:
        def info(self, *a, **k):
            pass

        warning = debug = error = info

    pt = types.ModuleType("pytorch_tools")
    fw = types.ModuleType("pytorch_tools.fit_wrapper")
    clb = types.ModuleType("pytorch_tools.fit_wrapper.callbacks")
    losses = types.ModuleType("pytorch_tools.losses")
    utils = types.ModuleType("pytorch_tools.utils")
    clb.Callback, clb.Cutmix, clb.Mixup, clb.rank_zero_only = Callback, Cutmix, Mixup, (lambda x: x)
    losses.Loss = torch.nn.Module
    pt.fit_wrapper, pt.losses, pt.utils, fw.callbacks = fw, losses, utils, clb
    loguru = types.ModuleType("loguru")
    loguru.logger = Logger()
    sys.modules.update({"pytorch_tools": pt, "pytorch_tools.fit_wrapper": fw, "pytorch_tools.fit_wrapper.callbacks": clb,
                        "pytorch_tools.losses": losses, "pytorch_tools.utils": utils, "loguru": loguru})


def load_reference(root):
    install_stubs()
    mods = {}
    for name in ("callbacks", "optimizers"):
        spec = importlib.util.spec_from_file_location(f"reference_{name}", os.path.join(root, "sota_imagenet", f"{name}.py"))
        mods[name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods[name])
    return mods["callbacks"], mods["optimizers"]


class _NoScaler:
    def unscale_(self, optimizer):
        pass

    def update(self):
        pass

    def scale(self, loss):
        return loss


def run(clb_mod, opt_mod, case, dtype):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params0()]
    model = Quadratic(ps, case["a"])
    lrs = lr_ramp(*case["lr"])
    groups = [{"params": [ps[i] for i in GROUPS[0]]}, {"params": [ps[i] for i in GROUPS[1]], "weight_decay": 0}]
    cls = torch.optim.SGD if case["cls"] == "SGD" else getattr(opt_mod, case["cls"])
    opt = cls(groups, lr=lrs[0], **case["kw"])
    clb = clb_mod.SAMOriginal(rho=RHO, eta=ETA)
    state = types.SimpleNamespace(model=model, optimizer=opt, criterion=criterion, input=None, grad_scaler=_NoScaler())
    clb.state = state
    norms = []
    inner = clb._grad_norm
    clb._grad_norm = lambda: (norms.append(inner()), norms[-1])[1]
    out = dict(norm=[], eps=[], p_pert=[], p_step=[], forwards=[])
    for k in range(STEPS):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        state.input = ([c.to(dtype) for c in targets(k)], None)
        del model.seen[:], norms[:]
        opt.zero_grad()
        criterion(model(state.input[0]), None).backward()
        clb.on_after_backward()
        skipped = not norms
        out["norm"].append(float("nan") if skipped else float(norms[0]))
        out["eps"].append(torch.zeros_like(flat(ps)) if skipped else flat([opt.state[p]["eps_step"] for p in ps]).clone())
        out["p_pert"].append(model.seen[-1].clone())
        out["forwards"].append(len(model.seen))
        opt.step()
        out["p_step"].append(flat(ps).clone())
    out["lrs"] = lrs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "sam_ref_trajectories.npz"))
    a = ap.parse_args()
    clb_mod, opt_mod = load_reference(a.reference)
    torch.set_num_threads(1)
    p0 = flat(params0())
    assert (p0.pow(2) < ETA).any() and (p0.pow(2) > ETA).any()  # both branches of max(p^2, eta) — and of max(|p|, eta): |p| < eta implies p^2 < eta
    assert (p0.abs() < ETA).any() and (p0.abs() > ETA).any()
    offs = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])

    def js(x):
        return np.frombuffer(json.dumps(x).encode(), dtype=np.uint8)

    arrays = {"p0": p0.numpy(), "shapes": js(SHAPES), "groups": js(GROUPS), "steps": js(STEPS)}
    for name, case in CASES.items():
        r64, r32 = run(clb_mod, opt_mod, case, torch.float64), run(clb_mod, opt_mod, case, torch.float32)
        assert r64["forwards"] == r32["forwards"] == [1] + [2] * (STEPS - 1), r64["forwards"]
        assert np.isnan(r64["norm"][0]) and np.isfinite(r64["norm"][1:]).all()
        if name == "clamp":
            assert all(x == 2e-5 for x in r64["norm"][1:]) and all(x == float(np.float32(2e-5)) for x in r32["norm"][1:]), r64["norm"]
        else:
            assert min(r64["norm"][1:]) > 1e-2, r64["norm"]
        arrays[f"{name}/a"], arrays[f"{name}/lrs"] = np.array(case["a"]), np.array(r64["lrs"])
        arrays[f"{name}/hyper"] = js(dict(cls=case["cls"], kw=case["kw"], rho=RHO, eta=ETA))
        arrays[f"{name}/norm"] = np.array(r64["norm"])
        arrays[f"{name}/forwards"] = np.array(r64["forwards"])
        before = [p0.double()] + r64["p_step"][:-1]
        assert all(torch.equal(r64["p_pert"][k], before[k] + r64["eps"][k]) for k in range(STEPS))
        for key in ("eps", "p_pert", "p_step"):
            t64, t32 = torch.stack(r64[key]), torch.stack(r32[key])
            assert torch.isfinite(t64).all() and torch.isfinite(t32).all()
            d = (t32.double() - t64).abs()
            if key != "p_pert":
                arrays[f"{name}/{key}"] = t64.numpy()
            arrays[f"{name}/yard_{key.replace('p_', '')}"] = np.array([[d[k, offs[i]:offs[i + 1]].max().item() for i in range(len(SHAPES))]
                                                                       for k in range(STEPS)])
        eps = arrays[f"{name}/eps"]
        assert not eps[0].any() and all(np.abs(eps[k]).max() > 0 for k in range(1, STEPS))
        print(name, "norm per step:", r64["norm"], " max |eps| per step:", [f"{np.abs(e).max():.3e}" for e in eps])
        print(name, "fp32 run's own distance to fp64 (max per step): eps", [f"{x:.2e}" for x in arrays[f"{name}/yard_eps"].max(1)],
              "params", [f"{x:.2e}" for x in arrays[f"{name}/yard_step"].max(1)])
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20  # float64 trajectories barely compress: 7 arrays of 6132 elements per case, about 1 MB


if __name__ == "__main__":
    main()
