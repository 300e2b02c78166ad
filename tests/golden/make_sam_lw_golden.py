#!/usr/bin/env python3
"""Records tests/golden/sam_lw_ref_trajectories.npz by running the REFERENCE's own SAM callback (sota_imagenet/callbacks.py:339-420 of a reference
checkout, loaded by path through make_sam_golden.load_reference; none of its text is here) on the CPU with one thread, once in float64 and once in
float32.

    python tests/golden/make_sam_lw_golden.py --reference <checkout of the reference>

The problem is make_sam_golden.py's with these changes: [41,13,3,3] gives way to [37,113] (4181 elements: two 4096-element work items, rows of odd
length, row 36 straddles the item boundary); tensor 4 ([5]) starts at 1e-4 of its values with a = 1e-9, so both norm floors apply to it; tensor
2 has a = 1e-7, so the gradient norm sits on its floor for the tensor and for every one of its rows; row ROW3 of tensor 3 starts at 1e-5 of
its values, so the weight norm sits on its floor for that unit only.  Asserted: no floor, the gradient floor only and both floors each occur
in at least one slot in every step of every case; the weight floor only occurs unit-wise in the first step — the optimizers' updates (SGD:
lr * a_3 * |p - c|, about 1e-2 per element) then take the row off the floor.  Layer-wise no whole tensor of this problem has ||p|| < 1e-3
with ||g|| >= 1e-5; the native kernels' test builds that case from values of its own.

Three steps on an lr ramp, every one perturbed (SAM has no first-step skip).  Cases: layer_sgd and unit_sgd (torch.optim.SGD, momentum 0.9,
rho 0.01), unit_adamlw (the reference's own AdamLayerwise with recipe 49's values, rho 0.001).

eps is a local of the reference's on_after_backward: it is taken from the list the callback hands to torch._foreach_add_, which is wrapped for the
length of that call.  The norms are those of the parameters and gradients the callback was given, through the reference's own unitwise_norm.

Arrays of the file (i = tensor index; flat = the tensors concatenated in index order; slots numbered tensor by tensor in index order):
    p0 [n], shapes, groups, steps (json)      inputs (float32); targets() rebuilds the targets from their seeds
    <case>/a [6], <case>/lrs [3], <case>/hyper (json: cls, kw, rho, unitwise)
    <case>/eps [3, n]                         eps of the float64 run
    <case>/p_step [3, n]                      parameters of the float64 run after the optimizer step (the parameters the second forward saw are,
                                              bit for bit, the parameters before the step plus eps — asserted here)
    <case>/gn, <case>/wn [3, slots]           the clamped norms of the float64 run
    <case>/forwards [3]                       forwards the step made: 2, 2, 2
    <case>/yard_eps, yard_pert, yard_step [3, 6]   max |float32 run - float64 run| per step and tensor: the reference's own float32 error
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_sam_golden import Quadratic, _NoScaler, criterion, load_reference  # noqa: E402
from make_sam_golden import flat, uniform_tensor  # noqa: E402

SHAPES = [(16, 3, 3, 3), (16,), (32, 16, 1, 1), (10, 37), (5,), (37, 113)]
GROUPS = [[0, 2, 3, 5], [1, 4]]  # the second group: weight_decay 0
STEPS = 3
ROW3 = 4  # the row of tensor 3 that starts small
A_WEIGHTS = [3.0, 1e-2, 1e-7, 30.0, 1e-9, 1.0]
GN_FLOOR, WN_FLOOR = 1e-5, 1e-3
_SGD = dict(cls="SGD", kw=dict(momentum=0.9, weight_decay=1e-4), lr=(1e-3, 2e-2), rho=0.01)
CASES = {
    "layer_sgd": dict(_SGD, unitwise=False),
    "unit_sgd": dict(_SGD, unitwise=True),
    "unit_adamlw": dict(cls="AdamLayerwise", kw=dict(betas=(0.9, 0.995), weight_decay=2e-2), lr=(1e-4, 2e-3), rho=0.001, unitwise=True),
}


def params0():
    ps = [uniform_tensor(s, 0.5, 7301 + i) for i, s in enumerate(SHAPES)]
    ps[4] = ps[4] * 1e-4
    ps[3][ROW3] = ps[3][ROW3] * 1e-5
    return ps


def targets(k):
    """c_t^k: the targets of step k (0-based), one per tensor"""
    return [uniform_tensor(s, 0.5, 7400 + 10 * k + i) for i, s in enumerate(SHAPES)]


def lr_ramp(lo, hi):
    return [lo + (hi - lo) * k / (STEPS - 1) for k in range(STEPS)]


def slot_counts(unitwise):
    return [s[0] if unitwise and len(s) > 1 else 1 for s in SHAPES]


def run(clb_mod, opt_mod, case, dtype):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params0()]
    model = Quadratic(ps, A_WEIGHTS)
    lrs = lr_ramp(*case["lr"])
    groups = [{"params": [ps[i] for i in GROUPS[0]]}, {"params": [ps[i] for i in GROUPS[1]], "weight_decay": 0}]
    cls = torch.optim.SGD if case["cls"] == "SGD" else getattr(opt_mod, case["cls"])
    opt = cls(groups, lr=lrs[0], **case["kw"])
    clb = clb_mod.SAM(unitwise=case["unitwise"], rho=case["rho"])
    assert (clb.eps, clb.eps_2) == (GN_FLOOR, WN_FLOOR)
    clb.state = types.SimpleNamespace(model=model, optimizer=opt, criterion=criterion, input=None, grad_scaler=_NoScaler())
    order = [i for idx in GROUPS for i in idx]  # the order of the callback's lists

    def norm(x):
        return (clb_mod.unitwise_norm(x) if case["unitwise"] else x.norm(2)).reshape(-1)

    out = dict(eps=[], p_pert=[], p_step=[], forwards=[], gn=[], wn=[], lrs=lrs)
    for k in range(STEPS):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        clb.state.input = ([c.to(dtype) for c in targets(k)], None)
        del model.seen[:]
        opt.zero_grad()
        criterion(model(clb.state.input[0]), None).backward()
        out["gn"].append(torch.cat([norm(p.grad.detach()).clamp_min(GN_FLOOR) for p in ps]).clone())
        out["wn"].append(torch.cat([norm(p.detach()).clamp_min(WN_FLOOR) for p in ps]).clone())
        taken, inner = [], torch._foreach_add_
        torch._foreach_add_ = lambda a, b: (taken.append([t.clone() for t in b]), inner(a, b))[1]
        try:
            clb.on_after_backward()
        finally:
            torch._foreach_add_ = inner
        assert len(taken) == 1 and len(taken[0]) == len(ps)
        eps = [None] * len(ps)
        for i, e in zip(order, taken[0]):
            eps[i] = e
        out["eps"].append(flat(eps).clone())
        out["p_pert"].append(model.seen[-1].clone())
        out["forwards"].append(len(model.seen))
        opt.step()
        out["p_step"].append(flat(ps).clone())
    return out


def main():
    import json

    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "sam_lw_ref_trajectories.npz"))
    a = ap.parse_args()
    clb_mod, opt_mod = load_reference(a.reference)
    torch.set_num_threads(1)
    p0 = flat(params0())
    offs = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])

    def js(x):
        return np.frombuffer(json.dumps(x).encode(), dtype=np.uint8)

    arrays = {"p0": p0.numpy(), "shapes": js(SHAPES), "groups": js(GROUPS), "steps": js(STEPS)}
    for name, case in CASES.items():
        r64, r32 = run(clb_mod, opt_mod, case, torch.float64), run(clb_mod, opt_mod, case, torch.float32)
        assert r64["forwards"] == r32["forwards"] == [2] * STEPS, r64["forwards"]
        counts = slot_counts(case["unitwise"])
        gn, wn = torch.stack(r64["gn"]), torch.stack(r64["wn"])
        assert gn.shape == wn.shape == (STEPS, sum(counts))
        for k in range(STEPS):
            g_fl, w_fl = gn[k] == GN_FLOOR, wn[k] == WN_FLOOR
            seen = {(bool(x), bool(y)) for x, y in zip(g_fl, w_fl)}
            want = {(False, False), (True, False), (True, True)} | ({(False, True)} if case["unitwise"] and k == 0 else set())
            assert seen >= want, (name, k, seen)
        s4, s2 = sum(counts[:4]), sum(counts[:2])
        assert (gn[:, s4] == GN_FLOOR).all() and (wn[:, s4] == WN_FLOOR).all()           # tensor 4: both
        assert (gn[:, s2:s2 + counts[2]] == GN_FLOOR).all()                              # tensor 2: the gradient floor, every row
        if case["unitwise"]:
            s3 = sum(counts[:3])
            assert [int(i) for i in (wn[0, s3:s3 + counts[3]] == WN_FLOOR).nonzero()] == [ROW3]  # tensor 3: the weight floor, one row
        arrays[f"{name}/a"], arrays[f"{name}/lrs"] = np.array(A_WEIGHTS), np.array(r64["lrs"])
        arrays[f"{name}/hyper"] = js(dict(cls=case["cls"], kw=case["kw"], rho=case["rho"], unitwise=case["unitwise"]))
        arrays[f"{name}/gn"], arrays[f"{name}/wn"] = gn.numpy(), wn.numpy()
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
        assert all(np.abs(eps[k, offs[i]:offs[i + 1]]).max() > 0 for k in range(STEPS) for i in range(len(SHAPES)))
        print(name, "max |eps| per step:", [f"{np.abs(e).max():.3e}" for e in eps])
        print(name, "fp32 run's own distance to fp64 (max per step): eps", [f"{x:.2e}" for x in arrays[f"{name}/yard_eps"].max(1)],
              "params", [f"{x:.2e}" for x in arrays[f"{name}/yard_step"].max(1)])
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 1 << 20


if __name__ == "__main__":
    main()
