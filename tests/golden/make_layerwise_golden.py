#!/usr/bin/env python3
"""Records tests/golden/layerwise_ref_trajectories.npz by running the REFERENCE's own MyNovograd, NovogradApex, AdamLayerwise and MyAdai
(sota_imagenet/optimizers.py of a reference checkout, loaded by path; none of its text is here) on the CPU with one thread.

    python tests/golden/make_layerwise_golden.py --reference <checkout of the reference>

The problem of make_optim_golden.py: five tensors ([16,3,3,3], [16], [32,16,1,1], [10,37], [5]) in two param groups, the second with
weight_decay 0; six steps on an lr ramp, seeded synth.uniform_tensor inputs, every case once in float32 and once in float64.  Here each
tensor has its own gradient scale (3, 1e-3, 3e-2, 0.3, 1e-3), because these optimizers act on one statistic per tensor: MyAdai's
beta1 then lands at the 0 clamp for tensor 0 and strictly between the clamps for the others with the recipe's values (which cannot reach
1 - eps: vt / mean >= beta2), and at 0, between and at 1 - eps with the second MyAdai case.  The regimes are asserted here.

Arrays of the file (i = tensor index; flat = the tensors concatenated):
    p0 [n], shapes, groups (json)             inputs (float32); the gradients are not stored: problem() of this file rebuilds them from
                                              their seeds (synth.uniform_tensor is a counter hash, the same on every machine)
    <case>/lrs [6], <case>/hyper (json)       constructor arguments
    <case>/p64 [6, n]                         parameters of the float64 run after every step
    <case>/yard [6, 5]                        max |p32 - p64| per step and tensor: the float32 reference run's own error (p32 is not stored)
    <case>/state5/<key> [n]                   tensor state of the float64 run after step 5 (rounded to float32), flat, dense as the reference keeps it
    <case>/state_keys, <case>/state_shapes    (json) key list of state[p] after the last step and the shapes of its tensors
    MyAdai cases: <case>/beta1 [6, 5]         beta1 of every step and tensor (float64 run), <case>/v0 [5] the floats in state[p]["exp_avg_sq"]
    nov_recipe: <case>/below_wd_eps [6]       share of elements with |p| < wd_eps after every step
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from sota_imagenet_amd.synth import uniform_tensor  # noqa: E402

SHAPES = [(16, 3, 3, 3), (16,), (32, 16, 1, 1), (10, 37), (5,)]
GROUPS = [[0, 2, 3], [1, 4]]  # the second group: weight_decay 0 (what train.filter_from_weight_decay makes of 1-D tensors)
GRAD_SCALES = [3.0, 1e-3, 3e-2, 0.3, 1e-3]
STEPS = 6
CASES = {
    # the four recipes' values (46.r50_nov, 47.r50_my-nov, 49.r50_nov-adam, 55.r50_adai_2) and one off-default set for three classes
    "nov_recipe": dict(cls="NovogradApex", kw=dict(betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01), lr=(1e-3, 5e-2)),
    "mynov_recipe": dict(cls="MyNovograd", kw=dict(betas=(0.9, 0.99), weight_decay=0.002), lr=(1e-3, 5e-2)),
    "adamlw_recipe": dict(cls="AdamLayerwise", kw=dict(betas=(0.9, 0.995), weight_decay=2e-2), lr=(1e-4, 5e-3)),
    "myadai_recipe": dict(cls="MyAdai", kw=dict(betas=(0.1, 0.99), weight_decay=3e-5, sgd_mom=True, stable_wd=True), lr=(1e-4, 1e-2)),
    "adamlw_alt": dict(cls="AdamLayerwise", kw=dict(betas=(0.8, 0.9), eps=1e-4, weight_decay=2e-2, ema_norm_init=1e-2, stable_wd=True), lr=(1e-4, 5e-3)),
    "nov_alt": dict(cls="NovogradApex", kw=dict(betas=(0.95, 0), weight_decay=1e-2), lr=(1e-3, 5e-2)),
    "myadai_alt": dict(cls="MyAdai", kw=dict(betas=(0.05, 0.9), eps=0.1, weight_decay=1e-3, sqrt_mom=True), lr=(1e-4, 1e-2)),
}


def problem():
    p0 = [uniform_tensor(s, 0.5, 7001 + i) for i, s in enumerate(SHAPES)]
    grads = [[uniform_tensor(s, 3.0 ** 0.5, 7100 + 10 * k + i) * GRAD_SCALES[i] for i, s in enumerate(SHAPES)] for k in range(STEPS)]
    return p0, grads


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def lr_ramp(lo, hi):
    return [lo + (hi - lo) * k / (STEPS - 1) for k in range(STEPS)]


def adai_beta1(opt, ps, mean):
    """beta1 of the step that is about to run, per tensor, from the state as it stands and the gradients (the class keeps no record of it)"""
    out = []
    for g in opt.param_groups:
        b0, b2 = g["betas"]
        for p in g["params"]:
            v0 = opt.state[p]["exp_avg_sq"] if p in opt.state else opt.ema_norm_init
            vt = v0 * b2 + p.grad.pow(2).mean().item() * (1 - b2)
            r = vt / mean
            out.append((id(p), float(np.clip(1 - (np.sqrt(r) if opt.sqrt_mom else r) * b0, 0, 1 - g["eps"]))))
    d = dict(out)
    return [d[id(p)] for p in ps]


def run(mod, case, p0, grads, dtype):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]
    lrs = lr_ramp(*case["lr"])
    groups = [{"params": [ps[i] for i in GROUPS[0]]}, {"params": [ps[i] for i in GROUPS[1]], "weight_decay": 0}]
    opt = getattr(mod, case["cls"])(groups, lr=lrs[0], **case["kw"])
    out = dict(p=[], beta1=[], below=[], state5=None)
    for k in range(STEPS):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(dtype).clone()
        if case["cls"] == "MyAdai":
            mean = opt.ema_norm_init if len(opt.state) == 0 else sum(v["exp_avg_sq"] for v in opt.state.values()) / len(opt.state)
            out["beta1"].append(adai_beta1(opt, ps, mean))
        opt.step()
        out["p"].append(flat(ps).clone())
        if case["kw"].get("wd_eps") is not None:
            out["below"].append(float((flat(ps).abs() < case["kw"]["wd_eps"]).double().mean()))
        if k == STEPS - 2:
            keys = [key for key, v in opt.state[ps[0]].items() if torch.is_tensor(v)]
            out["state5"] = {key: flat([opt.state[p][key] for p in ps]).clone() for key in keys}
    st = opt.state[ps[0]]
    out["state_keys"] = sorted(st.keys())
    out["state_shapes"] = {key: [list(opt.state[p][key].shape) for p in ps] for key, v in st.items() if torch.is_tensor(v)}
    if case["cls"] == "MyAdai":
        out["v0"] = [float(opt.state[p]["exp_avg_sq"]) for p in ps]
    out["lrs"] = lrs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "layerwise_ref_trajectories.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_optimizers", os.path.join(a.reference, "sota_imagenet", "optimizers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(1)
    p0, grads = problem()
    offs = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])
    arrays = {"p0": flat(p0).numpy(),
              "shapes": np.frombuffer(json.dumps(SHAPES).encode(), dtype=np.uint8), "groups": np.frombuffer(json.dumps(GROUPS).encode(), dtype=np.uint8)}
    for name, case in CASES.items():
        r64, r32 = run(mod, case, p0, grads, torch.float64), run(mod, case, p0, grads, torch.float32)
        p64, p32 = torch.stack(r64["p"]), torch.stack(r32["p"])
        assert torch.isfinite(p64).all() and torch.isfinite(p32).all()
        d = (p32.double() - p64).abs()
        arrays[f"{name}/p64"] = p64.numpy()
        arrays[f"{name}/yard"] = np.array([[d[k, offs[i]:offs[i + 1]].max().item() for i in range(len(SHAPES))] for k in range(STEPS)])
        arrays[f"{name}/lrs"] = np.array(r64["lrs"])
        arrays[f"{name}/hyper"] = np.frombuffer(json.dumps(dict(cls=case["cls"], **case["kw"])).encode(), dtype=np.uint8)
        for key, t in r64["state5"].items():
            arrays[f"{name}/state5/{key}"] = t.float().numpy()
        arrays[f"{name}/state_keys"] = np.frombuffer(json.dumps(r64["state_keys"]).encode(), dtype=np.uint8)
        arrays[f"{name}/state_shapes"] = np.frombuffer(json.dumps(r64["state_shapes"]).encode(), dtype=np.uint8)
        assert r64["state_keys"] == r32["state_keys"]
        if case["cls"] == "MyAdai":
            b1 = np.array(r64["beta1"])
            arrays[f"{name}/beta1"], arrays[f"{name}/v0"] = b1, np.array(r64["v0"])
            hi = 1 - case["kw"].get("eps", 1e-3)
            at0, at1 = b1 == 0.0, b1 == hi
            between = ~at0 & ~at1
            print(name, "beta1 per step and tensor:", np.round(b1, 4).tolist())
            if name == "myadai_recipe":
                # tensor 0 at the 0 clamp, the others strictly between; the upper clamp is out of reach (vt / mean >= beta2)
                assert at0[:, 0].all() and between[:, 1:].all() and not at1.any(), b1
            else:
                assert (at0.sum(1) >= 1).all() and (between.sum(1) >= 1).all() and (at1.sum(1) >= 2).all(), b1
        if r64["below"]:
            arrays[f"{name}/below_wd_eps"] = np.array(r64["below"])
            assert min(r64["below"]) > 0, r64["below"]
            print(name, "share of |p| < wd_eps per step:", np.round(r64["below"], 4).tolist())
        print(name, "fp32 run's own distance to fp64 (max per step):", [f"{x:.2e}" for x in arrays[f"{name}/yard"].max(1)])
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 500_000


if __name__ == "__main__":
    main()
