#!/usr/bin/env python3
"""Records tests/golden/optim_ref_trajectories.npz by running the REFERENCE's own MADGRAD and AdaiS (sota_imagenet/optimizers.py of a
reference checkout, loaded by path; none of its text is here) on the CPU: the first reference-generated numerics of this repository.

    python tests/golden/make_optim_golden.py --reference <checkout of the reference>

The problem: five tensors ([16,3,3,3], [16], [32,16,1,1], [10,37], [5]: n % 4 != 0 is covered) in two param groups, the second with
weight_decay 0; six steps, a different lr each (a warm-up ramp), seeded synth.uniform_tensor inputs.  Every case runs once in
float32 and once with everything in float64.  Gradients: unit variance times a per-tensor scale (3 for the weights, 1e-3 for the
1-D tensors) and 8x outliers on every 20th element of the [10,37] tensor, so that AdaiS's beta1 clamp is hit at 0 by some elements, at
1 - eps by others and at neither end by most; the fractions are checked here and recorded.

Arrays of the file (case = madgrad_recipe, madgrad_alt, adais_recipe, adais_alt; i = tensor index; flat = the tensors concatenated):
    p0, grads [6, n]                         inputs (float32)
    <case>/lrs [6], <case>/hyper (json)      constructor arguments, per-group overrides
    <case>/p64 [6, n], <case>/p32 [6, n]     parameters after every step
    <case>/yard [6, 5]                       max |p32 - p64| per step and tensor: the float32 reference run's own error
    <case>/state5/<key> [n]                  per-parameter state of the float64 run after step 5 (rounded to float32), flat
    <case>/state_keys, <case>/state_shapes   (json) key list of state[p] after the last step and the shapes of its tensors
    <case>/mean64 [6], <case>/mean32 [6]     AdaiS: exp_avg_sq_hat_mean of every step;  <case>/clamp [6, 2]: fraction at 0, at 1 - eps
    madgrad cases: <case>/k  the global counter after the last step
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
STEPS = 6
CASES = {
    # the recipes' values (54.r50_madgrad: the class defaults + the base config's weight_decay 1e-4; 50.r50_adais) and one off-default set each
    "madgrad_recipe": dict(cls="MADGRAD", kw=dict(momentum=0.9, weight_decay=1e-4, eps=1e-6), lr=(1e-4, 2e-3)),
    "madgrad_alt": dict(cls="MADGRAD", kw=dict(momentum=0.5, weight_decay=1e-2, eps=1e-4), lr=(1e-3, 2e-2)),
    "adais_recipe": dict(cls="AdaiS", kw=dict(betas=(0.1, 0.99), weight_decay=1e-3, eps=1e-3), lr=(1e-4, 0.1)),
    "adais_alt": dict(cls="AdaiS", kw=dict(betas=(0.3, 0.9), weight_decay=5e-2, eps=1e-2, ema_norm_init=1e-2), lr=(1e-3, 0.05)),
}


def problem():
    p0 = [uniform_tensor(s, 0.5, 7001 + i) for i, s in enumerate(SHAPES)]
    grads = []
    for k in range(STEPS):
        gs = []
        for i, s in enumerate(SHAPES):
            g = uniform_tensor(s, 3.0 ** 0.5, 7100 + 10 * k + i) * (1e-3 if len(s) == 1 else 3.0)
            if s == (10, 37):
                g.view(-1)[::20] *= 8.0
            gs.append(g)
        grads.append(gs)
    return p0, grads


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts])


def lr_ramp(lo, hi):
    return [lo + (hi - lo) * k / (STEPS - 1) for k in range(STEPS)]


def run(mod, case, p0, grads, dtype):
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in p0]
    lrs = lr_ramp(*case["lr"])
    groups = [{"params": [ps[i] for i in GROUPS[0]]}, {"params": [ps[i] for i in GROUPS[1]], "weight_decay": 0}]
    opt = getattr(mod, case["cls"])(groups, lr=lrs[0], **case["kw"])
    out = dict(p=[], mean=[], clamp=[], state5=None)
    adais = case["cls"] == "AdaiS"
    for k in range(STEPS):
        for g in opt.param_groups:
            g["lr"] = lrs[k]
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(dtype).clone()
        opt.step()
        out["p"].append(flat(ps).clone())
        if adais:
            # the statistic the step just used, from the state it left: mean over all elements of exp_avg_sq / (1 - beta2^step)
            hats = [opt.state[p]["exp_avg_sq"] / (1 - g["betas"][1] ** opt.state[p]["step"]) for g in opt.param_groups for p in g["params"]]
            mean = sum(h.sum() for h in hats) / sum(h.numel() for h in hats)
            out["mean"].append(float(mean))
            at0 = at1 = 0
            for g in opt.param_groups:
                for p in g["params"]:
                    h = opt.state[p]["exp_avg_sq"] / (1 - g["betas"][1] ** opt.state[p]["step"])
                    raw = 1.0 - (h / mean) * g["betas"][0]
                    at0 += int((raw <= 0).sum())
                    at1 += int((raw >= 1 - g["eps"]).sum())
            n = sum(p.numel() for p in ps)
            out["clamp"].append((at0 / n, at1 / n))
        if k == STEPS - 2:
            keys = [key for key, v in opt.state[ps[0]].items() if torch.is_tensor(v)]
            out["state5"] = {key: flat([opt.state[p][key] for p in ps]).clone() for key in keys}
    st = opt.state[ps[0]]
    out["state_keys"] = sorted(st.keys())
    out["state_shapes"] = {key: [list(opt.state[p][key].shape) for p in ps] for key, v in st.items() if torch.is_tensor(v)}
    out["k"] = int(opt.state["k"].item()) if "k" in opt.state else None
    out["lrs"] = lrs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "optim_ref_trajectories.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_optimizers", os.path.join(a.reference, "sota_imagenet", "optimizers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.set_num_threads(1)
    p0, grads = problem()
    offs = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])
    arrays = {"p0": flat(p0).numpy(), "grads": torch.stack([flat(g) for g in grads]).numpy(),
              "shapes": np.frombuffer(json.dumps(SHAPES).encode(), dtype=np.uint8), "groups": np.frombuffer(json.dumps(GROUPS).encode(), dtype=np.uint8)}
    for name, case in CASES.items():
        r64, r32 = run(mod, case, p0, grads, torch.float64), run(mod, case, p0, grads, torch.float32)
        p64, p32 = torch.stack(r64["p"]), torch.stack(r32["p"])
        assert torch.isfinite(p64).all() and torch.isfinite(p32).all()
        d = (p32.double() - p64).abs()
        arrays[f"{name}/p64"], arrays[f"{name}/p32"] = p64.numpy(), p32.numpy()
        arrays[f"{name}/yard"] = np.array([[d[k, offs[i]:offs[i + 1]].max().item() for i in range(len(SHAPES))] for k in range(STEPS)])
        arrays[f"{name}/lrs"] = np.array(r64["lrs"])
        arrays[f"{name}/hyper"] = np.frombuffer(json.dumps(dict(cls=case["cls"], **case["kw"])).encode(), dtype=np.uint8)
        for key, t in r64["state5"].items():
            arrays[f"{name}/state5/{key}"] = t.float().numpy()
        arrays[f"{name}/state_keys"] = np.frombuffer(json.dumps(r64["state_keys"]).encode(), dtype=np.uint8)
        arrays[f"{name}/state_shapes"] = np.frombuffer(json.dumps(r64["state_shapes"]).encode(), dtype=np.uint8)
        assert r64["state_keys"] == r32["state_keys"]
        if case["cls"] == "AdaiS":
            arrays[f"{name}/mean64"], arrays[f"{name}/mean32"] = np.array(r64["mean"]), np.array(r32["mean"], dtype=np.float64)
            clamp = np.array(r64["clamp"])
            arrays[f"{name}/clamp"] = clamp
            # both ends of the clamp are exercised at every step, and most elements are at neither
            assert (clamp[:, 0] > 0.005).all() and (clamp[:, 1] > 0.005).all() and (clamp.sum(1) < 0.5).all(), clamp
            print(name, "fraction at 0 / at 1 - eps per step:", np.round(clamp, 4).tolist())
        else:
            arrays[f"{name}/k"] = np.array([r64["k"]], dtype=np.int64)
        print(name, "fp32 run's own distance to fp64 (max per step):", [f"{x:.2e}" for x in arrays[f"{name}/yard"].max(1)])
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
