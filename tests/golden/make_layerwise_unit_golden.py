#!/usr/bin/env python3
"""Records tests/golden/layerwise_unit_ref_trajectories.npz by running the REFERENCE's own MyNovograd and NovogradApex with unitwise_norm=True
(sota_imagenet/optimizers.py of a reference checkout, loaded by path; none of its text is here) on the CPU with one thread.

    python tests/golden/make_layerwise_unit_golden.py --reference <checkout of the reference>

The problem of make_layerwise_golden.py (imported from there): the same five tensors, groups, seeds, per-tensor gradient scales and six steps.
The cases: the values of recipe configs/hydra_exp/48.r50_my-nov-unit.yaml, NovogradApex with recipe 46's values and wd_eps, NovogradApex off
its defaults.  Asserted here: the float64 second moment holds 16 distinct values over tensor 0's 16 units and one value per 1-D tensor, and
every unit-wise trajectory differs from the layer-wise one of the same class and values by more than 1e-3.

Arrays of the file, in the layout of layerwise_ref_trajectories.npz (i = tensor index; flat = the tensors concatenated):
    p0 [n], shapes, groups (json)             inputs (float32); the gradients are rebuilt from their seeds by make_layerwise_golden.problem()
    <case>/lrs [6], <case>/hyper (json)       constructor arguments
    <case>/p64 [6, n]                         parameters of the float64 run after every step
    <case>/yard [6, 5]                        max |p32 - p64| per step and tensor: the float32 reference run's own error
    <case>/state5/<key> [n]                   tensor state of the float64 run after step 5 (rounded to float32), flat and dense
    <case>/state_keys, <case>/state_shapes    (json) key list of state[p] after the last step and the shapes of its tensors
    <case>/v32_5 [n]                          the second moment of the FLOAT32 run after step 5, flat and dense
    <case>/spread [2, 5]                      largest relative spread (max - min) / max inside a unit after step 5, per tensor: float64 run, float32 run
    <case>/vs_layerwise                       max |p64 - p64 of the layer-wise run| after step 6
"""
import argparse
import importlib.util
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


base = _load("make_layerwise_golden", os.path.join(HERE, "make_layerwise_golden.py"))
SHAPES, GROUPS, STEPS = base.SHAPES, base.GROUPS, base.STEPS
V_KEY = {"MyNovograd": "ema_norm", "NovogradApex": "exp_avg_sq"}
CASES = {
    "mynov_unit_recipe": dict(cls="MyNovograd", kw=dict(betas=(0.9, 0.99), weight_decay=2e-4, unitwise_norm=True), lr=(1e-4, 5e-2)),
    "nov_unit": dict(cls="NovogradApex", kw=dict(betas=(0.9, 0.99), weight_decay=2e-3, wd_eps=0.01, unitwise_norm=True), lr=(1e-3, 5e-2)),
    "nov_unit_alt": dict(cls="NovogradApex", kw=dict(betas=(0.95, 0), weight_decay=1e-2, unitwise_norm=True), lr=(1e-3, 5e-2)),
}


def unit_rows(t, shape):
    """[slots, unit_len]: a flat tensor of `shape` with one row per slot"""
    return t.reshape(shape[0] if len(shape) > 1 else 1, -1)


def spread(flat, offs):
    out = []
    for i, s in enumerate(SHAPES):
        r = unit_rows(flat[offs[i]:offs[i + 1]].double(), s)
        out.append(((r.max(1).values - r.min(1).values) / r.abs().max(1).values).max().item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "layerwise_unit_ref_trajectories.npz"))
    a = ap.parse_args()
    mod = _load("reference_optimizers", os.path.join(a.reference, "sota_imagenet", "optimizers.py"))
    torch.set_num_threads(1)
    p0, grads = base.problem()
    offs = np.cumsum([0] + [int(np.prod(s)) for s in SHAPES])
    js = lambda x: np.frombuffer(json.dumps(x).encode(), dtype=np.uint8)  # noqa: E731
    arrays = {"p0": base.flat(p0).numpy(), "shapes": js(SHAPES), "groups": js(GROUPS)}
    for name, case in CASES.items():
        r64, r32 = base.run(mod, case, p0, grads, torch.float64), base.run(mod, case, p0, grads, torch.float32)
        lw = base.run(mod, dict(case, kw=dict(case["kw"], unitwise_norm=False)), p0, grads, torch.float64)
        p64, p32 = torch.stack(r64["p"]), torch.stack(r32["p"])
        assert torch.isfinite(p64).all() and torch.isfinite(p32).all()
        d = (p32.double() - p64).abs()
        arrays[f"{name}/p64"] = p64.numpy()
        arrays[f"{name}/yard"] = np.array([[d[k, offs[i]:offs[i + 1]].max().item() for i in range(len(SHAPES))] for k in range(STEPS)])
        arrays[f"{name}/lrs"] = np.array(r64["lrs"])
        arrays[f"{name}/hyper"] = js(dict(cls=case["cls"], **case["kw"]))
        for key, t in r64["state5"].items():
            arrays[f"{name}/state5/{key}"] = t.float().numpy()
        arrays[f"{name}/state_keys"], arrays[f"{name}/state_shapes"] = js(r64["state_keys"]), js(r64["state_shapes"])
        assert r64["state_keys"] == r32["state_keys"]
        vk = V_KEY[case["cls"]]
        v64, v32 = r64["state5"][vk], r32["state5"][vk]
        arrays[f"{name}/v32_5"] = v32.numpy()
        arrays[f"{name}/spread"] = np.array([spread(v64, offs), spread(v32, offs)])
        assert len(torch.unique(unit_rows(v64[offs[0]:offs[1]], SHAPES[0])[:, 0])) == 16           # one value per unit of tensor 0
        assert all(len(torch.unique(v64[offs[i]:offs[i + 1]])) == 1 for i in (1, 4))                # one value per 1-D tensor
        vs = (p64[-1] - lw["p"][-1]).abs().max().item()
        arrays[f"{name}/vs_layerwise"] = np.array(vs)
        assert vs > 1e-3, vs
        print(name, "fp32 run's own distance to fp64 (max per step):", [f"{x:.2e}" for x in arrays[f"{name}/yard"].max(1)])
        print(name, "spread inside a unit (fp64, fp32):", arrays[f"{name}/spread"].max(1).tolist(), " vs the layer-wise trajectory:", f"{vs:.3g}")
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) < 500_000


if __name__ == "__main__":
    main()
