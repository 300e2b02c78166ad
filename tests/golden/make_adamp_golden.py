#!/usr/bin/env python3
"""Records tests/golden/adamp_ref_trajectories.npz from a torch restatement of adamp.AdamP.step, on the CPU with one thread.

    python tests/golden/make_adamp_golden.py

PROVENANCE.  The `adamp` package is neither part of the reference tree nor available where this was written.  `adamp_tensor_step` below is the
published adamp.AdamP.step (package 0.3.0) written down from memory of the public package — the specification this project's AdamP is built to
(include/mi355rn.h).  The fixture is therefore UNPINNED against the package itself: it pins the project against this
restatement, in float64, with the restatement's own float32 run as the yardstick.

The problem: 4 steps on eight tensors — (8,3,7,7) whose units of 147 elements start at every alignment, (16,8,3,3), (1,4100) with dim 0 of 1 and a
unit longer than one 4096-element work item, (6,2) with a unit shorter than a float4, (64,), (1,40), (10,16), (5,).  The gradients of step k are
built from the float32 run's own parameters at step k so that the wanted decision holds with margin:
    channel mode  (8,3,7,7), (1,4100), (1,40): every row of g orthogonalised to the row of p
    layer mode    (16,8,3,3), (10,16):         g_row = a_row * p_row with sum a_row * ||p_row||^2 = 0 — rows aligned, the layer orthogonal
    no projection (6,2):                       noise plus a component along p
    1-D tensors                                plain noise
Cases: adamp_recipe51 (the defaults with weight_decay 1e-2 of configs/hydra_exp/51.r50_adamp.yaml, one group) and adamp_alt (nesterov, betas
(0.8, 0.95), eps 1e-5, delta 0.2, wd_ratio 0.5; the 1-D tensors in a group of their own with weight_decay 0, the others with 1e-3), both under
an lr ramp.

Asserted before the file is written — conditions on the inputs, not measurements:
    every decision's max cos / threshold is <= 0.5 or >= 2 in the float32 and in the float64 run, and the modes of the two runs agree;
    every projected tensor lies >= 100 x its yard away from the same run with the projection switched off;
    the file is <= 1.0 MB.

Arrays (i = tensor index; flat = the tensors concatenated in the order above):
    shapes, <case>/groups, <case>/wds, <case>/hyper (json)
    <case>/p0 [n], <case>/grads [4, n], <case>/lrs [4]     inputs (float32)
    <case>/p64 [4, n]                                      parameters of the float64 run after every step
    <case>/yard [4, 8]                                     max |p32 - p64| per step and tensor: the float32 run's own error
    <case>/modes [4, 8]                                    0 no projection, 1 per output unit, 2 per whole tensor
    <case>/margins [2, 4, 8, 2]                            max cos / threshold of the (rows, layer) decisions, float32 and float64 run; NaN where
                                                           a decision was not taken (1-D tensors; the layer after a projection of the rows)
    <case>/effect [4, 8]                                   max |p64 - p64 of the run without projection|
    <case>/state4/exp_avg, exp_avg_sq [n]                  state of the float32 run after the last step
"""
import json
import math
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "adamp_ref_trajectories.npz")
SHAPES = [(8, 3, 7, 7), (16, 8, 3, 3), (1, 4100), (6, 2), (64,), (1, 40), (10, 16), (5,)]
WANT = ["channel", "layer", "channel", "none", "1d", "channel", "layer", "1d"]
STEPS = 4
DEFAULTS = dict(betas=(0.9, 0.999), eps=1e-8, delta=0.1, wd_ratio=0.1, nesterov=False)
CASES = {
    "adamp_recipe51": dict(hyper={}, groups=[list(range(8))], wds=[1e-2], lrs=[2.5e-4, 5e-4, 7.5e-4, 1e-3], seed=51),
    "adamp_alt": dict(hyper=dict(nesterov=True, betas=(0.8, 0.95), eps=1e-5, delta=0.2, wd_ratio=0.5), groups=[[0, 1, 2, 3, 5, 6], [4, 7]],
                      wds=[1e-3, 0.0], lrs=[1e-3, 2e-3, 3e-3, 4e-3], seed=52),
}


def rows_of(x):
    return x.reshape(x.shape[0], -1)


def layer_of(x):
    return x.reshape(1, -1)


def cosine(x, y, eps):
    """|cosine_similarity(x, y, dim=1, eps)|: sum(x*y) / (max(||x||, eps) * max(||y||, eps)) per row"""
    return ((x * y).sum(1) / (x.norm(dim=1).clamp_min(eps) * y.norm(dim=1).clamp_min(eps))).abs()


def adamp_tensor_step(p, g, st, h, lr, wd, project=True):
    """one step of one tensor in the dtype of p.  st: {step, exp_avg, exp_avg_sq}, advanced in place; h: betas, eps, delta, wd_ratio, nesterov.
    Returns (new p, mode, [max cos / threshold of the rows decision, of the layer decision])"""
    b1, b2 = h["betas"]
    eps = h["eps"]
    st["step"] += 1
    bc1, bc2 = 1 - b1 ** st["step"], 1 - b2 ** st["step"]
    m = st["exp_avg"] = b1 * st["exp_avg"] + (1 - b1) * g
    v = st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1 - b2) * g * g
    den = v.sqrt() / math.sqrt(bc2) + eps
    u = (b1 * m + (1 - b1) * g) / den if h["nesterov"] else m / den
    ratio, mode, margins = 1.0, 0, [math.nan, math.nan]
    if p.dim() > 1:
        for k, view in enumerate((rows_of, layer_of)):
            x, y = view(g), view(p)
            cos = cosine(x, y, eps)
            thr = h["delta"] / math.sqrt(y.shape[1])
            margins[k] = cos.max().item() / thr
            if project and cos.max().item() < thr:
                pn = y / (y.norm(dim=1, keepdim=True) + eps)
                uv = view(u)
                u = (uv - pn * (pn * uv).sum(1, keepdim=True)).reshape(p.shape)
                ratio, mode = h["wd_ratio"], k + 1
                break
    if wd > 0:
        p = p * (1 - lr * wd * ratio)
    p = p + (-lr / bc1) * u
    return p, mode, margins


def make_grad(kind, p, gen):
    """the gradient of one tensor, built in float64 from the float32 parameter p so that the wanted decision holds with margin"""
    p = p.double()
    noise = torch.randn(p.shape, generator=gen, dtype=torch.float64)
    if kind == "channel":
        r, y = rows_of(noise), rows_of(p)
        g = (r - y * ((r * y).sum(1, keepdim=True) / (y * y).sum(1, keepdim=True))).reshape(p.shape)
    elif kind == "layer":
        y = rows_of(p)
        n2 = (y * y).sum(1)
        a = torch.randn(y.shape[0], generator=gen, dtype=torch.float64)
        a = a - n2 * ((a * n2).sum() / (n2 * n2).sum())
        g = (y * a[:, None] / y.abs().mean()).reshape(p.shape)
    elif kind == "none":
        g = p / p.pow(2).mean().sqrt() + 0.3 * noise
    else:
        g = noise
    return (1e-2 * g).float()


def run(case, dtype, p0, grads=None, project=True):
    """the trajectory in `dtype`; grads None: build them from this run's own parameters (the float32 run).  Returns a dict of lists per step"""
    c = CASES[case]
    h = dict(DEFAULTS, **c["hyper"])
    group_of = {i: gi for gi, idx in enumerate(c["groups"]) for i in idx}
    ps = [t.to(dtype).clone() for t in p0]
    sts = [dict(step=0, exp_avg=torch.zeros_like(t), exp_avg_sq=torch.zeros_like(t)) for t in ps]
    gen = torch.Generator().manual_seed(c["seed"] + 1000)
    out = dict(p=[], grads=[], modes=[], margins=[], state=sts)
    for k in range(STEPS):
        gk = [make_grad(WANT[i], ps[i], gen) for i in range(len(ps))] if grads is None else grads[k]
        modes, margins = [], []
        for i, g in enumerate(gk):
            ps[i], md, mg = adamp_tensor_step(ps[i], g.to(dtype), sts[i], h, c["lrs"][k], c["wds"][group_of[i]], project)
            modes.append(md)
            margins.append(mg)
        out["p"].append([t.clone() for t in ps])
        out["grads"].append(gk)
        out["modes"].append(modes)
        out["margins"].append(margins)
    return out


def flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def _js(x):
    return np.frombuffer(json.dumps(x).encode(), dtype=np.uint8)


def main():
    torch.set_num_threads(1)
    arrays = {"shapes": _js(SHAPES)}
    want_mode = {"channel": 1, "layer": 2, "none": 0, "1d": 0}
    for case, c in CASES.items():
        gen = torch.Generator().manual_seed(c["seed"])
        p0 = [(torch.randn(s, generator=gen) * (0.02 * 2.0 ** ((i + 1) % 3))) for i, s in enumerate(SHAPES)]
        r32 = run(case, torch.float32, p0)
        r64 = run(case, torch.float64, p0, r32["grads"])
        off = run(case, torch.float64, p0, r32["grads"], project=False)
        modes = np.array(r64["modes"], dtype=np.int32)
        assert (modes == np.array(r32["modes"])).all() and (modes == np.array([[want_mode[w] for w in WANT]] * STEPS)).all(), modes
        margins = np.array([r32["margins"], r64["margins"]])
        taken = margins[~np.isnan(margins)]
        assert ((taken <= 0.5) | (taken >= 2.0)).all(), margins
        yard = np.array([[(a.double() - b).abs().max().item() for a, b in zip(r32["p"][k], r64["p"][k])] for k in range(STEPS)])
        effect = np.array([[(a - b).abs().max().item() for a, b in zip(off["p"][k], r64["p"][k])] for k in range(STEPS)])
        assert (effect[modes > 0] >= 100 * yard[modes > 0]).all() and (effect[modes == 0] == 0).all(), (effect, yard)
        print(f"{case}: margins under the threshold <= {taken[taken < 1].max():.2e}, over it >= {taken[taken > 1].min():.2f}; "
              f"effect / yard >= {(effect[modes > 0] / yard[modes > 0]).min():.0f}; yard <= {yard.max():.2e}")
        arrays.update({
            f"{case}/hyper": _js(c["hyper"]), f"{case}/groups": _js(c["groups"]), f"{case}/wds": np.array(c["wds"]),
            f"{case}/lrs": np.array(c["lrs"]), f"{case}/p0": flat(p0).numpy(),
            f"{case}/grads": torch.stack([flat(g) for g in r32["grads"]]).numpy(),
            f"{case}/p64": torch.stack([flat(p) for p in r64["p"]]).numpy(), f"{case}/yard": yard, f"{case}/modes": modes,
            f"{case}/margins": margins, f"{case}/effect": effect,
            f"{case}/state4/exp_avg": flat([s["exp_avg"] for s in r32["state"]]).numpy(),
            f"{case}/state4/exp_avg_sq": flat([s["exp_avg_sq"] for s in r32["state"]]).numpy(),
        })
    np.savez(OUT, **arrays)
    size = os.path.getsize(OUT)
    assert size <= 1.0e6, size
    print(f"{OUT}: {size} bytes")


if __name__ == "__main__":
    main()
