#!/usr/bin/env python3
"""Records tests/golden/weight_norm_ref.npz by running the REFERENCE's own WeightNorm callback (sota_imagenet/callbacks.py:104-123 of a reference
checkout, loaded by path through make_sam_golden.load_reference and its stub modules; none of its text is here) on the CPU with one thread, in
float32, over a tiny module tree, and recording every weight before and after one on_batch_end.

    python tests/golden/make_weight_norm_golden.py --reference <checkout of the reference>

The module tree (MODULES below): Conv2d(3->8, k7) with a bias (rows of 147), Conv2d(64->4, k1), Conv2d(16->5, k3), Linear(65->3), Conv1d(1->1, k5)
(skipped by the reference: numel < 64), BatchNorm2d(32) (skipped: numel < 64), BatchNorm2d(64) — which the reference does NOT skip: its
view(64, -1) is 64 x 1, every row's mean is the element itself and its norm 0, so the whole weight becomes NaN, recorded here to document why
the native planner leaves tensors of one dimension alone — and Conv2d(8->6, k3) whose filter 2 is constant (0.25: a NaN row, 0 / 0).
Two draws: torch's default initialisation under a seed, and the same with 0.05 added to every weight (a mean that is not small against the
spread); the constant filter and the BatchNorm weights (ones) are set after that.

At recording time the reference's float32 result is held against the float64 restatement of the rule inside the reference bound
(tests/weight_norm_common.py); the worst ratio is printed and stored.

Arrays of the file: names (json: the modules' names in order), skipped (json: names the reference leaves alone), and per draw d in (0, 1) and
module name: d<d>/<name>/before, d<d>/<name>/after (float32, the weight's own shape), d<d>/<name>/bias_before, bias_after where there is a
bias; ratio [2]: the worst |reference - float64| / reference bound per draw."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_sam_golden import load_reference  # noqa: E402
import weight_norm_common as WN  # noqa: E402

MODULES = [("stem", lambda: torch.nn.Conv2d(3, 8, 7, bias=True)), ("point", lambda: torch.nn.Conv2d(64, 4, 1, bias=False)),
           ("conv3", lambda: torch.nn.Conv2d(16, 5, 3, bias=False)), ("fc", lambda: torch.nn.Linear(65, 3)),
           ("eca", lambda: torch.nn.Conv1d(1, 1, 5, bias=False)), ("bn32", lambda: torch.nn.BatchNorm2d(32)),
           ("bn64", lambda: torch.nn.BatchNorm2d(64)), ("flat", lambda: torch.nn.Conv2d(8, 6, 3, bias=False))]
SKIPPED = ["eca", "bn32"]   # numel < 64
NAN_WHOLE = ["bn64"]        # rows of one element
CONST_ROW = ("flat", 2, 0.25)
SHIFT = [0.0, 0.05]


def build(draw):
    torch.manual_seed(4100 + draw)
    model = torch.nn.Sequential()
    for name, make in MODULES:
        model.add_module(name, make())
    with torch.no_grad():
        for name, m in model.named_children():
            if not isinstance(m, torch.nn.BatchNorm2d):
                m.weight.add_(SHIFT[draw])
        getattr(model, CONST_ROW[0]).weight[CONST_ROW[1]].fill_(CONST_ROW[2])
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "weight_norm_ref.npz"))
    a = ap.parse_args()
    clb_mod, _ = load_reference(a.reference)
    torch.set_num_threads(1)

    def js(x):
        return np.frombuffer(json.dumps(x).encode(), dtype=np.uint8)

    arrays = {"names": js([n for n, _ in MODULES]), "skipped": js(SKIPPED)}
    ratios = []
    for d in range(2):
        model = build(d)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        clb = clb_mod.WeightNorm()
        clb.state = types.SimpleNamespace(model=model)
        clb.on_batch_end()
        after = {k: v.detach().clone() for k, v in model.state_dict().items()}
        worst = 0.0
        for name, _ in MODULES:
            b, f = before[f"{name}.weight"].numpy(), after[f"{name}.weight"].numpy()
            arrays[f"d{d}/{name}/before"], arrays[f"d{d}/{name}/after"] = b, f
            if f"{name}.bias" in before:
                arrays[f"d{d}/{name}/bias_before"], arrays[f"d{d}/{name}/bias_after"] = before[f"{name}.bias"].numpy(), after[f"{name}.bias"].numpy()
                assert np.array_equal(before[f"{name}.bias"].numpy(), after[f"{name}.bias"].numpy())  # no bias is touched
            if name in SKIPPED:
                assert np.array_equal(b, f)
                continue
            if name in NAN_WHOLE:
                assert np.isnan(f).all() and np.isfinite(b).all()
                continue
            x = b.reshape(b.shape[0], -1)
            M, N, Y = WN.rule64(x)
            ok = N[:, 0] > 0
            if name == CONST_ROW[0]:
                assert not ok[CONST_ROW[1]] and ok.sum() == len(ok) - 1 and np.isnan(f[CONST_ROW[1]]).all()
            else:
                assert ok.all()
            got = f.reshape(x.shape)
            assert np.isfinite(got[ok]).all()
            r = WN.worst_ratio(got[ok], Y[ok], WN.reference_bound(x[ok], M[ok], N[ok], Y[ok]))
            print(f"draw {d} {name} {tuple(b.shape)}: reference's float32 error / reference bound = {r:.3f}")
            assert r <= 1.0, (d, name, r)
            worst = max(worst, r)
        ratios.append(worst)
    arrays["ratio"] = np.array(ratios)
    np.savez_compressed(a.out, **arrays)
    print(a.out, os.path.getsize(a.out), "bytes; worst ratio per draw", ratios)
    assert os.path.getsize(a.out) < 100 << 10


if __name__ == "__main__":
    main()
