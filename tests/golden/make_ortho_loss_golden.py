#!/usr/bin/env python3
"""Records tests/golden/ortho_loss_ref.npz by running the REFERENCE's own OrthoLoss and NormLoss (sota_imagenet/callbacks.py of a reference
checkout, loaded by path through make_sam_golden.load_reference and its stubs; none of its text is here) on the CPU with one thread, once in
float32 and once in float64.

    python tests/golden/make_ortho_loss_golden.py --reference <checkout of the reference>

The module tree (MODULES; weights from synth.uniform_tensor, scaled per module): convolutions of several shapes, a grouped one, one with more
filters than filter elements (O > K: never penalised), one below min_filters in both settings, a Linear, a BatchNorm of 64 channels and one of 32
(below NormLoss's 64 elements), a Conv1d of 5 elements.  OrthoLoss runs at two settings of (min_filters, min_norm) (SETTINGS): conv `f` is open in
the first and closed by min_norm in the second, conv `c` is dropped by min_filters in the second.

Arrays of the file:
    names (json), w/<name>                    every module's weight, float32, torch's own layout
    ortho/<k>/setting (json), loss, F (json: name -> F of the float64 run for the matrices that passed the shape rule), contributed (json: names
                                              with a gradient), g/<name> (float64 gradient; zeros where the module did not contribute)
    norm/loss, contributed, g/<name>          likewise for NormLoss
    */yard_loss, */yard_g/<name>              |float32 run - float64 run|: the reference's own float32 error
At recording time it asserts that the float32 run lies inside the bounds of tests/ortho_loss_common.py around the float64 one and that every
F / O clears min_norm by a relative 1e-3."""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ortho_loss_common as C  # noqa: E402
from make_sam_golden import load_reference  # noqa: E402

from sota_imagenet_amd.synth import uniform_tensor  # noqa: E402

# name -> (constructor, weight scale)
MODULES = {
    "a": (lambda: torch.nn.Conv2d(8, 16, 3, bias=False), 0.2),            # [16, 72]
    "b": (lambda: torch.nn.Conv2d(16, 24, 1, bias=True), 0.24),           # [24, 16]: O > K
    "c": (lambda: torch.nn.Conv2d(4, 12, 3, bias=False), 0.3),            # [12, 36]
    "d": (lambda: torch.nn.Conv2d(16, 16, 3, groups=4, bias=False), 0.05),  # grouped: [16, 36]
    "e": (lambda: torch.nn.Conv2d(8, 4, 3, bias=False), 0.2),             # [4, 72]: below min_filters
    "f": (lambda: torch.nn.Conv2d(3, 64, 7, bias=False), 0.1),            # the stem's shape: [64, 147]
    "fc": (lambda: torch.nn.Linear(20, 10), 0.3),
    "bn64": (lambda: torch.nn.BatchNorm2d(64), 1.0),
    "bn32": (lambda: torch.nn.BatchNorm2d(32), 1.0),
    "eca": (lambda: torch.nn.Conv1d(1, 1, 5, bias=False), 0.5),
}
SETTINGS = [dict(min_filters=8, min_norm=0.0), dict(min_filters=16, min_norm=0.2)]


def build(dtype):
    net = torch.nn.Sequential()
    for k, (name, (make, scale)) in enumerate(MODULES.items()):
        m = make()
        with torch.no_grad():
            m.weight.copy_(uniform_tensor(tuple(m.weight.shape), scale * 1.7320508, 9100 + k))
        net.add_module(name, m)
    return net.to(dtype)


def run(term, net):
    net.zero_grad()
    with contextlib.redirect_stdout(io.StringIO()):
        loss = term(None, None)
    loss.backward()
    contributed = [n for n in MODULES if net._modules[n].weight.grad is not None]
    grads = {n: (net._modules[n].weight.grad.detach().double().numpy() if n in contributed else np.zeros(tuple(net._modules[n].weight.shape)))
             for n in MODULES}
    return float(loss.detach().double()), grads, contributed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "ortho_loss_ref.npz"))
    a = ap.parse_args()
    clb, _ = load_reference(a.reference)
    torch.set_num_threads(1)
    nets = {dt: build(dt) for dt in (torch.float32, torch.float64)}
    out = {"names": json.dumps(list(MODULES))}
    for n in MODULES:
        out[f"w/{n}"] = nets[torch.float32]._modules[n].weight.detach().numpy()
    mat = lambda n: out[f"w/{n}"].reshape(out[f"w/{n}"].shape[0], -1)  # noqa: E731
    for k, st in enumerate(SETTINGS):
        r32 = run(clb.OrthoLoss(nets[torch.float32], **st), nets[torch.float32])
        r64 = run(clb.OrthoLoss(nets[torch.float64], **st), nets[torch.float64])
        assert r32[2] == r64[2], (r32[2], r64[2])
        convs = [n for n in MODULES if out[f"w/{n}"].ndim == 4 and mat(n).shape[0] <= mat(n).shape[1] and mat(n).shape[0] >= st["min_filters"]]
        _, _, Fs, gates = C.ortho_loss64([mat(n) for n in convs], st["min_norm"])
        assert [n for n, g in zip(convs, gates) if g] == r64[2], (convs, gates, r64[2])
        b_loss = 0.0
        for n, F, gate in zip(convs, Fs, gates):
            assert C.clearance(F, mat(n).shape[0], st["min_norm"]) >= C.CLEAR, (n, F)
            bF, bg = C.whole_rule_bounds(mat(n), F, gate)
            b_loss += bF if gate else 0.0
            assert C.worst(r32[1][n].reshape(mat(n).shape), r64[1][n].reshape(mat(n).shape), bg) <= 1.0, n
        assert abs(r32[0] - r64[0]) <= b_loss, (r32[0], r64[0], b_loss)
        out[f"ortho/{k}/setting"] = json.dumps(st)
        out[f"ortho/{k}/loss"], out[f"ortho/{k}/yard_loss"] = np.float64(r64[0]), np.float64(abs(r32[0] - r64[0]))
        out[f"ortho/{k}/F"] = json.dumps(dict(zip(convs, Fs)))
        out[f"ortho/{k}/contributed"] = json.dumps(r64[2])
        for n in MODULES:
            out[f"ortho/{k}/g/{n}"] = r64[1][n]
            out[f"ortho/{k}/yard_g/{n}"] = np.float64(np.abs(r32[1][n] - r64[1][n]).max())
    assert json.loads(out["ortho/0/contributed"]) != json.loads(out["ortho/1/contributed"])
    r32 = run(clb.NormLoss(nets[torch.float32]), nets[torch.float32])
    r64 = run(clb.NormLoss(nets[torch.float64]), nets[torch.float64])
    assert r32[2] == r64[2]
    ref, bound, _ = C.norm_loss64([mat(n) for n in r64[2]], eps=C.U)
    assert abs(r64[0] - ref) <= 1e-12 * abs(ref) and abs(r32[0] - r64[0]) <= bound, (r32[0], r64[0], ref, bound)
    for n in r64[2]:
        g, bg = C.norm_grad64(mat(n), 1.0, eps=C.U)
        assert C.worst(r32[1][n].reshape(mat(n).shape), g, bg) <= 1.0, n
    out["norm/loss"], out["norm/yard_loss"] = np.float64(r64[0]), np.float64(abs(r32[0] - r64[0]))
    out["norm/contributed"] = json.dumps(r64[2])
    for n in MODULES:
        out[f"norm/g/{n}"] = r64[1][n]
        out[f"norm/yard_g/{n}"] = np.float64(np.abs(r32[1][n] - r64[1][n]).max())
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; ortho contributed {out['ortho/0/contributed']} / {out['ortho/1/contributed']}; "
          f"F/O " + ", ".join(f"{n}={F / mat(n).shape[0]:.3f}" for n, F in json.loads(out['ortho/0/F']).items()))


if __name__ == "__main__":
    main()
