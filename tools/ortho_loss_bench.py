"""What the orthogonality penalty costs on one MI355X: the launches of losses.OrthoLoss on ResNet-50's 33 matrices (min_filters 64; csrc/ortho_loss.hip:
three launches forward, one backward), timed serially, against the same rule written with torch-ROCm ops (mat @ mat.T, norm, autograd) on the
same weights, and the same pair for NormLoss.

    python tools/ortho_loss_bench.py [--out profiles/ortho_loss.json] [--reps 20] [--step-ms 17.6]

One process; each figure is the median of --reps repetitions, each between two device events with nothing else on the stream, after three
warm-up repetitions.  The torch form is the reference's loop as it stands (sota_imagenet/callbacks.py:138-156): one host synchronisation per
matrix for the gate, which the event window includes; "torch_nosync" drops the gate (min_norm 0 opens every one) to show the vendor GEMMs alone.
--step-ms: the bf16 forward + backward the shares are taken of."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--min-filters", type=int, default=64)
    ap.add_argument("--step-ms", type=float, default=17.6)
    a = ap.parse_args(argv)
    import torch

    from sota_imagenet_amd import ops
    from sota_imagenet_amd.losses import NormLoss, OrthoLoss
    from sota_imagenet_amd.models import resnet50

    assert torch.cuda.is_available(), "needs the MI355X"
    m = resnet50(dtype="bf16").cuda()
    flat = m.flat_params.detach()
    pen, nl = OrthoLoss(m, min_filters=a.min_filters, min_norm=0), NormLoss(m)
    pen._plan(), nl._plan()
    one = torch.ones(1, device=flat.device)
    ws = [flat[o: o + R * L].view(R, L).clone().requires_grad_(True) for o, L, R, _ in pen.mats]
    rows = [flat[o: o + R * L].view(R, L).clone().requires_grad_(True) for o, R, L in nl.records]

    def timed(fn):
        for _ in range(3):
            fn()
        out = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)

    def torch_ortho(sync):
        loss = 0
        for w in ws:
            w.grad = None
            corr = w @ w.T - torch.eye(w.size(0), device=w.device)
            if not sync or corr.norm() / corr.size(0) > 0:  # the reference's gate reads a device scalar
                loss = loss + corr.norm()
        (loss * 0.001).backward()

    def torch_norm():
        loss = 0
        for w in rows:
            w.grad = None
            loss = loss + (1 - w.norm(dim=-1)).pow(2).mean()
        (loss * 1e-4).backward()

    cases = {
        "ortho_native_fwd": lambda: pen._launch_forward(),
        "ortho_native_fwd_bwd": lambda: (pen._launch_forward(), ops.ortho_loss_bwd(flat, m.flat_grads, pen._tables, pen._scratch, one, accumulate=True)),
        "ortho_torch_fwd_bwd": lambda: torch_ortho(True),
        "ortho_torch_nosync_fwd_bwd": lambda: torch_ortho(False),
        "norm_native_fwd_bwd": lambda: (nl._launch_forward(), ops.norm_loss_bwd(flat, m.flat_grads, nl._items_dev, nl._tensors_dev, one, accumulate=True)),
        "norm_torch_fwd_bwd": torch_norm,
    }
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "min_filters": a.min_filters, "matrices": len(pen.mats),
           "gram_flop": sum(2 * R * R * L for _, L, R, _ in pen.mats), "gram_items": int(pen._tables["items"].shape[0]),
           "grad_items": int(pen._tables["gitems"].shape[0]), "norm_tensors": len(nl.records), "step_ms": a.step_ms, "ms": {}, "share_of_step": {}}
    for name, fn in cases.items():
        med, lo, hi = timed(fn)
        res["ms"][name] = {"median": med, "min": lo, "max": hi}
        res["share_of_step"][name] = round(med / a.step_ms, 4)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
