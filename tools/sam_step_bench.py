"""SAMOriginal timing on one MI355X: the four kernels of csrc/optim_sam.hip on the real ResNet-50 flat array (161 tensors, 25 557 032 parameter
elements) with adam_kernel timed in the same session as the yardstick, and the Runner step of the nov-adam_sam_test recipe's model (ResNet-50 bf16
under AdamLayerwise) at batch 256, 224 px with and without the callback.

    python tools/sam_step_bench.py [--out profiles/sam_step.json]

Kernel method of tools/layerwise_step_bench.py: a warm-up, then device events around a window of back-to-back launches of at least --window
seconds; every case --rounds times, the cases alternating inside a round; the JSON holds the median and the min / max of the rounds.
Traffic per element: sam_sumsq 8 B (p, g read), sam_perturb 16 B (p, g read; eps, p written), sam_restore 12 B (p, eps read; p written): 36 B a
step; sam_scale reads one double per work item.  Adam 28 B.  The stages are timed through sota_imagenet_amd.ops on the plan the callback built.
The Runner figure is wall time per step over --steps steps after a warm-up fit, one synthetic batch reused, host and device together."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import MEASURED_TBPS, SPEC_TBPS, time_window  # noqa: E402


def kernel_part(a, torch):
    from sota_imagenet_amd import ops
    from sota_imagenet_amd.callbacks import SAMOriginal
    from sota_imagenet_amd.models import resnet50

    m = resnet50(dtype="fp32").cuda()
    params = list(m.parameters())
    n_real, n_flat = sum(p.numel() for p in params), m.flat_params.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    m.flat_grads.copy_(torch.randn(n_flat, device="cuda", generator=gen) * 1e-3)
    p0 = m.flat_params.clone()
    sam = SAMOriginal()
    sam.build_plan(params)
    s1, s2 = torch.zeros_like(p0), torch.zeros_like(p0)
    step = [0]

    def adam():
        ops.adam_step(m.flat_params, m.flat_grads, s1, s2, step[0] % 1000, 1e-3, (0.9, 0.999), 1e-8, 5e-2, decoupled=True)
        step[0] += 1

    def sumsq():
        for seg in sam._segs:
            i0, i1 = seg.items
            ops.sam_sumsq(seg.p, seg.g, sam._items[i0:i1], sam._kind, sam._partial[i0:i1], sam.eta)

    def scale():
        ops.sam_scale(sam._partial, sam.rho, sam._out)

    def perturb():
        for seg in sam._segs:
            i0, i1 = seg.items
            ops.sam_perturb(seg.p, seg.g, seg.eps, sam._items[i0:i1], sam._kind, sam._out, sam.eta)

    def restore():
        for seg in sam._segs:
            i0, i1 = seg.items
            ops.sam_restore(seg.p, seg.eps, sam._items[i0:i1], sam._kind.numel())

    def four():
        sumsq()
        scale()
        perturb()
        restore()

    B = n_real
    cases = [("adam_kernel", adam, 28 * n_flat), ("sam_sumsq_kernel", sumsq, 8 * B), ("sam_scale_kernel", scale, 0),
             ("sam_perturb_kernel", perturb, 16 * B), ("sam_restore_kernel", restore, 12 * B), ("sam_four_stages", four, 36 * B)]
    times = {name: [] for name, _, _ in cases}
    for _ in range(max(a.rounds, 1)):
        for name, fn, _ in cases:
            m.flat_params.copy_(p0)
            sumsq()
            scale()  # a valid out[] for the perturbation, whichever case runs
            sam._eps[0].zero_()
            us, iters, secs = time_window(fn, max(a.window, 0.2))
            times[name].append(us)
    out = {}
    for name, _, nbytes in cases:
        ts = times[name]
        c = dict(us_per_step=round(statistics.median(ts), 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2), rounds=len(ts), bytes_per_step=nbytes)
        if nbytes:
            gbps = nbytes / (c["us_per_step"] * 1e-6) / 1e9
            c.update(GBps=round(gbps, 1), frac_of_spec_8TBps=round(gbps / (SPEC_TBPS * 1e3), 3),
                     **{"frac_of_measured_6.29TBps": round(gbps / (MEASURED_TBPS * 1e3), 3)})
        out[name] = c
    return {
        "n_parameter_elements": n_real,
        "n_flat_elements": n_flat,
        "tensors": len(params),
        "weights": int(sam._kind.sum()),
        "item_elems": ops.lw_item_elems(),
        "work_items": int(sam._items.shape[0]),
        "launches_per_step": 4,
        "bytes_per_element": {"sam_sumsq": 8, "sam_perturb": 16, "sam_restore": 12, "step": 36},
        "kernels": out,
        "us_vs_adam_kernel": {k: round(c["us_per_step"] / out["adam_kernel"]["us_per_step"], 3) for k, c in out.items()},
        "GBps_vs_adam_kernel": {k: round(c["GBps"] / out["adam_kernel"]["GBps"], 3) for k, c in out.items() if "GBps" in c},
    }


def runner_part(a, torch):
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAMOriginal
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.synth import synthetic_batch

    batch = synthetic_batch(a.batch, a.size, seed=0, index=0, device="cuda")

    class Loader:
        batch_size = a.batch

        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __iter__(self):
            return iter([batch] * self.n)

    res = {}
    for name in ("without_callback", "with_callback"):
        m = resnet50(dtype="bf16").cuda()
        opt = optim.AdamLayerwise([{"params": list(m.parameters())}], lr=1e-4, betas=(0.9, 0.995), weight_decay=2e-2)
        sam = SAMOriginal()
        runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[sam] if name == "with_callback" else [])
        runner.fit(Loader(3), epochs=1)  # contexts, plans, the skipped first step
        torch.cuda.synchronize()
        ts = []
        for _ in range(max(a.rounds, 1)):
            t0 = time.perf_counter()
            runner.fit(Loader(a.steps), epochs=1)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.steps * 1e3)
        res[name] = dict(ms_per_step=round(statistics.median(ts), 2), ms_min=round(min(ts), 2), ms_max=round(max(ts), 2), rounds=len(ts),
                         images_per_sec=round(a.batch / statistics.median(ts) * 1e3, 1), finite=bool(torch.isfinite(m.flat_params).all()))
        if name == "with_callback":
            res[name]["second_forwards"] = sam.forwards
        del runner, opt, m
        torch.cuda.empty_cache()
    res["step_time_ratio"] = round(res["with_callback"]["ms_per_step"] / res["without_callback"]["ms_per_step"], 3)
    return dict(model="resnet50 bf16, AdamLayerwise (recipe 49's values)", batch=a.batch, image_size=a.size, steps=a.steps, **res)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per case and round (>= 0.2)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args(argv)
    import torch

    assert torch.cuda.is_available(), "needs the MI355X"
    res = {"device": torch.cuda.get_device_name(0)}
    res.update(kernel_part(a, torch))
    torch.cuda.empty_cache()
    res["runner_step"] = runner_part(a, torch)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
