"""What forward spectral normalisation costs a training step on one MI355X: forward + backward of the plain ResNet-50 executor at bf16, batch 256,
224 px, with the switch off and on (csrc/spectral_norm.hip: 5 launches over the 53 conv matrices / 23 454 912 elements at the head of the
forward, 2 behind the weight gradients of each of the 17 backward segments that hold a convolution).

    python tools/spectral_norm_bench.py [--out profiles/spectral_norm.json] [--rounds 7] [--steps 10]
    python tools/spectral_norm_bench.py --off-only        # runs on a tree without the switch too: the off case against the parent commit

One process; the cases alternate inside every round; a case's figure in a round is a window of --steps steps between two device events, divided
by the steps; the JSON holds the median over the rounds and the rounds themselves.  The optimizer step and the loss are left out: the gradient
wrt the logits is a constant.  "other_class_ms" is one step's HIP-event time of the executor's profile class 6 — the weight preparation at the
head of the forward and the per-segment gradient rule, among other small launches — off and on: the difference is the new launches alone, timed
on their own streams."""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args(argv)
    import torch

    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.synth import synthetic_batch

    assert torch.cuda.is_available(), "needs the MI355X"
    m = resnet50(dtype="bf16").cuda()
    m.train()
    data, target = synthetic_batch(a.batch, a.size, seed=0, index=0, device="cuda")
    dlogits = (torch.softmax(torch.zeros_like(target), 1) - target) / a.batch
    cases = ["off"] if a.off_only else ["off", "on"]

    def window(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            m.zero_grad()
            m(data).backward(dlogits)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def switch(case):
        if not a.off_only:
            m.set_spectral_norm(case == "on")

    for case in cases:  # warm-up: contexts, scratch, caches
        switch(case)
        window(3)
    times = {c: [] for c in cases}
    for _ in range(max(a.rounds, 1)):
        for case in cases:
            switch(case)
            window(1)  # (the first step after a switch is not timed)
            times[case].append(window(a.steps))
    med = {c: statistics.median(v) for c, v in times.items()}
    res = {
        "device": torch.cuda.get_device_name(0),
        "dtype": "bf16", "batch": a.batch, "image_size": a.size, "rounds": a.rounds, "steps_per_window": a.steps,
        "fwd_bwd_ms": {c: round(v, 4) for c, v in med.items()},
        "rounds_ms": {c: [round(x, 4) for x in v] for c, v in times.items()},
        "spread_ms": {c: round(max(v) - min(v), 4) for c, v in times.items()},
    }
    if not a.off_only:
        res["on_cost_ms"] = {c: round(med[c] - med["off"], 4) for c in cases if c != "off"}
        from sota_imagenet_amd import item_plan

        mats, n_u, n_v = item_plan.spectral_mats(m._table)
        res["matrices"], res["rows"], res["v_elements"], res["elements"] = len(mats), n_u, n_v, sum(L * R for _, L, R, _, _ in mats)
        shape, other = (a.batch, a.size, a.size), {}
        for case in cases:  # one profiled step per case: the class of the small launches
            switch(case)
            window(1)
            m.profile(shape, 1 << 6)
            window(1)
            ms, n, _, _ = m.profile_read(shape, 6)
            m.profile(shape, 0)
            other[case] = {"ms": round(ms, 4), "records": n}
        res["other_class_ms"] = other
        res["new_launches_ms"] = round(other["on"]["ms"] - other["off"]["ms"], 4)
        m.set_spectral_norm(False)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
