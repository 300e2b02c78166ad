"""The WeightNorm callback's launch on one MI355X against the reference's loop, on the real ResNet-50 flat array (54 tensors, 27 560 rows,
25 502 912 elements: 204 MB to read once and write once).

    python tools/weight_norm_bench.py [--out profiles/weight_norm.json]

  native_warm    ops.weight_norm_rows_ back to back, device events around a window of launches (tools/optim_step_bench.time_window).  The 102 MB
                 array fits the 256 MiB Infinity Cache, so these launches find it there: the rate is the kernel's with its input on the die
  native_cold    the same launch behind a 512 MiB fill that pushes the array out of the caches, one pair of device events around every launch;
                 the median.  What a training step sees: a forward and a backward lie between two launches
  reference      the loop of sota_imagenet/callbacks.py:116-123 written with torch on the same rows of the flat array — per tensor mean, subtract,
                 norm, divide: four launches, 216 for the model —, back to back (its input on the die too)
Every case is timed --rounds times, the cases alternating inside a round; the JSON holds the median and the rounds.  Both ways run on the same
seeded array in one process and are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import MEASURED_TBPS, time_window  # noqa: E402

STEP_MS_BF16 = 17.5  # the bf16 training step at bs 256, 224 px (README)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cold-reps", type=int, default=30, help="flushed launches per round")
    a = ap.parse_args(argv)
    import torch

    from sota_imagenet_amd import item_plan, ops
    from sota_imagenet_amd.models import resnet50

    assert torch.cuda.is_available(), "needs the MI355X"
    m = resnet50(dtype="fp32").cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():  # a network's spread around a small mean
        m._flat_params.copy_(torch.randn(m._flat_params.numel(), device="cuda", generator=gen) * 2e-2 + 1e-3)
    flat = m.flat_params.detach()
    recs = item_plan.wnorm_records(m._table)
    items = item_plan.wnorm_items(recs, ops.WNORM_ITEM_ELEMS)
    items_dev = item_plan.pack_records(items, flat.device)
    ops.wnorm_check_items(items)
    n_elems = sum(rows * L for _, rows, L in recs)
    views = [flat[off:off + rows * L].view(rows, L) for off, rows, L in recs]

    def native():
        return ops.weight_norm_rows_(flat, None, items_dev)

    @torch.no_grad()
    def reference():
        for w in views:
            w -= w.mean(dim=-1, keepdim=True)
            w /= w.norm(dim=-1, keepdim=True)

    # the two ways on the same input
    start = flat.clone()
    status = native()
    got = flat.clone()
    flat.copy_(start)
    reference()
    diff = (got - flat).abs().max().item()
    assert status.eq(0).all().item() and diff < 1e-5, f"native and reference differ by {diff}"

    scratch = torch.empty(512 << 18, dtype=torch.float32, device="cuda")  # 512 MiB

    def native_cold_us(reps):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            scratch.fill_(1.0)
            e0.record()
            native()
            e1.record()
        torch.cuda.synchronize()
        return statistics.median(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)

    native_cold_us(3)
    times = {"native_warm_us": [], "native_cold_us": [], "reference_us": []}
    for _ in range(max(a.rounds, 1)):
        times["native_warm_us"].append(time_window(native, 0.2)[0])
        times["reference_us"].append(time_window(reference, 0.2)[0])
        times["native_cold_us"].append(native_cold_us(a.cold_reps))
    med = {k: statistics.median(v) for k, v in times.items()}
    moved = 8 * n_elems  # read once, written once
    res = {
        "device": torch.cuda.get_device_name(0),
        "tensors": len(recs),
        "rows": sum(rows for _, rows, _ in recs),
        "elements": n_elems,
        "work_items": len(items),
        "item_elems": ops.WNORM_ITEM_ELEMS,
        "wave_row_max": ops.WNORM_WAVE_ROW_MAX,
        "bytes_moved": moved,
        "rounds": {k: [round(x, 1) for x in v] for k, v in times.items()},
        "native_warm_us": round(med["native_warm_us"], 1),
        "native_warm_GBps": round(moved / (med["native_warm_us"] * 1e-6) / 1e9, 1),
        "native_cold_us": round(med["native_cold_us"], 1),
        "native_cold_GBps": round(moved / (med["native_cold_us"] * 1e-6) / 1e9, 1),
        "floor_us_at_6.29TBps": round(moved / (MEASURED_TBPS * 1e12) * 1e6, 1),
        "native_cold_share_of_bf16_step": round(med["native_cold_us"] * 1e-3 / STEP_MS_BF16, 4),
        "reference_us": round(med["reference_us"], 1),
        "reference_launches": 4 * len(recs),
        "reference_over_native_cold": round(med["reference_us"] / med["native_cold_us"], 1),
        "max_abs_difference_native_reference": diff,
    }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
