"""One logged epoch-begin of callbacks.WeightDistributionTB on one MI355X against the reference's way, on the real ResNet-50 (320 state_dict
entries: 161 parameters, 106 running statistics, 53 int64 counters).

    python tools/weight_dist_bench.py [--out profiles/weight_dist.json]

  native      cb.on_epoch_begin() with the plan built: one zero_ of the table, one mi355_tbbin_hist per flat array, the gather of the counters, ONE
              copy to the host, and the host's part (per tag: trimming, the items' statistics combined, the lists).  Host clock; the call ends in
              the copy's synchronise.
  kernels     the two counting launches alone, device events around a window of back-to-back launches (tools/optim_step_bench.time_window)
  reference   what add_histogram does per entry, as the reference's callback calls it: p.flatten().cpu().numpy().astype(float64), np.histogram
              over the 1549 default edges, min, max, sum, dot, the trimming.  Host clock; every entry's copy synchronises.
Every case is timed --rounds times, the cases alternating inside a round; the JSON holds the median and the min / max of the rounds.  Both ways
run on the same seeded model in one process, and their histograms are compared before anything is timed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import MEASURED_TBPS, time_window  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--native-reps", type=int, default=20, help="logged epochs per round")
    ap.add_argument("--reference-reps", type=int, default=2)
    a = ap.parse_args(argv)
    import numpy as np
    import torch

    from sota_imagenet_amd import callbacks, ops
    from sota_imagenet_amd.fit_wrapper import RunnerState
    from sota_imagenet_amd.models import resnet50

    assert torch.cuda.is_available(), "needs the MI355X"
    m = resnet50(dtype="fp32").cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():  # a trained network's spread: a few decades around 1e-2, the running variances positive
        m._flat_params.copy_(torch.randn(m._flat_params.numel(), device="cuda", generator=gen) * 2e-2)
        m._flat_buffers.copy_(torch.rand(m._flat_buffers.numel(), device="cuda", generator=gen) + 0.1)
        m._nbt.fill_(5004)
    edges = ops.tbbin_edges()

    def reference():
        out = {}
        for name, p in m.state_dict().items():
            v = p.flatten().cpu().numpy().astype(np.float64)
            counts, _ = np.histogram(v, bins=edges)
            limits, kept = callbacks.tb_trim(counts, edges)
            out["model/" + name] = dict(min=v.min(), max=v.max(), num=v.size, sum=v.sum(), sum_squares=v.dot(v), bucket_limits=limits,
                                        bucket_counts=kept)
        return out

    cb = callbacks.WeightDistributionTB()
    cb.set_state(RunnerState(model=m))
    t0 = time.perf_counter()
    cb.on_epoch_begin()  # builds the plan
    first_ms = (time.perf_counter() - t0) * 1e3
    ref = reference()
    same = list(ref) == list(cb.last) and all(
        ref[t]["bucket_counts"] == cb.last[t]["bucket_counts"] and ref[t]["bucket_limits"] == cb.last[t]["bucket_limits"]
        and ref[t]["min"] == cb.last[t]["min"] and ref[t]["max"] == cb.last[t]["max"] for t in ref)
    assert same, "the native histograms differ from the reference's way"
    worst_sum = max(abs(ref[t]["sum"] - cb.last[t]["sum"]) / max(abs(ref[t]["sum"]), 1e-300) for t in ref)

    def host_ms(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    P = cb._plan

    def kernels():
        for src, items, (i0, i1) in P.launches:
            ops.tbbin_hist(src, items, P.hist, P.partial[i0:i1])

    times = {"native_epoch_begin_ms": [], "reference_way_ms": [], "kernels_us": []}
    for _ in range(max(a.rounds, 1)):
        times["native_epoch_begin_ms"].append(host_ms(cb.on_epoch_begin, a.native_reps))
        times["reference_way_ms"].append(host_ms(reference, a.reference_reps))
        times["kernels_us"].append(time_window(kernels, 0.2)[0])
    n_counted = sum(src_items[1].shape[0] for src_items in P.launches)
    n_kernel = sum(cb.last["model/" + n]["num"] for k, n in enumerate(m.state_dict()) if k in set(P.rows))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "device": torch.cuda.get_device_name(0),
        "state_dict_entries": len(ref),
        "elements": sum(d["num"] for d in ref.values()),
        "kernel_entries": len(P.rows),
        "kernel_elements": n_kernel,
        "host_rule_entries": len(P.where),
        "launches": len(P.launches),
        "work_items": n_counted,
        "host_copy_bytes": P.buf.numel() * 8,
        "first_epoch_begin_with_plan_build_ms": round(first_ms, 2),
        "rounds": {k: [round(x, 3) for x in v] for k, v in times.items()},
        "native_epoch_begin_ms": round(med["native_epoch_begin_ms"], 3),
        "reference_way_ms": round(med["reference_way_ms"], 2),
        "reference_over_native": round(med["reference_way_ms"] / med["native_epoch_begin_ms"], 1),
        "kernels_us": round(med["kernels_us"], 1),
        "kernels_GBps": round(4 * n_kernel / (med["kernels_us"] * 1e-6) / 1e9, 1),
        "kernels_read_floor_us_at_6.29TBps": round(4 * n_kernel / (MEASURED_TBPS * 1e12) * 1e6, 1),
        "histograms_equal_the_reference_way": same,
        "worst_relative_difference_of_a_sum": worst_sum,
    }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
