"""What profiles/grad_dist.json holds: one logged step of callbacks.GradDistributionTB on the ResNet-50 flat arrays (25.5 M parameters, AdamW state after
one step on synthetic gradients, subsample 10) — the whole step by the host clock (it ends in the callback's one copy to the host) and, by device
events, every tag and the two kernels alone; the same step by the reference's method (sota_imagenet/callbacks.py:44-60 restated with torch sorts on
the same GPU, up to the log10 array it hands to the histogram); the time to read each array once at the achievable HBM rate; the counting kernel on
arrays of the same length that are all equal (every lane on one bin), spread evenly over the bins, and the trained-like parameters; and the cost per
training step at log_every 50 against a given step time.  Medians of --rounds timed runs after --warmup untimed ones.
    python tools/grad_dist_measure.py --out FILE [--bench-ms MS_PER_STEP] [--commit HASH]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sota_imagenet_amd import callbacks, item_plan, ops, optim  # noqa: E402
from sota_imagenet_amd.fit_wrapper import RunnerState  # noqa: E402
from sota_imagenet_amd.models import resnet50  # noqa: E402

HBM_ACHIEVABLE = 6.29e12  # bytes / s: the measured float4 copy rate of the MI355X (79 % of the 8.0 TB/s of the data sheet)


def _events(fn, warmup, rounds):
    """median, min, max of fn's device time in ms"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def _wall(fn, warmup, rounds):
    """the same by the host clock, for work that ends in a synchronising copy"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def _reference_method(tensors, s):
    """the reference's gathering for one tag, on the device the tensors live on"""
    kept = torch.cat([t.flatten().abs().sort().values[::s] for t in tensors])
    return kept.sort().values[::s].log10().clamp_min(-15)


def _commit(given):
    if given:
        return given
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return "unknown (not a git checkout)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--subsample", type=int, default=10)
    ap.add_argument("--log-every", type=int, default=50)
    ap.add_argument("--bench-ms", type=float, default=None, help="ms per training step of bench.py on the same machine")
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    s = a.subsample
    m = resnet50(dtype="fp32").cuda()
    opt = optim.AdamW([{"params": list(m.parameters())}], lr=1e-3, weight_decay=2e-2)
    opt.attach_model(m)
    g = torch.zeros_like(m.flat_grads)
    gen = torch.Generator(device=dev).manual_seed(5)
    g.copy_(torch.randn(g.shape, generator=gen, device=dev) * 1e-2)
    m.flat_grads.copy_(g)
    opt.zero_grad()
    opt.step()
    cb = callbacks.GradDistributionTB(log_every=a.log_every, subsample=s)
    st = RunnerState(model=m, optimizer=opt)
    st.step, st.is_train = 0, True
    cb.set_state(st)
    out = {"what": __doc__.split("    python")[0].strip(), "commit": _commit(a.commit), "device": torch.cuda.get_device_name(0),
           "subsample": s, "log_every": a.log_every, "warmup": a.warmup, "rounds": a.rounds, "item_elems": ops.lw_item_elems(),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE}
    out["native_logged_step_wall"] = _wall(cb.log, a.warmup, a.rounds)
    tagged = cb._tensors()
    out["tensors_per_tag"] = len(tagged[0][1])
    out["elements_per_tag"] = sum(t.numel() for t in tagged[-1][1])
    out["tags"] = {}
    total_ref = 0.0
    for k, ((tag, launches, rep, (r0, r1)), (_, tensors)) in enumerate(zip(cb._tags, tagged)):
        hist, counts = cb._hist[r0:r1], cb._counts[k]

        def count_pass():
            for src, items in launches:
                ops.absbin_hist(src, items, hist)

        def native():
            hist.zero_()
            count_pass()
            ops.subsample_counts(hist, rep, s, counts)

        read = 4 * sum(int((items[:, 1] & 0xFFFFFFFF).sum()) for _, items in launches)  # the lengths of the work items
        row = dict(bytes_read=read, work_items=sum(int(i.shape[0]) for _, i in launches), launches=len(launches),
                   native=_events(native, a.warmup, a.rounds), absbin_hist=_events(count_pass, a.warmup, a.rounds),
                   subsample_counts=_events(lambda: ops.subsample_counts(hist, rep, s, counts), a.warmup, a.rounds),
                   reference_method=_events(lambda: _reference_method(tensors, s), 1, 5))
        row["read_floor_ms"] = 1e3 * read / HBM_ACHIEVABLE
        row["absbin_hist_over_read_floor"] = row["absbin_hist"]["median_ms"] / row["read_floor_ms"]
        row["reference_over_native"] = row["reference_method"]["median_ms"] / row["native"]["median_ms"]
        total_ref += row["reference_method"]["median_ms"]
        out["tags"][tag] = row
    out["native_sum_of_tags_ms"] = sum(r["native"]["median_ms"] for r in out["tags"].values())
    out["reference_method_sum_of_tags_ms"] = total_ref
    out["reference_over_native_logged_step"] = total_ref / out["native_logged_step_wall"]["median_ms"]
    out["read_floor_sum_ms"] = sum(r["read_floor_ms"] for r in out["tags"].values())

    # the counting kernel alone on one array of the parameters' length: the contention cases
    n = out["elements_per_tag"]
    items = item_plan.pack_records(item_plan.plan_items([(0, n)], ops.lw_item_elems())[0], dev)
    hist = torch.zeros(1, ops.ABSBIN_BINS, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(6)
    arrays = {
        "all_equal": torch.full((n,), 1e-3, device=dev),
        "spread_over_the_bins": torch.pow(10.0, torch.rand(n, generator=gen, device=dev) * 19.0 - 15.0),
        "normal_0.02": torch.randn(n, generator=gen, device=dev) * 0.02,
    }
    out["contention"] = {}
    for name, x in arrays.items():
        r = _events(lambda: ops.absbin_hist(x, items, hist), a.warmup, a.rounds)
        hist.zero_()
        ops.absbin_hist(x, items, hist)
        r["bins_used"] = int((hist != 0).sum())
        r["over_read_floor"] = r["median_ms"] / (1e3 * 4 * n / HBM_ACHIEVABLE)
        out["contention"][name] = r
    amort = out["native_logged_step_wall"]["median_ms"] / a.log_every
    out["amortised_ms_per_step"] = amort
    out["reference_method_amortised_ms_per_step"] = total_ref / a.log_every
    if a.bench_ms:
        out["bench_ms_per_step"] = a.bench_ms
        out["amortised_share_of_bench_step"] = amort / a.bench_ms
        out["reference_method_amortised_share_of_bench_step"] = total_ref / a.log_every / a.bench_ms
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
