"""Optimizer-step timing on one MI355X: unitwise_norm=True of MyNovograd / NovogradApex (csrc/optim_lw.hip) on the real ResNet-50 flat array
(161 tensors, 27 667 slots, 25 557 032 parameter elements) against the unitwise_norm=False step of the same class from the same build — the
yardstick: it moves the same bytes, 4 B / element for the statistic, 20 for the update, 28 with the parameter average.

    python tools/layerwise_unit_step_bench.py --json RUN.json              one process: every case, --rounds alternating rounds
    python tools/layerwise_unit_step_bench.py --existing --json RUN.json   optimizer.step() of the four layer-wise classes only (runs on the parent tree too)
    python tools/layerwise_unit_step_bench.py --runner --json RUN.json     Runner step of ResNet-50 bf16 at bs 192, MyNovograd unit-wise against layer-wise
    python tools/layerwise_unit_step_bench.py --merge DIR --out profiles/layerwise_unit_step.json
                                                                            DIR: new_*.json, parent_*.json, runner_*.json, bench_new_*.json, bench_parent_*.json (the output of bench.py: its first line is read)

Method of tools/layerwise_step_bench.py: a warm-up, then device events around a window of back-to-back launches of at least --window seconds,
the cases alternating inside a round.  One process gives the median over its rounds; the merged file lists per case the median, min and max
over the processes, the ratio to the yardstick and whether the median lies inside the yardstick's own min..max widened by its own spread."""
import argparse
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import time_window  # noqa: E402

EXISTING = {
    "nov": ("NovogradApex", dict(betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01)),
    "mynov": ("MyNovograd", dict(betas=(0.9, 0.99), weight_decay=0.0002)),
    "adamlw": ("AdamLayerwise", dict(betas=(0.9, 0.995), weight_decay=2e-2)),
    "myadai": ("MyAdai", dict(betas=(0.1, 0.99), weight_decay=3e-5, sgd_mom=True, stable_wd=True)),
}


def kernel_part(a, torch):
    import train
    from sota_imagenet_amd import ops, optim
    from sota_imagenet_amd.models import resnet50

    m = resnet50(dtype="fp32").cuda()
    n_real, n_flat = sum(p.numel() for p in m.parameters()), m.flat_params.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    m.flat_grads.copy_(torch.randn(n_flat, device="cuda", generator=gen) * 1e-3)
    p0, ema = m.flat_params.clone(), m.flat_params.clone()

    def make(cls, kw, two_groups=False, with_ema=False, **more):
        groups = train.filter_from_weight_decay(m, ["bn", "bias"]) if two_groups else [{"params": list(m.parameters())}]
        o = getattr(optim, cls)(groups, lr=1e-3, **kw, **more)
        o.attach_model(m)
        if with_ema:
            o.attach_ema(m.flat_params, ema, 0.9993)
        o.step()  # builds the plan
        return o

    cases = [(f"{k}_optimizer_step", make(*EXISTING[k]).step) for k in EXISTING]
    info = {}
    if not a.existing:
        def lw_a(o):
            def f():
                for seg in o._segs:
                    i0, i1 = seg.items
                    ops.lw_sumsq(seg.p if o._param_stat else seg.g, o._items[i0:i1], o._partial[i0:i1], o._sums.numel())
            return f

        def lw_b(o):
            def f():
                for gi, t0, t1 in o._coefs:
                    g = o.param_groups[gi]
                    flags, b1, b2, eps = o._coef_args(g)
                    ops.lw_coef(o._rule, flags, o._partial, o._tensors[t0:t1], o._v[t0:t1], o._coef[t0:t1], o._sums[t0:t1], b1, b2, eps, 1e-3,
                                float(g["weight_decay"]))
            return f

        def lw_c(o):
            def f():
                for seg in o._segs:
                    for gi, i0, i1 in seg.by_group:
                        ops.lw_update(o._rule, seg.p, seg.g, seg.m, o._items[i0:i1], o._coef, 1e-3, wd_eps=o._wd_eps(), ema=seg.ema, ema_decay=0.9993)
            return f

        def un_a(o, unit=True, whole=True):
            nt, ns = o._tensors.shape[0], o._den.numel()

            def f():
                for seg in o._segs:
                    (pa, pb), (wa, wb), k0 = seg.pieces, seg.whole, seg.partial0
                    k1 = k0 + pb - pa
                    src = seg.p if o._param_stat else seg.g
                    if unit:
                        ops.lw_unit_sumsq(src, o._pieces[pa:pb], o._partial[k0:k1], ns)
                    if whole:
                        ops.lw_sumsq(src, o._whole[wa:wb], o._partial[k1:k1 + wb - wa], nt)
            return f

        def un_b(o):
            def f():
                for gi, s0, s1 in o._coefs:
                    _, _, b2, eps = o._coef_args(o.param_groups[gi])
                    ops.lw_unit_coef(o._partial, o._slots[s0:s1], o._v[s0:s1], o._den[s0:s1], o._sums[s0:s1], b2, eps)
            return f

        def un_c(o):
            def f():
                for seg in o._segs:
                    for gi, i0, i1 in seg.by_group:
                        g = o.param_groups[gi]
                        ops.lw_unit_update(o._rule, seg.p, seg.g, seg.m, o._items[i0:i1], o._tensors, o._den, o._coef_args(g)[1], 1e-3,
                                           float(g["weight_decay"]), wd_eps=o._wd_eps(), ema=seg.ema, ema_decay=0.9993)
            return f

        for k in ("mynov", "nov"):
            cls, kw = EXISTING[k]
            lw, lw_e = make(cls, kw), make(cls, kw, with_ema=True)
            un, un_e = make(cls, kw, unitwise_norm=True), make(cls, kw, with_ema=True, unitwise_norm=True)
            un_2 = make(cls, kw, two_groups=True, unitwise_norm=True)
            lw_2 = make(cls, kw, two_groups=True)
            cases += [(f"{k}/layer/sums", lw_a(lw)), (f"{k}/unit/sums", un_a(un)), (f"{k}/unit/sums_units_only", un_a(un, whole=False)),
                      (f"{k}/unit/sums_1d_only", un_a(un, unit=False)),
                      (f"{k}/layer/coef", lw_b(lw)), (f"{k}/unit/coef", un_b(un)),
                      (f"{k}/layer/update", lw_c(lw)), (f"{k}/unit/update", un_c(un)),
                      (f"{k}/layer/update_ema", lw_c(lw_e)), (f"{k}/unit/update_ema", un_c(un_e)),
                      (f"{k}/layer/optimizer_step", lw.step), (f"{k}/unit/optimizer_step", un.step),
                      (f"{k}/layer/optimizer_step_ema", lw_e.step), (f"{k}/unit/optimizer_step_ema", un_e.step),
                      (f"{k}/layer/optimizer_step_two_groups", lw_2.step), (f"{k}/unit/optimizer_step_two_groups", un_2.step)]
            info = dict(slots=int(un._den.numel()), pieces=int(un._pieces.shape[0]), whole_items=int(un._whole.shape[0]),
                        work_items=int(un._items.shape[0]), item_elems=ops.lw_item_elems())
    times = {name: [] for name, _ in cases}
    for _ in range(max(a.rounds, 1)):
        for name, fn in cases:
            m.flat_params.copy_(p0)
            us, _, _ = time_window(fn, max(a.window, 0.2))
            times[name].append(us)
    return dict(device=torch.cuda.get_device_name(0), n_parameter_elements=n_real, tensors=len(list(m.parameters())), rounds=a.rounds, **info,
                us={k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()},
                finite=bool(torch.isfinite(m.flat_params).all()))


def runner_part(a, torch):
    import time

    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.synth import synthetic_batch

    batch = synthetic_batch(a.batch, 224, seed=0, index=0, device="cuda")

    class Loader:
        batch_size = a.batch

        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __iter__(self):
            return iter([batch] * self.n)

    runs = {}
    for name, unit in (("layer", False), ("unit", True)):
        m = resnet50(dtype="bf16").cuda()
        opt = optim.MyNovograd([{"params": list(m.parameters())}], lr=1e-3, betas=(0.9, 0.99), weight_decay=0.0002, unitwise_norm=unit)
        opt.attach_model(m)
        runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[])
        runner.fit(Loader(3), epochs=1)
        runs[name] = (m, runner, [])
    for _ in range(a.rounds):
        for name, (m, runner, ts) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            runner.fit(Loader(a.steps), epochs=1)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.steps * 1e3)
    return dict(model="resnet50 bf16, MyNovograd (recipe 48's values)", batch=a.batch, image_size=224, steps=a.steps, rounds=a.rounds,
                ms_per_step={k: dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3)) for k, (_, _, ts) in runs.items()},
                finite=all(bool(torch.isfinite(m.flat_params).all()) for m, _, _ in runs.values()))


def _pool(runs, key):
    meds = [r["us"][key]["median"] for r in runs if key in r["us"]]
    if not meds:
        return None
    return dict(median=round(statistics.median(meds), 2), min=round(min(r["us"][key]["min"] for r in runs), 2),
                max=round(max(r["us"][key]["max"] for r in runs), 2), process_medians=meds)


def _verdict(x, lo, hi, widen=0.0):
    return "within" if lo - widen <= x <= hi + widen else ("below (faster)" if x < lo else "above (slower)")


def merge(a):
    load = lambda pat: [json.load(open(f)) for f in sorted(glob.glob(os.path.join(a.merge, pat)))]  # noqa: E731
    new, parent, runner = load("new_*.json"), load("parent_*.json"), load("runner_*.json")
    res = dict(what="unitwise_norm=True of MyNovograd / NovogradApex against the unitwise_norm=False step of the same class and build, one MI355X, "
                    "one session, one fresh process per run, the runs of the two trees alternating",
               device=new[0]["device"], processes=dict(new=len(new), parent=len(parent)), rounds_per_process=new[0]["rounds"],
               **{k: new[0][k] for k in ("n_parameter_elements", "tensors", "slots", "pieces", "whole_items", "work_items", "item_elems")})
    stages = {}
    for k in ("mynov", "nov"):
        for st in ("sums", "coef", "update", "update_ema", "optimizer_step", "optimizer_step_ema", "optimizer_step_two_groups"):
            y, u = _pool(new, f"{k}/layer/{st}"), _pool(new, f"{k}/unit/{st}")
            spread = y["max"] - y["min"]
            stages[f"{k}/{st}"] = dict(yardstick_layerwise=y, unitwise=u, ratio=round(u["median"] / y["median"], 3),
                                       unit_median_vs_yardstick_min_max_widened_by_its_spread=_verdict(u["median"], y["min"], y["max"], spread))
        for st in ("sums_units_only", "sums_1d_only"):
            stages[f"{k}/{st}"] = dict(unitwise=_pool(new, f"{k}/unit/{st}"))
        step, coef = stages[f"{k}/optimizer_step"]["unitwise"]["median"], stages[f"{k}/coef"]["unitwise"]["median"]
        stages[f"{k}/coef"]["share_of_unit_optimizer_step"] = round(coef / step, 3)
    res["us_per_step"] = stages
    ab = {}
    for k in EXISTING:
        p, n = _pool(parent, f"{k}_optimizer_step"), _pool(new, f"{k}_optimizer_step")
        ab[f"{k}_optimizer_step (us)"] = dict(parent=p, new=n, new_median_vs_parent_min_max=_verdict(n["median"], p["min"], p["max"]),
                                              parent_process_spread=round(max(p["process_medians"]) - min(p["process_medians"]), 2))
    bench = {}
    for side in ("parent", "new"):
        vals = [json.loads(open(f).readline())["ms_per_step"] for f in sorted(glob.glob(os.path.join(a.merge, f"bench_{side}_*.json")))]
        if vals:
            bench[side] = dict(ms_per_step=vals, median=round(statistics.median(vals), 3), min=min(vals), max=max(vals))
    if len(bench) == 2:
        bench["new_median_vs_parent_min_max"] = _verdict(bench["new"]["median"], bench["parent"]["min"], bench["parent"]["max"])
        ab["bench.py --gpus 1 (ms per step)"] = bench
    res["parent_against_new"] = ab
    if runner:
        res["runner_step"] = runner if len(runner) > 1 else runner[0]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="where one process writes its result")
    ap.add_argument("--out", default=None, help="where --merge writes the summary")
    ap.add_argument("--merge", default=None, help="directory of per-process results")
    ap.add_argument("--existing", action="store_true", help="optimizer.step() of the four layer-wise classes only")
    ap.add_argument("--runner", action="store_true")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per case and round (>= 0.2)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args(argv)
    if a.merge:
        return merge(a)
    import torch

    assert torch.cuda.is_available(), "needs the MI355X"
    res = runner_part(a, torch) if a.runner else kernel_part(a, torch)
    line = json.dumps(res, indent=1)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
