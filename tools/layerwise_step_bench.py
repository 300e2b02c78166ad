"""Optimizer-step timing on one MI355X: the three stages of the layer-wise optimizers (csrc/optim_lw.hip) on the real ResNet-50 flat array
(161 tensors, 25 557 032 parameter elements), with adam_kernel timed in the same session as the yardstick.

    python tools/layerwise_step_bench.py [--out profiles/layerwise_step.json]

Method of tools/optim_step_bench.py: a warm-up, then device events around a window of back-to-back launches of at least --window seconds.
Every case is timed --rounds times, the cases alternating inside a round; the JSON holds the median and the min / max of the rounds.
Traffic per element: Adam 28 B; stage (a) 4 B (the gradient, or the parameter for MyNovograd), stage (c) 20 B (p, m read + write, g read),
28 B with the average: 24 B a step, 32 B with the average.  Stage (b) reads the partial sums (one double per work item) only.
The stages are timed through sota_imagenet_amd.ops on the plan an optimizer built; `*_optimizer_step` is optimizer.step() itself, the 161
Python step counters included."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import MEASURED_TBPS, SPEC_TBPS, time_window  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per case and round (>= 0.2)")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args(argv)
    import torch

    import train
    from sota_imagenet_amd import ops, optim
    from sota_imagenet_amd.models import resnet50

    assert torch.cuda.is_available(), "needs the MI355X"
    m = resnet50(dtype="fp32").cuda()
    n_real = sum(p.numel() for p in m.parameters())
    n_flat = m.flat_params.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    m.flat_grads.copy_(torch.randn(n_flat, device="cuda", generator=gen) * 1e-3)
    p0, ema = m.flat_params.clone(), m.flat_params.clone()

    def make(cls, two_groups=False, with_ema=False, **kw):
        groups = train.filter_from_weight_decay(m, ["bn", "bias"]) if two_groups else [{"params": list(m.parameters())}]
        o = getattr(optim, cls)(groups, lr=1e-3, **kw)
        o.attach_model(m)
        if with_ema:
            o.attach_ema(m.flat_params, ema, 0.9993)
        o.step()  # builds the plan
        return o

    opts = {
        "adamlw": make("AdamLayerwise", betas=(0.9, 0.995), weight_decay=2e-2),
        "adamlw_ema": make("AdamLayerwise", with_ema=True, betas=(0.9, 0.995), weight_decay=2e-2),
        "adamlw_two_groups": make("AdamLayerwise", two_groups=True, betas=(0.9, 0.995), weight_decay=2e-2),
        "nov_wd_eps": make("NovogradApex", betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01),
        "mynov": make("MyNovograd", betas=(0.9, 0.99), weight_decay=0.002),
        "myadai": make("MyAdai", betas=(0.1, 0.99), weight_decay=3e-5, sgd_mom=True, stable_wd=True),
    }
    s1, s2 = torch.zeros_like(p0), torch.zeros_like(p0)
    step = [0]

    def adam():
        ops.adam_step(m.flat_params, m.flat_grads, s1, s2, step[0] % 1000, 1e-3, (0.9, 0.999), 1e-8, 5e-2, decoupled=True)
        step[0] += 1

    def stage_a(o):
        def f():
            for seg in o._segs:
                i0, i1 = seg.items
                ops.lw_sumsq(seg.p if o._param_stat else seg.g, o._items[i0:i1], o._partial[i0:i1], o._sums.numel())
        return f

    def stage_b(o):
        def f():
            for gi, t0, t1 in o._coefs:
                g = o.param_groups[gi]
                flags, b1, b2, eps = o._coef_args(g)
                ops.lw_coef(o._rule, flags, o._partial, o._tensors[t0:t1], o._v[t0:t1], o._coef[t0:t1], o._sums[t0:t1], b1, b2, eps, 1e-3,
                            float(g["weight_decay"]), mean=1e-3)
        return f

    def stage_c(o):
        def f():
            for seg in o._segs:
                for gi, i0, i1 in seg.by_group:
                    ops.lw_update(o._rule, seg.p, seg.g, seg.m, o._items[i0:i1], o._coef, 1e-3, wd_eps=o._wd_eps(), ema=seg.ema, ema_decay=0.9993)
        return f

    def stages(o):
        fa, fb, fc = stage_a(o), stage_b(o), stage_c(o)

        def f():
            fa()
            fb()
            fc()
        return f

    B = n_real
    cases = [("adam_kernel", adam, 28 * n_flat)]  # (adam_kernel sweeps the whole flat array, padding included)
    o = opts["adamlw"]
    cases += [("lw_sumsq_kernel", stage_a(o), 4 * B), ("lw_coef_kernel", stage_b(o), 0), ("lw_update_kernel", stage_c(o), 20 * B)]
    for name, o in opts.items():
        cases.append((f"{name}_three_stages", stages(o), (32 if name.endswith("_ema") else 24) * B))
    cases.append(("adamlw_optimizer_step", opts["adamlw"].step, 24 * B))
    times = {name: [] for name, _, _ in cases}
    for _ in range(max(a.rounds, 1)):
        for name, fn, _ in cases:
            m.flat_params.copy_(p0)
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
    res = {
        "device": torch.cuda.get_device_name(0),
        "n_parameter_elements": n_real,
        "n_flat_elements": n_flat,
        "tensors": len(list(m.parameters())),
        "item_elems": ops.lw_item_elems(),
        "work_items": int(opts["adamlw"]._items.shape[0]),
        "launches_per_step": {"one_group": 3, "two_groups": 5},
        "kernels": out,
        "us_vs_adam_kernel": {k: round(c["us_per_step"] / out["adam_kernel"]["us_per_step"], 3) for k, c in out.items()},
        "GBps_vs_adam_kernel": {k: round(c["GBps"] / out["adam_kernel"]["GBps"], 3) for k, c in out.items() if "GBps" in c},
        "finite": bool(torch.isfinite(m.flat_params).all()),
    }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
