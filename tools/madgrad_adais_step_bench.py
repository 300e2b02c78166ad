"""Optimizer-step timing on one MI355X: the MADGRAD kernel (with and without the parameter average) and the three AdaiS stages
(csrc/optim.hip) on the 25 557 032-element ResNet-50 parameter array, with adam_kernel timed in the same session as the yardstick.

    python tools/madgrad_adais_step_bench.py [--out profiles/madgrad_adais_step.json]

Method of tools/optim_step_bench.py: a warm-up, then device events around a window of back-to-back launches of at least --window
seconds.  Traffic per element: Adam 28 B; MADGRAD 32 B (p, grad_sum_sq, s read + write, g, x0 read), 40 B with the average; AdaiS
12 B (moments: g read, v read + write) + 32 B (step: p, m, beta1_prod read + write, g, v read) = 44 B, 52 B with the average."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import MEASURED_TBPS, N_ELEM, SPEC_TBPS, time_window  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per case (>= 0.2)")
    a = ap.parse_args(argv)
    import torch

    from sota_imagenet_amd import ops

    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(N_ELEM, device=dev, generator=gen) * 0.05
    gr = torch.randn(N_ELEM, device=dev, generator=gen) * 1e-3
    s1, s2, s3, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone(), p.clone()
    ws = torch.zeros(ops.adais_workspace_elems(N_ELEM), dtype=torch.float64, device=dev)
    mean = torch.ones(1, device=dev)
    step = [0]

    def reset(kind):
        p.copy_(ema)
        s1.zero_()
        if kind == "adais":
            s2.fill_(1e-3)
            s3.fill_(1.0)
        else:
            s2.zero_()
            s3.copy_(p)
        step[0] = 0

    def adam(e=None):
        def f():
            ops.adam_step(p, gr, s1, s2, step[0] % 1000, 1e-3, (0.9, 0.999), 1e-8, 5e-2, decoupled=True, ema=e, ema_decay=0.9999)
            step[0] += 1
        return f

    def madgrad(e=None):
        def f():  # s1 = grad_sum_sq, s2 = s, s3 = x0
            ops.madgrad_step(p, gr, s1, s2, s3, step[0] % 1000, 2e-3, 0.9, 1e-4, 1e-6, ema=e, ema_decay=0.9993)
            step[0] += 1
        return f

    def moments():
        ops.adais_moments(gr, s2, step[0] % 1000 + 1, 0.99, ws)

    def the_mean():
        ops.adais_mean(ws, N_ELEM, mean)

    def adais_update(e=None):
        def f():  # s1 = exp_avg, s2 = exp_avg_sq, s3 = beta1_prod
            ops.adais_step(p, gr, s1, s2, s3, mean, step[0] % 1000 + 1, 0.1, (0.1, 0.99), 1e-3, 1e-3, ema=e, ema_decay=0.9993)
        return f

    def adais(e=None):
        upd = adais_update(e)

        def f():
            moments()
            the_mean()
            upd()
            step[0] += 1
        return f

    cases = {}
    for name, kind, fn, bpe in (("adam_kernel", "adam", adam(), 28),
                                ("madgrad_kernel", "madgrad", madgrad(), 32),
                                ("madgrad_kernel_ema", "madgrad", madgrad(ema), 40),
                                ("adais_three_stages", "adais", adais(), 44),
                                ("adais_three_stages_ema", "adais", adais(ema), 52),
                                ("adais_moments_kernel", "adais", moments, 12),
                                ("adais_mean_kernel", "adais", the_mean, 0),
                                ("adais_step_kernel", "adais", adais_update(), 32)):
        reset(kind)
        if kind == "adais":  # a mean for the stage that is timed alone
            moments()
            the_mean()
        us, iters, secs = time_window(fn, max(a.window, 0.2))
        c = dict(us_per_step=round(us, 2), bytes_per_step=bpe * N_ELEM, iters=iters, window_s=round(secs, 3))
        if bpe:
            gbps = c["bytes_per_step"] / (us * 1e-6) / 1e9
            c.update(GBps=round(gbps, 1), frac_of_spec_8TBps=round(gbps / (SPEC_TBPS * 1e3), 3),
                     **{"frac_of_measured_6.29TBps": round(gbps / (MEASURED_TBPS * 1e3), 3)})
        c["finite"] = bool(torch.isfinite(p).all())
        cases[name] = c
    yard = cases["adam_kernel"]["GBps"]
    res = {
        "device": torch.cuda.get_device_name(0),
        "n_elements": N_ELEM,
        "kernels": cases,
        "GBps_vs_adam_kernel": {k: round(c["GBps"] / yard, 3) for k, c in cases.items() if "GBps" in c},
        "adais_mean_share_of_step": round(cases["adais_mean_kernel"]["us_per_step"] / cases["adais_three_stages"]["us_per_step"], 4),
        "note": "every case moves more than the 256 MiB Infinity Cache per step except adais_mean_kernel (128 KiB of partial sums): HBM rates",
    }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
