"""Optimizer-step timing on one MI355X: the fused SGD kernel against the fused Adam / AdamW kernel (csrc/optim.hip) on the
25 557 032-element ResNet-50 parameter array, and torch's foreach AdamW over the 161 parameter views of a resnet50(), plus the
whole bf16 bs-256 training step under native SGD, native AdamW and torch's AdamW.

    python tools/optim_step_bench.py [--out profiles/adamw_step.json]
    python tools/optim_step_bench.py --train-steps 3 --opt adamw [--wd-groups]     (a few training steps, for a kernel trace)

Each kernel case: a warm-up, then device events around a window of back-to-back launches of at least --window seconds.
Traffic per element: SGD 20 B (p, m read + write, g read), Adam 28 B (p, m, v read + write, g read), Adam + average 36 B; the
foreach row is credited with the same 28 B (what it must move at least).  716 MB of Adam traffic is larger than the 256 MiB
Infinity Cache, so the rate is an HBM rate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ELEM = 25557032
SPEC_TBPS = 8.0        # MI355X HBM3E spec
MEASURED_TBPS = 6.29   # sustained copy rate measured on this part (MI355X_MICROARCH.md)


def time_window(fn, window, warmup=5):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 5
    iters = max(10, int(1.25 * window / max(per, 1e-6)) + 1)  # (host-timed estimate: margin so the device window is >= window)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b)
    return ms * 1e3 / iters, iters, ms / 1e3


def kernel_cases(window):
    import torch

    from sota_imagenet_amd import ops
    from sota_imagenet_amd.models import resnet50

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(N_ELEM, device=dev, generator=g) * 0.05
    gr = torch.randn(N_ELEM, device=dev, generator=g) * 1e-3
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    step = [0]

    def adam(e=None):
        def f():
            ops.adam_step(p, gr, m, v, step[0] % 1000, 1e-3, (0.9, 0.999), 1e-8, 5e-2, decoupled=True, ema=e, ema_decay=0.9999)
            step[0] += 1
        return f

    cases = {}
    for name, fn, bpe in (("sgd_kernel", lambda: ops.sgd_step(p, gr, m, 0.0, 0.9, 3e-5), 20),
                          ("adam_kernel", adam(), 28),
                          ("adam_kernel_ema", adam(ema), 36)):
        us, iters, secs = time_window(fn, window)
        cases[name] = dict(us_per_step=round(us, 2), bytes_per_step=bpe * N_ELEM, iters=iters, window_s=round(secs, 3))
    del p, gr, m, v, ema
    model = resnet50(dtype="fp32").cuda()
    params = list(model.parameters())
    assert len(params) == 161
    for q in params:
        q.grad = q.grad if q.grad is not None else torch.zeros_like(q)
    opt = torch.optim.AdamW(params, lr=1e-3, weight_decay=5e-2, foreach=True)
    us, iters, secs = time_window(opt.step, window)
    cases["torch_foreach_adamw_161_tensors"] = dict(us_per_step=round(us, 2), bytes_per_step=28 * sum(q.numel() for q in params),
                                                     iters=iters, window_s=round(secs, 3))
    for c in cases.values():
        gbps = c["bytes_per_step"] / (c["us_per_step"] * 1e-6) / 1e9
        c["GBps"] = round(gbps, 1)
        c["frac_of_spec_8TBps"] = round(gbps / (SPEC_TBPS * 1e3), 3)
        c["frac_of_measured_6.29TBps"] = round(gbps / (MEASURED_TBPS * 1e3), 3)
    del model, opt
    torch.cuda.empty_cache()
    return cases


def make_opt(kind, model, wd_groups):
    import torch

    from sota_imagenet_amd import optim

    sys.path.insert(0, ROOT)
    import train

    params = train.filter_from_weight_decay(model, ["bn", "bias"]) if wd_groups else [{"params": list(model.parameters())}]
    if kind == "sgd":
        opt = optim.SGD(params, lr=0.1, momentum=0.9, weight_decay=3e-5)
    elif kind == "adamw":
        opt = optim.AdamW(params, lr=1e-3, weight_decay=5e-2)
    else:
        return torch.optim.AdamW(params, lr=1e-3, weight_decay=5e-2, foreach=True)
    opt.attach_model(model)
    return opt


def train_step_ms(kind, steps, N=256, S=224, wd_groups=False, warmup=3):
    import torch

    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.models import resnet50
    from sota_imagenet_amd.synth import synthetic_batch

    model = resnet50(dtype="bf16").cuda()
    crit = CrossEntropyLoss(smoothing=0.1)
    opt = make_opt(kind, model, wd_groups)
    data, target = synthetic_batch(N, S, seed=0, index=0, device="cuda")
    model.train()

    def step():
        loss = crit(model(data), target)
        opt.zero_grad(set_to_none=kind == "torch_adamw")
        loss.backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / steps
    ok = bool(torch.isfinite(model.flat_params).all())
    del model, opt
    torch.cuda.empty_cache()
    return round(ms, 3), ok


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per kernel case (>= 0.2)")
    ap.add_argument("--steps", type=int, default=20, help="timed bf16 bs-256 training steps per optimizer")
    ap.add_argument("--train-steps", type=int, default=0, help="only run this many training steps of --opt (kernel-trace mode)")
    ap.add_argument("--opt", default="adamw", choices=["sgd", "adamw", "torch_adamw"])
    ap.add_argument("--warmup", type=int, default=3, help="untimed training steps first (kernel-trace mode)")
    ap.add_argument("--kernels-only", action="store_true", help="only the four optimizer-step cases")
    ap.add_argument("--wd-groups", action="store_true", help="the two param groups of train.filter_from_weight_decay")
    a = ap.parse_args(argv)
    import torch

    assert torch.cuda.is_available(), "needs the MI355X"
    if a.train_steps:
        ms, ok = train_step_ms(a.opt, a.train_steps, wd_groups=a.wd_groups, warmup=a.warmup)
        print(json.dumps({"opt": a.opt, "wd_groups": a.wd_groups, "train_steps": a.train_steps, "warmup_steps": a.warmup, "ms_per_step": ms,
                          "finite": ok}))
        return
    cases = kernel_cases(max(a.window, 0.2))
    if a.kernels_only:
        print(json.dumps({"lib": os.environ.get("MI355RN_LIB", "default"), **{k: (v["us_per_step"], v["GBps"]) for k, v in cases.items()}}))
        return
    steps = {}
    for kind in ("sgd", "adamw", "torch_adamw"):
        ms, ok = train_step_ms(kind, a.steps)
        steps[kind] = dict(ms_per_step=ms, finite=ok)
    res = {
        "device": torch.cuda.get_device_name(0),
        "n_elements": N_ELEM,
        "kernels": cases,
        "adam_vs_sgd_GBps": round(cases["adam_kernel"]["GBps"] / cases["sgd_kernel"]["GBps"], 3),
        "adam_ema_vs_sgd_GBps": round(cases["adam_kernel_ema"]["GBps"] / cases["sgd_kernel"]["GBps"], 3),
        "train_step_bf16_bs256_224px": steps,
        "adamw_minus_sgd_step_ms": round(steps["adamw"]["ms_per_step"] - steps["sgd"]["ms_per_step"], 3),
        "torch_adamw_minus_native_adamw_step_ms": round(steps["torch_adamw"]["ms_per_step"] - steps["adamw"]["ms_per_step"], 3),
        "note": "716 MB of Adam traffic per step > 256 MiB Infinity Cache: HBM-bound; foreach row credited with 28 B/element",
    }
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
