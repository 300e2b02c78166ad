"""SAM timing on one MI355X: the stages of csrc/optim_sam_lw.hip on the real ResNet-50 flat array (161 tensors, 25 557 032 parameter elements),
layer-wise and unit-wise, with the three sweep kernels of SAMOriginal (csrc/optim_sam.hip) timed in the same run as the yardsticks — the
layer-wise sums move the bytes of sam_sumsq_kernel (8 B / element), the perturbation those of sam_perturb_kernel (16 B / element) — and the
Runner step of ResNet-50 bf16 under AdamLayerwise at batch 256, 224 px with SAM(unitwise=True) against the same step with SAMOriginal.

    python tools/sam_lw_step_bench.py [--out profiles/sam_lw_step.json]

Kernel method of tools/sam_step_bench.py: a warm-up, then device events around a window of back-to-back launches of at least --window seconds;
every case --rounds times, the cases alternating inside a round; the JSON holds the median and the min / max of the rounds.  The unit reduction
is timed with one wave per piece (threads_per_piece 64) and with one workgroup per piece (256).  The Runner figure is wall time per step over
--steps steps after a warm-up fit, one synthetic batch reused, host and device together, the two callbacks alternating inside a round."""
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
    from sota_imagenet_amd.callbacks import SAM, SAMOriginal
    from sota_imagenet_amd.models import resnet50

    m = resnet50(dtype="fp32").cuda()
    params = list(m.parameters())
    n_real, n_flat = sum(p.numel() for p in params), m.flat_params.numel()
    n_unit = sum(p.numel() for p in params if p.ndim > 1)
    gen = torch.Generator(device="cuda").manual_seed(0)
    m.flat_grads.copy_(torch.randn(n_flat, device="cuda", generator=gen) * 1e-3)
    p0 = m.flat_params.clone()
    orig, lw, un = SAMOriginal(), SAM(unitwise=False), SAM(unitwise=True)
    for c in (orig, lw, un):
        c.build_plan(params)
    (oseg,) = orig._segs
    ofp, ofg, ofe, (oi0, oi1) = oseg.p, oseg.g, oseg.eps, oseg.items

    def sums(c, tpp=ops.SAM_THREADS_PER_PIECE, unit=True, whole=True):
        nt, ns = c._tensors.shape[0], c._coef.numel()
        for seg in c._segs:
            (pa, pb), (wa, wb), k0 = seg.pieces, seg.whole, seg.partial0
            k1 = k0 + pb - pa
            if pb > pa and unit:
                ops.sam_unit_sumsq(seg.p, seg.g, c._pieces[pa:pb], c._partial[2 * k0:2 * k1], ns, threads_per_piece=tpp)
            if wb > wa and whole:
                ops.sam_lw_sumsq(seg.p, seg.g, c._whole[wa:wb], c._partial[2 * k1:2 * (k1 + wb - wa)], nt)

    def coef(c):
        ops.sam_lw_coef(c._partial, c._slots, c._coef, c._norms)

    def perturb(c):
        for seg in c._segs:
            i0, i1 = seg.items
            ops.sam_lw_perturb(seg.p, seg.g, seg.eps, c._items[i0:i1], c._tensors, c._coef, c.rho)

    def stages(c):
        sums(c)
        coef(c)
        perturb(c)
        for seg in c._segs:
            i0, i1 = seg.items
            ops.sam_restore(seg.p, seg.eps, c._items[i0:i1], c._tensors.shape[0])

    B = n_real
    n1d = n_real - n_unit
    cases = [
        ("sam_sumsq_kernel", lambda: ops.sam_sumsq(ofp, ofg, orig._items[oi0:oi1], orig._kind, orig._partial[oi0:oi1], orig.eta), 8 * B),
        ("sam_perturb_kernel", lambda: ops.sam_perturb(ofp, ofg, ofe, orig._items[oi0:oi1], orig._kind, orig._out, orig.eta), 16 * B),
        ("sam_restore_kernel", lambda: ops.sam_restore(ofp, ofe, orig._items[oi0:oi1], orig._kind.numel()), 12 * B),
        ("layer/sam_lw_sumsq_kernel", lambda: sums(lw), 8 * B),
        ("layer/sam_lw_coef_kernel", lambda: coef(lw), 0),
        ("layer/sam_lw_perturb_kernel", lambda: perturb(lw), 16 * B),
        ("layer/four_stages", lambda: stages(lw), 36 * B),
        ("unit/sam_unit_sumsq_kernel<64>", lambda: sums(un, 64, whole=False), 8 * n_unit),
        ("unit/sam_unit_sumsq_kernel<256>", lambda: sums(un, 256, whole=False), 8 * n_unit),
        ("unit/sam_lw_sumsq_kernel_1d", lambda: sums(un, unit=False), 8 * n1d),
        ("unit/sam_lw_coef_kernel", lambda: coef(un), 0),
        ("unit/sam_lw_perturb_kernel", lambda: perturb(un), 16 * B),
        ("unit/five_stages", lambda: stages(un), 36 * B),
    ]
    times = {name: [] for name, _, _ in cases}
    for _ in range(max(a.rounds, 1)):
        for name, fn, _ in cases:
            m.flat_params.copy_(p0)
            ops.sam_sumsq(ofp, ofg, orig._items[oi0:oi1], orig._kind, orig._partial[oi0:oi1], orig.eta)
            ops.sam_scale(orig._partial, orig.rho, orig._out)
            for c in (lw, un):  # valid coefficients for the perturbation, whichever case runs
                sums(c)
                coef(c)
            for c in (orig, lw, un):
                c._eps[0].zero_()
            us, iters, secs = time_window(fn, max(a.window, 0.2))
            times[name].append(us)
    m.flat_params.copy_(p0)
    out = {}
    for name, _, nbytes in cases:
        ts = times[name]
        c = dict(us_per_step=round(statistics.median(ts), 2), us_min=round(min(ts), 2), us_max=round(max(ts), 2), rounds=len(ts), bytes_per_step=nbytes)
        if nbytes:
            gbps = nbytes / (c["us_per_step"] * 1e-6) / 1e9
            c.update(GBps=round(gbps, 1), frac_of_spec_8TBps=round(gbps / (SPEC_TBPS * 1e3), 3),
                     **{"frac_of_measured_6.29TBps": round(gbps / (MEASURED_TBPS * 1e3), 3)})
        out[name] = c

    def ratio(x, y):
        return round(out[x]["us_per_step"] / out[y]["us_per_step"], 3)

    return {
        "n_parameter_elements": n_real,
        "n_flat_elements": n_flat,
        "n_unitwise_elements": n_unit,
        "tensors": len(params),
        "item_elems": ops.lw_item_elems(),
        "work_items": int(lw._items.shape[0]),
        "layer": {"slots": int(lw._coef.numel()), "launches_per_step": 4},
        "unit": {"slots": int(un._coef.numel()), "pieces": int(un._pieces.shape[0]), "whole_tensor_items": int(un._whole.shape[0]),
                 "launches_per_step": 5, "threads_per_piece_used": ops.SAM_THREADS_PER_PIECE},
        "kernels": out,
        "us_vs_yardstick": {
            "layer/sam_lw_sumsq_kernel / sam_sumsq_kernel": ratio("layer/sam_lw_sumsq_kernel", "sam_sumsq_kernel"),
            "layer/sam_lw_perturb_kernel / sam_perturb_kernel": ratio("layer/sam_lw_perturb_kernel", "sam_perturb_kernel"),
            "unit/sam_lw_perturb_kernel / sam_perturb_kernel": ratio("unit/sam_lw_perturb_kernel", "sam_perturb_kernel"),
        },
        "unit_reduction_GBps_vs_sam_sumsq_kernel": {k: round(out[k]["GBps"] / out["sam_sumsq_kernel"]["GBps"], 3)
                                                    for k in ("unit/sam_unit_sumsq_kernel<64>", "unit/sam_unit_sumsq_kernel<256>")},
    }


def runner_part(a, torch):
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAM, SAMOriginal
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

    runs = {}
    for name, clb in (("with_SAMOriginal", SAMOriginal()), ("with_SAM_unitwise", SAM(unitwise=True, rho=0.001))):
        m = resnet50(dtype="bf16").cuda()
        opt = optim.AdamLayerwise([{"params": list(m.parameters())}], lr=1e-4, betas=(0.9, 0.995), weight_decay=2e-2)
        runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[clb])
        runner.fit(Loader(3), epochs=1)  # contexts, plans, SAMOriginal's skipped first step
        runs[name] = (m, clb, runner, [])
    torch.cuda.synchronize()
    for _ in range(max(a.rounds, 1)):
        for name, (m, clb, runner, ts) in runs.items():
            t0 = time.perf_counter()
            runner.fit(Loader(a.steps), epochs=1)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / a.steps * 1e3)
    res = {}
    for name, (m, clb, runner, ts) in runs.items():
        res[name] = dict(ms_per_step=round(statistics.median(ts), 2), ms_min=round(min(ts), 2), ms_max=round(max(ts), 2), rounds=len(ts),
                         images_per_sec=round(a.batch / statistics.median(ts) * 1e3, 1), finite=bool(torch.isfinite(m.flat_params).all()),
                         second_forwards=clb.forwards)
    res["step_time_ratio_SAM_unitwise_vs_SAMOriginal"] = round(res["with_SAM_unitwise"]["ms_per_step"] / res["with_SAMOriginal"]["ms_per_step"], 3)
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
