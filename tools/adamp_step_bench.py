"""Optimizer-step timing on one MI355X: the native AdamP step (csrc/optim_adamp.hip; three stages, 16 + 28 B / element) against the native AdamW
step (csrc/optim.hip; one launch, 28 B / element) on the real ResNet-50 flat array (161 tensors, 25 557 032 parameter elements), in the same
process and from the same build.  By bytes AdamP should cost about 44 / 28 = 1.6 x AdamW plus two small launches; that is a derivation from
traffic, this tool measures.

    python tools/adamp_step_bench.py --out profiles/adamp_step.json

Method of tools/layerwise_step_bench.py: a warm-up, then device events around a window of back-to-back launches of at least --window seconds,
the cases alternating inside a round; per case the median, min and max over --rounds rounds.  The stages of AdamP are timed one by one as well,
so that a ratio far from 1.6 names its stage."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.optim_step_bench import time_window  # noqa: E402

KW = dict(weight_decay=1e-2)  # recipe 51


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="where the result is written")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per case and round (>= 0.2)")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args(argv)
    import torch

    import train
    from sota_imagenet_amd import ops, optim
    from sota_imagenet_amd.models import resnet50

    assert torch.cuda.is_available(), "needs the MI355X"
    m = resnet50(dtype="fp32").cuda()
    n_real, n_flat = sum(p.numel() for p in m.parameters()), m.flat_params.numel()
    gen = torch.Generator(device="cuda").manual_seed(0)
    m.flat_grads.copy_(torch.randn(n_flat, device="cuda", generator=gen) * 1e-3)
    p0, ema = m.flat_params.clone(), m.flat_params.clone()

    def make(cls, two_groups=False, with_ema=False):
        groups = train.filter_from_weight_decay(m, ["bn", "bias"]) if two_groups else [{"params": list(m.parameters())}]
        o = getattr(optim, cls)(groups, lr=1e-3, **KW)
        o.attach_model(m)
        if with_ema:
            o.attach_ema(m.flat_params, ema, 0.9993)
        o.step()  # builds the plan
        return o

    ap_, ap_e, ap_2 = make("AdamP"), make("AdamP", with_ema=True), make("AdamP", two_groups=True)
    aw, aw_e, aw_2 = make("AdamW"), make("AdamW", with_ema=True), make("AdamW", two_groups=True)
    ns = ap_._coef.shape[0]
    adam = dict(step=2, betas=(0.9, 0.999), eps=1e-8)

    def stage_a():
        for seg in ap_._segs:
            for gi, i0, i1, k in seg.sums:
                ops.adamp_unit_sums(seg.p, seg.g, seg.m, seg.v, ap_._sum_pieces[i0:i1], ap_._partial[k:k + i1 - i0], ns, **adam)

    def stage_b():
        for gi, t0, t1 in ap_._groups:
            ops.adamp_coef(ap_._partial, ap_._slots, ap_._decide[t0:t1], ap_._coef, ap_._wdf[t0:t1], ap_._modes[t0:t1], 1e-3, KW["weight_decay"])

    def stage_c(o):
        def f():
            for seg in o._segs:
                for gi, i0, i1 in seg.by_group:
                    ops.adamp_update(seg.p, seg.g, seg.m, seg.v, o._items[i0:i1], o._tensors, o._coef, o._wdf, lr=1e-3, ema=seg.ema,
                                     ema_decay=0.9993, **adam)
        return f

    cases = [("adamw/optimizer_step", aw.step), ("adamp/optimizer_step", ap_.step),
             ("adamw/optimizer_step_ema", aw_e.step), ("adamp/optimizer_step_ema", ap_e.step),
             ("adamw/optimizer_step_two_groups", aw_2.step), ("adamp/optimizer_step_two_groups", ap_2.step),
             ("adamp/unit_sums", stage_a), ("adamp/coef", stage_b), ("adamp/update", stage_c(ap_)), ("adamp/update_ema", stage_c(ap_e))]
    times = {name: [] for name, _ in cases}
    for _ in range(max(a.rounds, 1)):
        for name, fn in cases:
            m.flat_params.copy_(p0)
            us, _, _ = time_window(fn, max(a.window, 0.2))
            times[name].append(us)
    us = {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in times.items()}
    modes = [int(x) for x in ap_.projection_modes.cpu()]
    res = dict(what="AdamP optimizer.step() against the native AdamW step on the ResNet-50 flat fp32 array, one MI355X, one process, the cases "
                    "alternating inside each round; us per call",
               device=torch.cuda.get_device_name(0), n_parameter_elements=n_real, tensors=len(list(m.parameters())), slots=int(ns),
               pieces=int(ap_._sum_pieces.shape[0]), work_items=int(ap_._items.shape[0]), item_elems=ops.lw_item_elems(), rounds=a.rounds,
               tensors_in_mode_0_1_2=[modes.count(x) for x in (0, 1, 2)], us=us,
               ratio_adamp_to_adamw={k: round(us[f"adamp/{k}"]["median"] / us[f"adamw/{k}"]["median"], 3)
                                     for k in ("optimizer_step", "optimizer_step_ema", "optimizer_step_two_groups")},
               ratio_by_bytes=round(44 / 28, 3), finite=bool(torch.isfinite(m.flat_params).all()))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
