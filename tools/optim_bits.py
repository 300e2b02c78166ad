"""One digest per output array of every optimizer entry point that csrc/optim_sweep.h and csrc/optim_items.h carry, on fixed seeded inputs:
the flat steps (sgd, adam, madgrad, adais), the layer-wise and unit-wise steps (lw_*, lw_unit_*), AdamP, SAMOriginal (sam_*) and SAM (sam_lw_*,
sam_unit_sumsq).  Run it once per build of the library, one process each (MI355RN_LIB selects the build), and compare the printed lines: a
refactor of the device code must leave every line as it was.

    python tools/optim_bits.py > new.txt;  MI355RN_LIB=/path/to/other/libmi355rn.so python tools/optim_bits.py > other.txt;  diff other.txt new.txt

The table cases lay tensors out in one flat array with sentinel-filled gaps between them (the tool itself checks that the gaps keep their bits):
whole-tensor slots of 1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096 and 9000 elements (three work items), and unit-wise tensors whose units are 1, 2, 3,
4, 5, 9, 27, 37, 113, 147, 255, 256, 257, 4095, 4096 and 4100 elements long — the odd ones begin at every off & 3, (2, 4100) is cut into two
pieces per unit and its second work item starts mid-unit, the second item of (40, 113) starts inside unit 36 and runs over three more,
(37, 113), (10, 37) and (8, 3, 7, 7) have items that span many units — in two param groups with their own hyper-parameters."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sota_imagenet_amd import ops  # noqa: E402
from sota_imagenet_amd.callbacks import SAM, SAMOriginal  # noqa: E402
from sota_imagenet_amd.item_plan import TENSOR_FIELDS, pack_records  # noqa: E402
from sota_imagenet_amd.optim import AdamP, _Layerwise  # noqa: E402

DEV = "cuda:0"
SENTINEL = -1234.5
SHAPES = [  # (shape, param group)
    ((1,), 0), ((2,), 0), ((3,), 0), ((4,), 0), ((5,), 0), ((255,), 0), ((256,), 0), ((257,), 0), ((4095,), 0), ((4096,), 0), ((5, 1), 0),
    ((3, 2), 0), ((7, 3), 0), ((3, 4), 0), ((3, 5), 0), ((2, 255), 0), ((2, 256), 0), ((2, 257), 0), ((2, 4095), 0), ((2, 4096), 0),
    ((6, 9), 1), ((4, 27), 1), ((10, 37), 1), ((8, 3, 7, 7), 1), ((37, 113), 1), ((40, 113), 1), ((1, 4100), 1), ((2, 4100), 1), ((9000,), 1), ((3, 4096), 1),
]


def emit(case, **arrays):
    for name, t in arrays.items():
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:20]
        print(f"{case}/{name} {h}", flush=True)


def rand(gen, n, lo=-1.0, hi=1.0):
    return (torch.rand(n, generator=gen, dtype=torch.float32) * (hi - lo) + lo).to(DEV)


def layout():
    """[(param base, grad base, first element, numel, group, unit_len, kind)], the array length and the mask of the gaps"""
    tensors, cur = [], 4
    for shape, gi in SHAPES:
        n = int(np.prod(shape))
        tensors.append((0, 0, cur, n, gi, n // shape[0] if len(shape) > 1 else n, int(len(shape) > 1)))
        cur = (cur + n + 3) // 4 * 4 + 4
    gap = torch.ones(cur, dtype=torch.bool)
    for _, _, off, n, *_ in tensors:
        gap[off:off + n] = False
    return tensors, cur, gap.to(DEV)


class Arrays:
    """seeded flat arrays with the sentinel in every gap; view(name) is the range [lo, hi) the item offsets count from"""

    def __init__(self, seed, total, gap, lo, hi, **ranges):
        gen = torch.Generator().manual_seed(seed)
        self.gap, self.lo, self.hi, self.full = gap, lo, hi, {}
        for name, (a, b) in ranges.items():
            self.full[name] = torch.where(gap, torch.full((total,), SENTINEL, device=DEV), rand(gen, total, a, b))

    def view(self, name):
        return self.full[name][self.lo:self.hi]

    def emit(self, case, *names):
        for name in names:
            assert bool((self.full[name][self.gap] == SENTINEL).all()), f"{case}/{name}: a gap between tensors was written"
        emit(case, **{n: self.full[n] for n in names})


def flat_cases():
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 70001):
        for ema_on in (False, True):
            gen = torch.Generator().manual_seed(n)
            case = f"n{n}_ema{int(ema_on)}"
            ema = dict(ema=rand(gen, n), ema_decay=0.99) if ema_on else {}
            out = lambda **a: dict(a, **({"ema": ema["ema"]} if ema_on else {}))  # noqa: E731
            p, g, m = rand(gen, n), rand(gen, n), rand(gen, n)
            ops.sgd_step(p, g, m, 0.1, momentum=0.9, weight_decay=5e-5, grad_scale=0.5, **ema)
            emit(f"sgd/{case}", **out(p=p, m=m))
            for decoupled in (True, False):
                p, g, m, v = rand(gen, n), rand(gen, n), rand(gen, n), rand(gen, n, 0.0, 1.0)
                ops.adam_step(p, g, m, v, 3, 1e-3, weight_decay=0.01, decoupled=decoupled, grad_scale=0.5, **ema)
                emit(f"adam_dec{int(decoupled)}/{case}", **out(p=p, m=m, v=v))
            p, g, q, s, x0 = rand(gen, n), rand(gen, n), rand(gen, n, 0.0, 1.0), rand(gen, n), rand(gen, n)
            ops.madgrad_step(p, g, q, s, x0, 5, 1e-2, momentum=0.9, weight_decay=1e-4, grad_scale=0.5, **ema)
            emit(f"madgrad/{case}", **out(p=p, gss=q, s=s))
            p, g, m, v, bp = rand(gen, n), rand(gen, n), rand(gen, n), rand(gen, n, 0.0, 1.0), rand(gen, n, 0.1, 0.9)
            ws = torch.zeros(ops.adais_workspace_elems(n), dtype=torch.float64, device=DEV)
            mean = torch.zeros(1, dtype=torch.float32, device=DEV)
            ops.adais_moments(g, v, 4, 0.99, ws, grad_scale=0.5)
            ops.adais_mean(ws, n, mean)
            ops.adais_step(p, g, m, v, bp, mean, 4, 0.1, weight_decay=5e-4, grad_scale=0.5, **ema)
            emit(f"adais/{case}", **out(p=p, m=m, v=v, b1prod=bp, partial=ws, mean=mean))


GROUPS = [dict(lr=0.01, wd=1e-3, b1=0.9, b2=0.98, eps=1e-8), dict(lr=0.003, wd=0.0, b1=0.95, b2=0.25, eps=1e-3)]


def layerwise_cases(tensors, total, gap):
    tab = _Layerwise.plan_tables([t[:5] for t in tensors], ops.lw_item_elems())
    (lo, hi, i0, i1, by_group, _), = tab["pairs"]
    items, trec, nt = pack_records(tab["items"], DEV), pack_records(tab["tensors"], DEV, TENSOR_FIELDS), len(tensors)
    flag_sets = {0: (0, ops.LW_MEAN | ops.LW_STABLE_WD, ops.LW_SOFT_WD), 1: (0, ops.LW_STABLE_WD), 2: (0, ops.LW_SGD_MOM | ops.LW_SQRT_MOM | ops.LW_STABLE_WD)}
    for rule, sets in flag_sets.items():
        for flags in sets:
            for ema_on in (False, True):
                case = f"lw/rule{rule}_flags{flags}_ema{int(ema_on)}"
                A = Arrays(100 + rule, total, gap, lo, hi, p=(-1, 1), g=(-1, 1), m=(-1, 1), ema=(-1, 1))
                partial = torch.zeros(len(tab["items"]), dtype=torch.float64, device=DEV)
                v = torch.full((nt,), 0.5, dtype=torch.float64 if rule == 2 else torch.float32, device=DEV)
                coef, sums = torch.zeros(nt, 4, dtype=torch.float32, device=DEV), torch.zeros(nt, dtype=torch.float64, device=DEV)
                ops.lw_sumsq(A.view("p" if rule == 1 else "g"), items[i0:i1], partial[i0:i1], nt, scale=1.0 if rule == 1 else 0.5)
                for gi, t0, t1 in tab["groups"]:
                    G = GROUPS[gi]
                    ops.lw_coef(rule, flags, partial, trec[t0:t1], v[t0:t1], coef[t0:t1], sums[t0:t1], 0.1 if rule == 2 else G["b1"], G["b2"], G["eps"],
                                G["lr"], G["wd"], mean=0.3)
                for gi, a, b in by_group:
                    ops.lw_update(rule, A.view("p"), A.view("g"), A.view("m"), items[a:b], coef, GROUPS[gi]["lr"],
                                  wd_eps=1e-2 if flags & ops.LW_SOFT_WD else None, grad_scale=0.5, ema=A.view("ema") if ema_on else None,
                                  ema_decay=0.99 if ema_on else 0.0)
                emit(case, partial=partial, sums=sums, v=v, coef=coef)
                A.emit(case, "p", "m", "ema")


def unit_tables(tensors):
    tab = _Layerwise.plan_unit_tables([t[:6] for t in tensors], ops.lw_item_elems())
    dev = dict(items=pack_records(tab["items"], DEV), tensors=pack_records(tab["tensors"], DEV), pieces=pack_records(tab["pieces"], DEV),
               whole=pack_records(tab["whole"], DEV), slots=torch.tensor(tab["slots"], dtype=torch.int32, device=DEV))
    return tab, dev


def unitwise_cases(tensors, total, gap):
    tab, d = unit_tables(tensors)
    (lo, hi, i0, i1, (pa, pb), (wa, wb), k0, _, by_group), = tab["pairs"]
    ns, nt = len(tab["slots"]), len(tensors)
    for rule, wd_eps in ((0, None), (0, 1e-2), (1, None)):
        for ema_on in (False, True):
            case = f"lw_unit/rule{rule}_wdeps{int(wd_eps is not None)}_ema{int(ema_on)}"
            A = Arrays(200 + rule, total, gap, lo, hi, p=(-1, 1), g=(-1, 1), m=(-1, 1), ema=(-1, 1))
            partial = torch.zeros(pb - pa + wb - wa, dtype=torch.float64, device=DEV)
            v, den = torch.full((ns,), 0.5, dtype=torch.float32, device=DEV), torch.zeros(ns, dtype=torch.float32, device=DEV)
            sums = torch.zeros(ns, dtype=torch.float64, device=DEV)
            src, scale, k1 = A.view("p" if rule == 1 else "g"), 1.0 if rule == 1 else 0.5, k0 + pb - pa
            ops.lw_unit_sumsq(src, d["pieces"][pa:pb], partial[k0:k1], ns, scale=scale)
            ops.lw_sumsq(src, d["whole"][wa:wb], partial[k1:k1 + wb - wa], nt, scale=scale)
            for gi, s0, s1 in tab["groups"]:
                ops.lw_unit_coef(partial, d["slots"][s0:s1], v[s0:s1], den[s0:s1], sums[s0:s1], GROUPS[gi]["b2"], GROUPS[gi]["eps"])
            for gi, a, b in by_group:
                G = GROUPS[gi]
                ops.lw_unit_update(rule, A.view("p"), A.view("g"), A.view("m"), d["items"][a:b], d["tensors"], den, G["b1"], G["lr"], G["wd"],
                                   wd_eps=wd_eps, grad_scale=0.5, ema=A.view("ema") if ema_on else None, ema_decay=0.99 if ema_on else 0.0)
            emit(case, partial=partial, sums=sums, v=v, den=den)
            A.emit(case, "p", "m", "ema")


def adamp_cases(tensors, total, gap):
    tab = AdamP.plan_tables(tensors, ops.lw_item_elems())
    (lo, hi, _, _, _, _, _, _, by_group, sum_launches), = tab["pairs"]
    items, trec, pieces = pack_records(tab["items"], DEV), pack_records(tab["tensors"], DEV), pack_records(tab["sum_pieces"], DEV)
    slots, decide = torch.tensor(tab["slots"], dtype=torch.int32, device=DEV), torch.tensor(tab["decide"], dtype=torch.int32, device=DEV)
    ns, nt = len(tab["slots"]), len(tensors)
    # delta 0.1 leaves random tensors alone (mode 0), 1.0 projects most of them by layer (mode 2), 10.0 all of them by unit (mode 1)
    for deltas in ((0.1, 10.0), (1.0, 1.0)):
        for nesterov in (False, True):
            for ema_on in (False, True):
                case = f"adamp/delta{deltas[0]}_{deltas[1]}_nesterov{int(nesterov)}_ema{int(ema_on)}"
                A = Arrays(300, total, gap, lo, hi, p=(-1, 1), g=(-1, 1), m=(-1, 1), v=(0, 1), ema=(-1, 1))
                partial = torch.zeros(len(tab["pieces"]) + len(tab["whole"]), 4, dtype=torch.float64, device=DEV)
                coef, wdf = torch.zeros(ns, 2, dtype=torch.float32, device=DEV), torch.ones(nt, dtype=torch.float32, device=DEV)
                mode = torch.zeros(nt, dtype=torch.int32, device=DEV)
                adam = lambda gi: dict(step=3, betas=(GROUPS[gi]["b1"], 0.999), eps=GROUPS[gi]["eps"], nesterov=nesterov, grad_scale=0.5)  # noqa: E731
                for gi, a, b, k in sum_launches:
                    ops.adamp_unit_sums(A.view("p"), A.view("g"), A.view("m"), A.view("v"), pieces[a:b], partial[k:k + b - a], ns, **adam(gi))
                for gi, t0, t1 in tab["groups"]:
                    G = GROUPS[gi]
                    ops.adamp_coef(partial, slots, decide[t0:t1], coef, wdf[t0:t1], mode[t0:t1], G["lr"], 1e-2 * (1 - gi), G["eps"], deltas[gi], 0.1)
                for gi, a, b in by_group:
                    ops.adamp_update(A.view("p"), A.view("g"), A.view("m"), A.view("v"), items[a:b], trec, coef, wdf, lr=GROUPS[gi]["lr"],
                                     ema=A.view("ema") if ema_on else None, ema_decay=0.99 if ema_on else 0.0, **adam(gi))
                emit(case, partial=partial, coef=coef, wdf=wdf, mode=mode)
                print(f"{case}/modes_0_1_2 {[int((mode == k).sum()) for k in range(3)]}")
                A.emit(case, "p", "m", "v", "ema")


def sam_cases(tensors, total, gap):
    items_l, kind_l, pairs = SAMOriginal.plan_tables([t[:4] + (1 + t[6],) for t in tensors], ops.lw_item_elems())
    (lo, hi, i0, i1, _), = pairs
    items, kind = pack_records(items_l, DEV), torch.tensor(kind_l, dtype=torch.int32, device=DEV)
    A = Arrays(400, total, gap, lo, hi, p=(-1, 1), g=(-1, 1), eps=(-1, 1))
    partial, out = torch.zeros(len(items_l), dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.float32, device=DEV)
    ops.sam_sumsq(A.view("p"), A.view("g"), items[i0:i1], kind, partial[i0:i1], 0.01, grad_scale=0.5)
    ops.sam_scale(partial, 0.05, out)
    ops.sam_perturb(A.view("p"), A.view("g"), A.view("eps"), items[i0:i1], kind, out, 0.01, grad_scale=0.5)
    emit("sam/perturb", partial=partial, out=out)
    A.emit("sam/perturb", "p", "eps")
    ops.sam_restore(A.view("p"), A.view("eps"), items[i0:i1], len(tensors))
    A.emit("sam/restore", "p")

    tab = SAM.plan_tables([t[:4] + (t[5],) for t in tensors], ops.lw_item_elems())
    (lo, hi, i0, i1, (pa, pb), (wa, wb), k0, _), = tab["pairs"]
    d = {k: pack_records(tab[k], DEV) for k in ("items", "tensors", "pieces", "whole")}
    slots, ns, nt, k1 = torch.tensor(tab["slots"], dtype=torch.int32, device=DEV), len(tab["slots"]), len(tensors), k0 + pb - pa
    for tpp in (64, 256):
        A = Arrays(500, total, gap, lo, hi, p=(-1, 1), g=(-1, 1), eps=(-1, 1))
        partial = torch.zeros(2 * (pb - pa + wb - wa), dtype=torch.float64, device=DEV)
        coef, norms = torch.zeros(ns, dtype=torch.float32, device=DEV), torch.zeros(2 * ns, dtype=torch.float32, device=DEV)
        ops.sam_unit_sumsq(A.view("p"), A.view("g"), d["pieces"][pa:pb], partial[2 * k0:2 * k1], ns, grad_scale=0.5, threads_per_piece=tpp)
        ops.sam_lw_sumsq(A.view("p"), A.view("g"), d["whole"][wa:wb], partial[2 * k1:2 * (k1 + wb - wa)], nt, grad_scale=0.5)
        ops.sam_lw_coef(partial, slots, coef, norms)
        ops.sam_lw_perturb(A.view("p"), A.view("g"), A.view("eps"), d["items"][i0:i1], d["tensors"], coef, 0.05, grad_scale=0.5)
        emit(f"sam_lw/tpp{tpp}", partial=partial, coef=coef, norms=norms)
        A.emit(f"sam_lw/tpp{tpp}", "p", "eps")


def main():
    assert torch.cuda.is_available(), "optim_bits.py needs the GPU"
    torch.cuda.set_device(0)
    tensors, total, gap = layout()
    flat_cases()
    layerwise_cases(tensors, total, gap)
    unitwise_cases(tensors, total, gap)
    adamp_cases(tensors, total, gap)
    sam_cases(tensors, total, gap)
    torch.cuda.synchronize()
    print("lines above: one digest per output array;", os.environ.get("MI355RN_LIB", "the default library"), file=sys.stderr)


if __name__ == "__main__":
    main()
