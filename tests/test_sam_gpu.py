"""Native SAMOriginal (csrc/optim_sam.hip, callbacks.SAMOriginal) on the MI355X: the four kernels against torch on the same arrays (the norm to
the summation bound, the elementwise stages bit for bit), the callback over the native optimizers against the trajectories recorded from the
reference's own callback (tests/golden/sam_ref_trajectories.npz, the yardstick rule of tests/optim_harness.py), and the callback inside Runner on
the real models: what the second forward sees, what the optimizer steps on, what it leaves behind."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_harness as H
from optim_harness import NAN, U
from plan_common import layout as _layout
from plan_common import table
from sam_common import CASES, NORM_FLOOR, Fixture, generator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 123.0
RHO, ETA = 0.5, 0.01


# ---- the kernels, driven directly --------------------------------------------------------------------------------------------------------
class _Arrays:
    """tensors laid out in `nbuf` pairs of flat parameter / gradient buffers (tensor i in pair i % nbuf): the sentinel in every gap of p, NaN in
    every gap of g, and the tables of SAMOriginal.plan_tables"""

    def __init__(self, sizes, kinds, vals, grads, dev, nbuf=1):
        from sota_imagenet_amd import ops
        from sota_imagenet_amd.callbacks import SAMOriginal

        self.sizes, self.kinds, self.nbuf = sizes, kinds, nbuf
        members = [[i for i in range(len(sizes)) if i % nbuf == b] for b in range(nbuf)]
        self.where = {}
        self.fp, self.fg, self.mask = [], [], []
        for b, idx in enumerate(members):
            offs, n = _layout([sizes[i] for i in idx])
            fp, fg = torch.full((n,), SENTINEL, device=dev), torch.full((n,), NAN, device=dev)
            mask = torch.zeros(n, dtype=torch.bool, device=dev)
            for i, o in zip(idx, offs):
                fp[o:o + sizes[i]] = vals[i].to(dev)
                fg[o:o + sizes[i]] = grads[i].to(dev)
                mask[o:o + sizes[i]] = True
                self.where[i] = (b, o)
            self.fp.append(fp), self.fg.append(fg), self.mask.append(mask)
        order = [i for idx in members for i in idx]
        tensors = [(self.fp[self.where[i][0]].data_ptr(), self.fg[self.where[i][0]].data_ptr(), self.where[i][1], sizes[i], 1 + kinds[i]) for i in order]
        items, kind, self.pairs = SAMOriginal.plan_tables(tensors, ops.lw_item_elems())
        assert kind == [kinds[i] for i in order] and len(self.pairs) == nbuf
        self.order = order
        self.items = table(items, dev)
        self.kind = torch.tensor(kind, dtype=torch.int32, device=dev)
        self.partial = torch.full((len(items),), NAN, dtype=torch.float64, device=dev)
        self.out = torch.full((2,), NAN, device=dev)
        self.eps = [torch.full_like(fp, SENTINEL) for fp in self.fp]

    def sumsq_and_scale(self, gs, rho=RHO, eta=ETA):
        from sota_imagenet_amd import ops

        for b, (lo, hi, i0, i1, _) in enumerate(self.pairs):
            ops.sam_sumsq(self.fp[b][lo:hi], self.fg[b][lo:hi], self.items[i0:i1], self.kind, self.partial[i0:i1], eta, grad_scale=gs)
        ops.sam_scale(self.partial, rho, self.out)

    def perturb(self, gs, eta=ETA):
        from sota_imagenet_amd import ops

        for b, (lo, hi, i0, i1, _) in enumerate(self.pairs):
            ops.sam_perturb(self.fp[b][lo:hi], self.fg[b][lo:hi], self.eps[b][lo:hi], self.items[i0:i1], self.kind, self.out, eta, grad_scale=gs)

    def restore(self):
        from sota_imagenet_amd import ops

        for b, (lo, hi, i0, i1, _) in enumerate(self.pairs):
            ops.sam_restore(self.fp[b][lo:hi], self.eps[b][lo:hi], self.items[i0:i1], self.kind.numel())

    def tensor(self, bufs, i):
        b, o = self.where[i]
        return bufs[b][o:o + self.sizes[i]]


def _problem(dev, nbuf=1, zero_grad=False, seed=5):
    """the fixture's six tensors plus 1, 3, 64, 4096, 4097 and 2 * 4096 + 5 elements, weights and others mixed; |p| on both sides of eta and of
    sqrt(eta), gradients of very different magnitude per tensor"""
    fx = Fixture("sgd")
    sizes = fx.sizes + [1, 3, 64, 4096, 4097, 2 * 4096 + 5]
    kinds = [int(len(s) > 1) for s in fx.shapes] + [1, 0, 0, 1, 0, 1]
    gen = torch.Generator().manual_seed(seed)
    vals = [(torch.rand(s, generator=gen) - 0.5) * (1.0 if i % 3 else 0.05) for i, s in enumerate(sizes)]
    grads = [torch.zeros(s) if zero_grad else torch.randn(s, generator=gen) * (10.0 ** (i % 4 - 2)) for i, s in enumerate(sizes)]
    assert any((v.abs() < ETA).any() and (v.abs() > ETA).any() for v in vals) and any((v * v > ETA).any() for v in vals)
    return _Arrays(sizes, kinds, vals, grads, dev, nbuf)


def _w_products(A, gs, eta=ETA):
    """the float32 products w of the norm, computed by torch on the device from the same arrays, per tensor"""
    out = []
    for i in range(len(A.sizes)):
        p, ge = A.tensor(A.fp, i), A.tensor(A.fg, i) * gs
        out.append(ge * p.abs().clamp_min(eta) if A.kinds[i] else ge)
    return out


@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("nbuf", [1, 2])
def test_norm_equals_the_float64_sum_of_the_float32_products(dev, gs, nbuf):
    """out[1] against sqrt of the float64 sum of the squares of the float32 products w: relative error <= n * 2^-53 (the worst-case summation
    bound in double) + 2^-24 (the one rounding to float); out[0] within one float32 ulp of rho / max(norm64, 2e-5).  NaN in every gap of the
    gradient buffer and a sentinel in every gap of the parameter buffer: a gap read into the sum would show"""
    A = _problem(dev, nbuf)
    A.sumsq_and_scale(gs)
    torch.cuda.synchronize()
    n = sum(A.sizes)
    S = sum(float(w.double().pow(2).sum()) for w in _w_products(A, gs))
    norm64 = math.sqrt(S)
    got_scale, got_norm = (float(x) for x in A.out.cpu())
    rel = abs(got_norm - norm64) / norm64
    bound = n * 2.0 ** -53 + 2.0 ** -24
    print(f"gs={gs} pairs={nbuf}: n={n} items={A.items.shape[0]} norm {got_norm!r} vs float64 {norm64!r}: relative error {rel:.3e} (bound {bound:.3e})")
    assert norm64 > NORM_FLOOR and rel <= bound
    want = RHO / max(norm64, NORM_FLOOR)
    assert abs(got_scale - want) <= float(np.spacing(np.float32(want))), (got_scale, want)
    assert torch.isfinite(A.partial).all() and A.partial.numel() == A.items.shape[0] >= len(A.sizes) + 3
    # per item: the partial sums are those of the items' own elements
    per_tensor = torch.zeros(len(A.sizes), dtype=torch.float64)
    rec = A.items.cpu().numpy().reshape(-1).view([("off", "<i8"), ("len", "<i4"), ("t", "<i4")])
    per_tensor.index_add_(0, torch.from_numpy(rec["t"].astype(np.int64)), A.partial.cpu())
    want_t = torch.stack([w.double().pow(2).sum().cpu() for w in _w_products(A, gs)])[A.order]
    assert ((per_tensor - want_t).abs() <= 1e-12 * want_t).all()


def test_zero_gradient_sits_on_the_floor_of_the_norm(dev):
    A = _problem(dev, zero_grad=True)
    A.sumsq_and_scale(1.0)
    before = [fp.clone() for fp in A.fp]
    A.perturb(1.0)
    torch.cuda.synchronize()
    assert float(A.out[1]) == float(np.float32(NORM_FLOOR)) and math.isfinite(float(A.out[0])) and float(A.out[0]) == float(np.float32(RHO / NORM_FLOOR))
    assert all((e[m] == 0).all() and (e[~m] == SENTINEL).all() for e, m in zip(A.eps, A.mask))
    assert all(torch.equal(a, b) for a, b in zip(A.fp, before))


@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("nbuf", [1, 2])
def test_perturbation_and_restore_are_bitwise_torchs(dev, gs, nbuf):
    """with s = out[0]: eps == ((p*p).clamp_min(eta) * (g*gs)) * s for weights and (g*gs) * s for the others, in torch float32 on the device;
    p_after == p + eps and p_restored == p_after - eps, bit for bit; the gaps keep their sentinel in p and in eps"""
    A = _problem(dev, nbuf)
    A.sumsq_and_scale(gs)
    p0 = [fp.clone() for fp in A.fp]
    s = A.out[0].clone()
    A.perturb(gs)
    p1 = [fp.clone() for fp in A.fp]
    A.restore()
    torch.cuda.synchronize()
    moved = 0
    for i in range(len(A.sizes)):
        p, g = A.tensor(p0, i), A.tensor(A.fg, i)
        want = ((p * p).clamp_min(ETA) * (g * gs)) * s if A.kinds[i] else (g * gs) * s
        eps = A.tensor(A.eps, i)
        assert torch.equal(eps, want), f"eps of tensor {i} ({A.sizes[i]} elements, kind {A.kinds[i]})"
        assert torch.equal(A.tensor(p1, i), p + eps) and torch.equal(A.tensor(A.fp, i), (p + eps) - eps)
        moved += int((A.tensor(p1, i) != p).any())
    assert moved == len(A.sizes)
    assert any(not torch.equal(a, b) for a, b in zip(A.fp, p0))  # (p + eps) - eps is not p everywhere
    for b in range(nbuf):
        gap = ~A.mask[b]
        assert gap.any() and (p1[b][gap] == SENTINEL).all() and (A.fp[b][gap] == SENTINEL).all() and (A.eps[b][gap] == SENTINEL).all()
        assert torch.isnan(A.fg[b][gap]).all() and torch.isfinite(A.fp[b]).all()


def test_replay_is_bitwise(dev):
    res = []
    for _ in range(2):
        A = _problem(dev, 2)
        A.sumsq_and_scale(0.25)
        A.perturb(0.25)
        torch.cuda.synchronize()
        res.append((A.partial.clone(), A.out.clone(), [e.clone() for e in A.eps]))
    (pa, oa, ea), (pb, ob, eb) = res
    assert torch.equal(pa, pb) and torch.equal(oa, ob) and all(torch.equal(x, y) for x, y in zip(ea, eb))
    one = _problem(dev, 1)  # the same tensors in ONE storage pair: the table order differs, the norm is summed in another order
    one.sumsq_and_scale(0.25)
    torch.cuda.synchronize()
    assert abs(float(one.out[1]) - float(oa[1])) <= float(np.spacing(np.float32(float(oa[1]))))


# ---- the callback over the native optimizers, on the fixture's problem --------------------------------------------------------------------
class _Record:
    """callbacks around SAMOriginal in a Runner: lr per step before it, what it left behind after it"""

    def __init__(self, fw, sam, lrs, ps, fp):
        rec = self

        class Before(fw.Callback):
            def on_batch_begin(self):
                for g in self.state.optimizer.param_groups:
                    g["lr"] = lrs[self.state.step]

            def on_after_backward(self):
                rec.fp_before = fp.clone()

        class After(fw.Callback):
            def on_after_backward(self):
                rec.fp_pairs.append((rec.fp_before, fp.clone()))
                e = sam.eps_flat
                rec.eps.append(None if e is None else ([t.clone() for t in e] if isinstance(e, list) else e.clone()))
                rec.norm.append(None if sam.norm is None else sam.norm.clone())

            def on_batch_end(self):
                rec.step.append(torch.cat([p.detach().reshape(-1) for p in ps]).clone())

        self.eps, self.norm, self.step, self.fp_pairs = [], [], [], []
        self.before, self.after = Before(), After()


def _run_fixture(fx, dev, separate=False):
    """the fixture's four steps through fit_wrapper.Runner with the native optimizer and the native callback; parameters laid out group by group
    in one flat buffer pair (NaN in the gradient's gaps, the sentinel in the parameter's), or each tensor in a storage of its own"""
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAMOriginal

    gen = generator()
    order = [i for idx in fx.groups for i in idx]
    offs, n = _layout(fx.sizes, order)
    fp, fg = torch.full((n,), SENTINEL, device=dev), torch.full((n,), NAN, device=dev)
    ps = []
    for i, (o, s, shape) in enumerate(zip(offs, fx.sizes, fx.shapes)):
        v = fx.split(fx.p0)[i].to(dev)
        if separate:
            p = torch.nn.Parameter(v.clone().view(shape))
            p.grad = torch.zeros(s, device=dev).view(shape)
        else:
            fp[o:o + s] = v
            fg[o:o + s] = 0
            p = torch.nn.Parameter(fp[o:o + s].view(shape))
            p.grad = fg[o:o + s].view(shape)
        ps.append(p)
    groups = [{"params": [ps[i] for i in fx.groups[0]]}, {"params": [ps[i] for i in fx.groups[1]], "weight_decay": 0}]
    opt = getattr(optim, fx.cls)(groups, lr=fx.lrs[0], **fx.kw)
    model = gen.Quadratic(ps, fx.a)
    sam = SAMOriginal(rho=fx.rho, eta=fx.eta)
    rec = _Record(fw, sam, fx.lrs, ps, fp)

    class Loader:
        batch_size = 1

        def __len__(self):
            return fx.steps

        def __iter__(self):
            return iter([([c.to(dev) for c in fx.targets(k)], None) for k in range(fx.steps)])

    forwards = []

    class Count(fw.Callback):
        def on_batch_end(self):
            forwards.append(len(model.seen))

    runner = fw.Runner(model, opt, gen.criterion, callbacks=[rec.before, sam, rec.after, Count()])
    runner.fit(Loader(), epochs=1)
    torch.cuda.synchronize()
    return dict(rec=rec, sam=sam, opt=opt, ps=ps, fp=fp, fg=fg, offs=offs, seen=model.seen, forwards=forwards, order=order)


@pytest.mark.parametrize("case", CASES)
def test_callback_follows_the_reference_trajectory(dev, case):
    """the three recorded cases (the reference callback over torch SGD, over its own AdamLayerwise with recipe 49's values, and on the floor of the
    norm) with the native callback over the native optimizers: eps, the parameters the second forward saw and the parameters after every step
    within 1.5 x the reference's own float32 error + 4 * 2^-24 * max|ref| of the reference's float64 run.  Step 1 is a plain step: one forward,
    no eps.  The callback never touches the gaps of the flat buffers (a sentinel in p, NaN in g)."""
    fx = Fixture(case)
    r = _run_fixture(fx, dev)
    rec, sam = r["rec"], r["sam"]
    assert [b - a for a, b in zip([0] + r["forwards"], r["forwards"])] == fx.forwards == [1, 2, 2, 2]
    assert rec.eps[0] is None and rec.norm[0] is None and sam.forwards == 3  # step 1 allocates nothing
    worst = 0.0
    second = [2, 4, 6]  # model.seen: index of the second forward of steps 2, 3, 4
    for k in range(fx.steps):
        worst = max(worst, fx.check(k, rec.step[k], "step"))
        if k == 0:
            continue
        eps = torch.cat([rec.eps[k][r["offs"][i]:r["offs"][i] + fx.sizes[i]] for i in range(len(fx.sizes))])
        worst = max(worst, fx.check(k, eps, "eps"), fx.check(k, r["seen"][second[k - 1]], "pert"))
        norm = float(rec.norm[k])
        print(f"{case} step {k + 1}: norm {norm!r} (reference float64 {fx.norm[k]!r})")
        assert abs(norm - fx.norm[k]) <= 4 * U * fx.norm[k]
        assert (norm == float(np.float32(NORM_FLOOR))) == (case == "clamp")
    print(f"{case}: worst native error / max(reference-fp32 error, floor) {worst:.2f}")
    fp, fg = r["fp"], r["fg"]
    gap = torch.ones_like(fp, dtype=torch.bool)
    for o, s in zip(r["offs"], fx.sizes):
        gap[o:o + s] = False
    assert gap.any() and torch.isnan(fg[gap]).all() and torch.isfinite(fp[~gap]).all()
    for k, (before, after) in enumerate(rec.fp_pairs):  # across the callback the gaps keep their bits; the tensors come back to within rounding
        assert torch.equal(before.view(torch.int32)[gap], after.view(torch.int32)[gap])
        assert torch.equal(before, after) == (k == 0)
    if fx.cls != "SGD":  # (the native SGD merges neighbouring ranges and sweeps the 64-element gaps between them; the layer-wise step does not)
        assert (fp[gap] == SENTINEL).all()
    assert (sam.eps_flat[gap[:sam.eps_flat.numel()]] == 0).all()
    assert sam._kind.cpu().tolist() == [int(len(fx.shapes[i]) > 1) for i in r["order"]]


@pytest.mark.parametrize("case", ["sgd", "adamlw_recipe"])
def test_placement_is_bitwise(dev, case):
    """every tensor in a parameter / gradient storage of its own (six launch sets, one norm over all of them) gives the parameters of the
    flat-buffer run bit for bit after every step, and the same eps"""
    fx = Fixture(case)
    a, b = _run_fixture(fx, dev), _run_fixture(fx, dev, separate=True)
    assert len(a["sam"]._segs) == 1 and len(b["sam"]._segs) == 6
    for k in range(fx.steps):
        assert torch.equal(a["rec"].step[k], b["rec"].step[k])
    for k in range(1, fx.steps):
        flat = torch.cat([a["rec"].eps[k][a["offs"][i]:a["offs"][i] + fx.sizes[i]] for i in a["order"]])
        assert torch.equal(flat, torch.cat(b["rec"].eps[k])) and torch.equal(a["rec"].norm[k], b["rec"].norm[k])


def test_parameters_that_do_not_fit_raise(dev):
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd.callbacks import SAMOriginal

    def state_of(p):
        opt = torch.optim.SGD([p], lr=0.1)
        opt.state[p]["x"] = 1  # (a state: the callback does not skip)
        sam = SAMOriginal()
        sam.set_state(fw.RunnerState(model=None, optimizer=opt, criterion=None))
        return sam

    p = torch.nn.Parameter(torch.zeros(8))  # on the CPU
    p.grad = torch.zeros(8)
    with pytest.raises(RuntimeError, match="CUDA fp32"):
        state_of(p).on_after_backward()
    buf = torch.zeros(64, device=dev)
    p = torch.nn.Parameter(buf[2:10])  # 8 bytes into its storage
    p.grad = torch.zeros(64, device=dev)[2:10]
    with pytest.raises(RuntimeError, match="16-byte"):
        state_of(p).on_after_backward()
    p = torch.nn.Parameter(buf[4:12])
    p.grad = torch.zeros(64, device=dev)[8:16]
    with pytest.raises(RuntimeError, match="share their flat offset"):
        state_of(p).on_after_backward()


# ---- the callback inside Runner on the real models ------------------------------------------------------------------------------------------
def _model(kind):
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.models import resnet50

    if kind == "bresnet50-bf16":
        return BResNet50(dtype="bf16").cuda()
    return resnet50(dtype=kind.split("-")[1]).cuda()


@pytest.mark.parametrize("kind", ["resnet50-fp32", "resnet50-bf16", "bresnet50-bf16"])
def test_three_runner_steps_on_the_real_model(dev, kind):
    """N = 4 at 64 px, AdamLayerwise with recipe 49's values, a spy before and one after SAMOriginal: num_batches_tracked reads 1, 3, 5; the
    parameters the second forward saw are p0 + eps_flat and the callback leaves that minus eps_flat, bit for bit; the padding of the flat array
    never changes; the gradient the optimizer steps on is the second one — overwritten, not accumulated (fp32: against a manual forward /
    backward at the perturbed parameters on a second model; the two thresholds tell "overwritten" from "accumulated", they are no accuracy
    claims); loss and parameters stay finite"""
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAMOriginal
    from sota_imagenet_amd.losses import CrossEntropyLoss

    m = _model(kind)
    crit = CrossEntropyLoss(smoothing=0.1)
    opt = optim.AdamLayerwise([{"params": list(m.parameters())}], lr=1e-3, betas=(0.9, 0.995), weight_decay=2e-2)
    sam = SAMOriginal()
    pad = H.padding_mask(m)
    pad0 = m.flat_params[pad].clone()
    nbt = next(b for n, b in m.named_buffers() if n.endswith("num_batches_tracked"))
    log = dict(seen=[], p0=[], g1=[], after=[], g_cb=[], eps=[], norm=[], nbt=[], finite=[])
    m.register_forward_pre_hook(lambda mod, inp: log["seen"].append(mod.flat_params.clone()))

    class Before(fw.Callback):
        def on_after_backward(self):
            log["p0"].append(m.flat_params.clone())
            log["g1"].append(m.flat_grads.clone())

    class After(fw.Callback):
        def on_after_backward(self):
            log["after"].append(m.flat_params.clone())
            log["g_cb"].append(m.flat_grads.clone())
            log["eps"].append(None if sam.eps_flat is None else sam.eps_flat.clone())
            log["norm"].append(None if sam.norm is None else sam.norm.clone())

        def on_batch_end(self):
            log["nbt"].append(int(nbt))
            log["finite"].append(bool(torch.isfinite(m.flat_params).all()) and bool(torch.isfinite(self.state.loss_meter.val)))

    loader = H.Loader()
    runner = fw.Runner(m, opt, crit, callbacks=[Before(), sam, After()])
    runner.fit(loader, epochs=1)
    torch.cuda.synchronize()
    assert log["nbt"] == [1, 3, 5] and all(log["finite"]) and math.isfinite(runner.state.loss_meter.avg)
    assert len(log["seen"]) == 5 and sam.forwards == 2 and log["eps"][0] is None
    assert torch.equal(log["after"][0], log["p0"][0]) and torch.equal(log["g_cb"][0], log["g1"][0])  # step 1: a plain step
    assert int(sam._kind.sum()) == sum(p.ndim > 1 for p in m.parameters()) and sam._kind.numel() == len(list(m.parameters()))
    assert len(sam._segs) == 1 and sam.eps_flat.numel() <= m.flat_params.numel()
    ref = None
    if kind == "resnet50-fp32":
        ref = _model(kind)
        ref.train()
    for k, second in ((1, 2), (2, 4)):  # steps 2 and 3: log["seen"][second] is what their second forward saw
        p0, eps = log["p0"][k], torch.zeros_like(log["p0"][k])
        eps[:log["eps"][k].numel()] = log["eps"][k]
        assert torch.equal(log["seen"][second - 1], p0)
        assert (eps[pad] == 0).all() and (eps[~pad] != 0).float().mean().item() > 0.5
        assert torch.equal(log["seen"][second], p0 + eps)
        assert torch.equal(log["after"][k], (p0 + eps) - eps)
        g1, g_cb = log["g1"][k][~pad], log["g_cb"][k][~pad]
        assert torch.isfinite(g_cb).all() and not torch.equal(g_cb, g1)
        if ref is not None:
            with torch.no_grad():
                ref.flat_params.copy_(log["seen"][second])
            ref.mark_grads_clean()
            data, target = loader.batches[k]
            crit(ref(data), target).backward()
            g_manual = ref.flat_grads[~pad]
            d_over = ((g_cb - g_manual).norm() / g_manual.norm()).item()
            d_acc = ((g_cb - (g1 + g_manual)).norm() / g1.norm()).item()
            print(f"{kind} step {k + 1}: |g_cb - g_manual| / |g_manual| = {d_over:.3e},  |g_cb - (g1 + g_manual)| / |g1| = {d_acc:.3e}")
            assert d_over <= 0.01 and d_acc > 0.5
        print(f"{kind} step {k + 1}: norm {float(log['norm'][k]):.6g}  max |eps| {eps.abs().max().item():.3e}")
    assert torch.equal(m.flat_params[pad], pad0)
    assert not torch.equal(m.flat_params, log["p0"][0])


def test_model_ema_inside_the_step_kernel_matches_the_callback(dev):
    """ModelEma under AdamLayerwise + SAMOriginal: the average advanced by the optimizer's update kernel (attach_ema) equals the callback's own lerp
    after every batch, the parameters are the same bits either way, and the perturbed parameters never enter the average"""
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAMOriginal

    def make():
        m = _model("resnet50-fp32")
        return m, optim.AdamLayerwise([{"params": list(m.parameters())}], lr=1e-4, betas=(0.9, 0.995), weight_decay=2e-2)

    def two_forwards(sam):
        assert sam.forwards == 2

    H.ema_matches_callback(make, 1e-4, callbacks=(SAMOriginal,), val_loader=H.Loader(2, seed=8), after_fit=two_forwards)


# ---- smoke: train.py and the data-parallel wrapper --------------------------------------------------------------------------------------------
def test_train_py_runs_the_smoke_config(dev, tmp_path, monkeypatch):
    """train.py on nov-adam_sam_test: the native callback is built from the reference's target, perturbs in every step but the first, and the losses
    are finite"""
    from sota_imagenet_amd import callbacks

    made = []
    init = callbacks.SAMOriginal.__init__
    monkeypatch.setattr(callbacks.SAMOriginal, "__init__", lambda self, *a, **k: (made.append(self), init(self, *a, **k))[1])
    calls = H.count_launches(monkeypatch, ["sam_sumsq", "sam_scale", "sam_perturb", "sam_restore"])
    _, _, _, losses = H.run_smoke_config("nov-adam_sam_test", tmp_path, ["run.fp16=false", "random_seed=0", "data.pool=2"])
    assert len(made) == 1 and (made[0].rho, made[0].eta) == (0.5, 0.01) and made[0].forwards > 0
    assert calls[:4] == ["sam_sumsq", "sam_scale", "sam_perturb", "sam_restore"] and len(calls) == 4 * made[0].forwards  # four launches a step
    print("nov-adam_sam_test train losses:", losses, " SAM steps:", made[0].forwards, " last norm:", float(made[0].norm))
    assert losses and all(math.isfinite(x) for x in losses) and math.isfinite(float(made[0].norm))


_DDP_SAM_CHECK = r"""
import os, torch, torch.distributed as dist
from sota_imagenet_amd import fit_wrapper as fw
from sota_imagenet_amd.callbacks import SAMOriginal
from sota_imagenet_amd.losses import CrossEntropyLoss
from sota_imagenet_amd.models import resnet50
from sota_imagenet_amd.optim import AdamLayerwise
from sota_imagenet_amd.parallel import FlatBucketDDP
from sota_imagenet_amd.synth import synthetic_batch
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
dist.init_process_group("nccl", init_method="env://", world_size=world, rank=rank)
m = resnet50(dtype="fp32").cuda()
ddp = FlatBucketDDP(m, device_ids=[torch.cuda.current_device()], bucket_cap_mb=8.0)
ddp.comm_stats()
opt = AdamLayerwise([{"params": list(m.parameters())}], lr=1e-3, betas=(0.9, 0.995), weight_decay=2e-2)
sam = SAMOriginal()
logs = []
class Stats(fw.Callback):
    def on_batch_end(self):
        logs.append(ddp.comm_stats())
class Loader:
    batch_size = 4
    def __len__(self):
        return 2
    def __iter__(self):
        return iter([synthetic_batch(4, 64, seed=31, stream=rank, index=i, device="cuda") for i in range(2)])
runner = fw.Runner(ddp, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[sam, Stats()])
runner.fit(Loader(), epochs=1)
torch.cuda.synchronize()
plan = [(0, b, e) for b, e, _ in ddp.buckets]
# step 1 is a plain step: one reduced backward; step 2 reduces the first gradient (the norm is that of the mean gradient) AND the second one
assert len(plan) >= 3 and logs[0] == plan and logs[1] == plan + plan, (logs, plan)
assert sam.forwards == 1 and torch.isfinite(m.flat_params).all() and torch.isfinite(sam.norm).all()
print(f"SAM-DDP-OK rank {rank} norm {float(sam.norm):.6g}")
dist.barrier()
dist.destroy_process_group()
"""


def test_single_rank_under_the_native_rccl_wrapper(dev):
    """two Runner steps over FlatBucketDDP on a 1-rank RCCL communicator: the second forward goes through the wrapper, so the second gradient is
    reduced like the first (the communicator's log shows the bucket plan twice in the SAM step)"""
    path = os.path.join(ROOT, "tests", "_sam_ddp_check.py")
    with open(path, "w") as f:
        f.write(_DDP_SAM_CHECK)
    try:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", PYTHONPATH=ROOT)
        out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                              "--master-port", "29541", path], capture_output=True, text=True, env=env, timeout=600)
    finally:
        os.remove(path)
    assert out.returncode == 0 and "SAM-DDP-OK rank 0" in out.stdout, (out.stdout[-800:], out.stderr[-2500:])
