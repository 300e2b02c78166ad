"""Native SAM (csrc/optim_sam_lw.hip, callbacks.SAM) on the MI355X: the kernels against torch on the same arrays (the norms to the summation
bound, the elementwise stages bit for bit), the callback over the native optimizers against the trajectories recorded from the reference's own
callback (tests/golden/sam_lw_ref_trajectories.npz, the yardstick rule of tests/optim_harness.py), and the callback inside Runner on the real models:
what the second forward sees, what it leaves behind, how many launches a step makes."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_harness as H
from optim_harness import NAN, U
from plan_common import layout, table
from sam_lw_common import CASES, Fixture, generator

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 123.0
RHO = 0.01
GN_FLOOR, WN_FLOOR = float(np.float32(1e-5)), float(np.float32(1e-3))
SHAPES = [(16, 3, 3, 3), (32, 16, 1, 1), (10, 37), (37, 113), (7, 147), (2, 1), (3, 4099), (5, 64), (1,), (5,), (4097,)]


# ---- the kernels, driven directly --------------------------------------------------------------------------------------------------------
class _Arrays:
    """SHAPES laid out in `nbuf` pairs of flat parameter / gradient buffers (tensor i in pair i % nbuf) at 64-element aligned offsets: the
    sentinel in every gap of p and eps, NaN in every gap of g, and the tables of SAM.plan_tables on the device"""

    def __init__(self, vals, grads, dev, nbuf, unitwise):
        from sota_imagenet_amd import ops
        from sota_imagenet_amd.callbacks import SAM

        self.sizes = sizes = [int(np.prod(s)) for s in SHAPES]
        self.nbuf, self.unitwise = nbuf, unitwise
        members = [[i for i in range(len(sizes)) if i % nbuf == b] for b in range(nbuf)]
        self.where, self.fp, self.fg, self.mask = {}, [], [], []
        for b, idx in enumerate(members):
            offs, n = layout([sizes[i] for i in idx])
            fp, fg = torch.full((n,), SENTINEL, device=dev), torch.full((n,), NAN, device=dev)
            mask = torch.zeros(n, dtype=torch.bool, device=dev)
            for i, o in zip(idx, offs):
                fp[o:o + sizes[i]] = vals[i].reshape(-1).to(dev)
                fg[o:o + sizes[i]] = grads[i].reshape(-1).to(dev)
                mask[o:o + sizes[i]] = True
                self.where[i] = (b, o)
            self.fp.append(fp), self.fg.append(fg), self.mask.append(mask)
        self.order = order = [i for idx in members for i in idx]
        self.unit = {i: (sizes[i] // SHAPES[i][0] if unitwise and len(SHAPES[i]) > 1 else sizes[i]) for i in order}
        tensors = [(self.fp[self.where[i][0]].data_ptr(), self.fg[self.where[i][0]].data_ptr(), self.where[i][1], sizes[i], self.unit[i]) for i in order]
        self.tab = tab = SAM.plan_tables(tensors, ops.lw_item_elems())
        assert len(tab["pairs"]) == nbuf
        self.slot0 = {i: tab["tensors"][j][2] for j, i in enumerate(order)}
        self.items, self.tensors = table(tab["items"], dev), table(tab["tensors"], dev)
        self.pieces, self.whole = table(tab["pieces"], dev), table(tab["whole"], dev)
        self.slots = torch.tensor(tab["slots"], dtype=torch.int32, device=dev)
        ns = len(tab["slots"])
        self.partial = torch.full((2 * (len(tab["pieces"]) + len(tab["whole"])),), NAN, dtype=torch.float64, device=dev)
        self.coef, self.norms = torch.full((ns,), NAN, device=dev), torch.full((ns, 2), NAN, device=dev)
        self.eps = [torch.full_like(fp, SENTINEL) for fp in self.fp]

    def sums_and_coef(self, gs, threads_per_piece=None):
        from sota_imagenet_amd import ops

        kw = {} if threads_per_piece is None else dict(threads_per_piece=threads_per_piece)
        nt, ns = self.tensors.shape[0], self.coef.numel()
        for b, (lo, hi, i0, i1, (pa, pb), (wa, wb), k0, _) in enumerate(self.tab["pairs"]):
            k1 = k0 + pb - pa
            if pb > pa:
                ops.sam_unit_sumsq(self.fp[b][lo:hi], self.fg[b][lo:hi], self.pieces[pa:pb], self.partial[2 * k0:2 * k1], ns, grad_scale=gs, **kw)
            if wb > wa:
                ops.sam_lw_sumsq(self.fp[b][lo:hi], self.fg[b][lo:hi], self.whole[wa:wb], self.partial[2 * k1:2 * (k1 + wb - wa)], nt, grad_scale=gs)
        ops.sam_lw_coef(self.partial, self.slots, self.coef, self.norms)

    def perturb(self, gs, rho=RHO):
        from sota_imagenet_amd import ops

        for b, (lo, hi, i0, i1, *_) in enumerate(self.tab["pairs"]):
            ops.sam_lw_perturb(self.fp[b][lo:hi], self.fg[b][lo:hi], self.eps[b][lo:hi], self.items[i0:i1], self.tensors, self.coef, rho, grad_scale=gs)

    def restore(self):
        from sota_imagenet_amd import ops

        for b, (lo, hi, i0, i1, *_) in enumerate(self.tab["pairs"]):
            ops.sam_restore(self.fp[b][lo:hi], self.eps[b][lo:hi], self.items[i0:i1], self.tensors.shape[0])

    def tensor(self, bufs, i):
        b, o = self.where[i]
        return bufs[b][o:o + self.sizes[i]]

    def slot_range(self, i):
        return slice(self.slot0[i], self.slot0[i] + self.sizes[i] // self.unit[i])


def _problem(dev, nbuf=1, unitwise=True, zero_grad=False, seed=5):
    """values in +-0.5 and gradients of very different magnitude per tensor; [32,16,1,1] has gradients of 1e-9 (the gradient floor alone, whole
    and row by row), [5,64] values of 1e-6 (the weight floor alone, whole and row by row), the 1-D tensor of 5 both, row 3 of [10,37] tiny
    values and row 5 of it tiny gradients (one floor each, for that unit only)"""
    gen = torch.Generator().manual_seed(seed)
    vals = [torch.rand(s, generator=gen) - 0.5 for s in SHAPES]
    grads = [torch.zeros(s) if zero_grad else torch.randn(s, generator=gen) * (10.0 ** (i % 4 - 2)) for i, s in enumerate(SHAPES)]
    vals[7] *= 1e-6
    vals[9] *= 1e-4
    vals[2][3] *= 1e-5
    if not zero_grad:
        grads[1] *= 1e-9
        grads[9] *= 1e-9
        grads[2][5] *= 1e-9
    return _Arrays(vals, grads, dev, nbuf, unitwise)


def _reference_norms(A, gs):
    """per slot, in the table's slot numbering: sqrt of the float64 sums of squares of the float32 operands ge = g * gs and p, and the slot lengths"""
    ns = A.coef.numel()
    gn, wn, ln = torch.zeros(ns, dtype=torch.float64), torch.zeros(ns, dtype=torch.float64), torch.zeros(ns, dtype=torch.int64)
    for i in range(len(A.sizes)):
        ge, p = (A.tensor(A.fg, i) * gs).double().view(-1, A.unit[i]), A.tensor(A.fp, i).double().view(-1, A.unit[i])
        r = A.slot_range(i)
        gn[r], wn[r], ln[r] = ge.pow(2).sum(1).sqrt().cpu(), p.pow(2).sum(1).sqrt().cpu(), A.unit[i]
    return gn, wn, ln


def _coef_by_element(A, i):
    return torch.repeat_interleave(A.coef[A.slot_range(i)], A.unit[i])


@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("nbuf", [1, 2])
@pytest.mark.parametrize("unitwise,tpp", [(False, None), (True, 64), (True, 256)])
def test_norms_equal_the_float64_sums_of_the_float32_operands(dev, gs, nbuf, unitwise, tpp):
    """per slot, gn and wn against max(sqrt of the float64 sum of squares of the float32 operands, floor): relative error <= len * 2^-53 (the
    worst-case summation bound in double) + 2^-24 (the one rounding to float); a slot under its floor sits on it exactly; coef = wn / gn, rounded
    once.  NaN in every gap of the gradient buffer and a sentinel in every gap of the parameter buffer: a gap read into a sum would show.  One
    wave and one workgroup per piece both."""
    A = _problem(dev, nbuf, unitwise)
    p0 = [fp.clone() for fp in A.fp]
    A.sums_and_coef(gs, tpp)
    torch.cuda.synchronize()
    assert torch.isfinite(A.partial).all() and all(torch.equal(a, b) for a, b in zip(A.fp, p0))
    gn64, wn64, ln = _reference_norms(A, gs)
    got = A.norms.cpu().double()
    for what, ref, floor, col in (("gn", gn64, GN_FLOOR, 0), ("wn", wn64, WN_FLOOR, 1)):
        assert ((ref - floor).abs() > 1e-4 * floor).all()  # no slot of this problem sits at the edge of a floor
        under = ref < floor
        assert under.any() and (~under).any() and (got[under, col] == floor).all(), what
        rel = ((got[:, col] - ref).abs() / ref)[~under]
        bound = (ln.double() * 2.0 ** -53 + 2.0 ** -24)[~under]
        print(f"{what} unitwise={unitwise} tpp={tpp} gs={gs} pairs={nbuf}: {int((~under).sum())} slots, worst relative error {rel.max():.3e} "
              f"(bound {bound.min():.3e}), {int(under.sum())} on the floor")
        assert (rel <= bound).all(), what
    combos = {(bool(a), bool(b)) for a, b in zip(gn64 < GN_FLOOR, wn64 < WN_FLOOR)}
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    n = A.norms.cpu().numpy()
    assert np.array_equal(A.coef.cpu().numpy(), n[:, 1] / n[:, 0])
    assert A.coef.numel() == (sum(s[0] if len(s) > 1 else 1 for s in SHAPES) if unitwise else len(SHAPES))
    if unitwise:
        # 112 units; each row of 4099 is two pieces; 56 pieces start off a 16-byte boundary
        assert len(A.tab["pieces"]) == 112 + 3 and sum(1 for p in A.tab["pieces"] if p[0] % 4) == 56


def test_zero_gradient_sits_on_the_floor_of_the_gradient_norm(dev):
    for unitwise in (False, True):
        A = _problem(dev, 2, unitwise, zero_grad=True)
        before = [fp.clone() for fp in A.fp]
        A.sums_and_coef(1.0)
        A.perturb(1.0)
        torch.cuda.synchronize()
        assert (A.norms[:, 0] == GN_FLOOR).all() and torch.isfinite(A.coef).all() and (A.coef > 0).all()
        assert all((e[m] == 0).all() and (e[~m] == SENTINEL).all() for e, m in zip(A.eps, A.mask))
        assert all(torch.equal(a, b) for a, b in zip(A.fp, before))


@pytest.mark.parametrize("gs", [1.0, 0.25])
@pytest.mark.parametrize("nbuf", [1, 2])
@pytest.mark.parametrize("unitwise", [False, True])
def test_perturbation_and_restore_are_bitwise_torchs(dev, gs, nbuf, unitwise):
    """eps == (coef[slot] * (g*gs)) * rho in torch float32 on the device, the coefficient of every element by repeat_interleave — a vector that
    took its coefficient from its first lane would show in the rows of 27, 37, 113, 147, 4099 and 1 elements; p_after == p + eps and
    p_restored == p_after - eps, bit for bit; the gaps keep their bits in p, eps and g"""
    A = _problem(dev, nbuf, unitwise)
    A.sums_and_coef(gs)
    p0 = [fp.clone() for fp in A.fp]
    A.perturb(gs)
    p1 = [fp.clone() for fp in A.fp]
    A.restore()
    torch.cuda.synchronize()
    moved = 0
    for i in range(len(A.sizes)):
        p, g = A.tensor(p0, i), A.tensor(A.fg, i)
        want = (_coef_by_element(A, i) * (g * gs)) * RHO
        eps = A.tensor(A.eps, i)
        assert torch.equal(eps, want), f"eps of tensor {i} {SHAPES[i]}: {int((eps != want).sum())} elements differ"
        assert torch.equal(A.tensor(p1, i), p + eps) and torch.equal(A.tensor(A.fp, i), (p + eps) - eps)
        moved += int((A.tensor(p1, i) != p).any())
    assert moved == len(A.sizes)
    assert any(not torch.equal(a, b) for a, b in zip(A.fp, p0))  # (p + eps) - eps is not p everywhere
    for b in range(nbuf):
        gap = ~A.mask[b]
        assert gap.any() and (p1[b][gap] == SENTINEL).all() and (A.fp[b][gap] == SENTINEL).all() and (A.eps[b][gap] == SENTINEL).all()
        assert torch.isnan(A.fg[b][gap]).all() and torch.isfinite(A.fp[b]).all()


def test_rho_zero_is_legal_and_perturbs_nothing(dev):
    A = _problem(dev, 1, True)
    A.sums_and_coef(1.0)
    p0 = A.fp[0].clone()
    A.perturb(1.0, rho=0.0)
    torch.cuda.synchronize()
    assert torch.equal(A.fp[0], p0) and (A.eps[0][A.mask[0]] == 0).all()


def test_replay_and_placement_are_bitwise(dev):
    """the same launches twice give the same bits; every tensor in a storage pair of its own (eleven launch sets) gives the eps and the norms of
    the one-pair layout: pieces and items are cut from the start of their unit / tensor, and every tensor starts on a 16-byte boundary"""
    res = []
    for nbuf in (2, 2, 1, len(SHAPES)):
        A = _problem(dev, nbuf, True)
        A.sums_and_coef(0.25)
        A.perturb(0.25)
        torch.cuda.synchronize()
        res.append(A)
    a, b = res[0], res[1]
    assert torch.equal(a.partial, b.partial) and torch.equal(a.coef, b.coef) and torch.equal(a.norms, b.norms)
    assert all(torch.equal(x, y) for x, y in zip(a.eps, b.eps))
    one = res[2]
    for other in (res[0], res[3]):
        assert len(other.tab["pairs"]) == other.nbuf
        for i in range(len(SHAPES)):
            assert torch.equal(one.tensor(one.eps, i), other.tensor(other.eps, i)), i
            assert torch.equal(one.norms[one.slot_range(i)], other.norms[other.slot_range(i)]), i


# ---- the callback over the native optimizers, on the fixture's problem --------------------------------------------------------------------
def _run_fixture(fx, dev, separate=False):
    """the fixture's three steps through fit_wrapper.Runner with the native optimizer and the native callback; parameters laid out group by
    group in one flat buffer pair (NaN in the gradient's gaps, the sentinel in the parameter's), or each tensor in a storage of its own"""
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAM

    gen = generator()
    order = [i for idx in fx.groups for i in idx]
    offs, n = layout(fx.sizes, order)
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
    sam = SAM(unitwise=fx.unitwise, rho=fx.rho)
    rec = dict(eps=[], norms=[], step=[], fp_pairs=[], forwards=[])

    class Before(fw.Callback):
        def on_batch_begin(self):
            for g in self.state.optimizer.param_groups:
                g["lr"] = fx.lrs[self.state.step]

        def on_after_backward(self):
            rec["fp_before"] = fp.clone()

    class After(fw.Callback):
        def on_after_backward(self):
            rec["fp_pairs"].append((rec["fp_before"], fp.clone()))
            e = sam.eps_flat
            rec["eps"].append([t.clone() for t in e] if isinstance(e, list) else e.clone())
            rec["norms"].append(sam.norms.clone())

        def on_batch_end(self):
            rec["step"].append(torch.cat([p.detach().reshape(-1) for p in ps]).clone())
            rec["forwards"].append(len(model.seen))

    class Loader:
        batch_size = 1

        def __len__(self):
            return fx.steps

        def __iter__(self):
            return iter([([c.to(dev) for c in fx.targets(k)], None) for k in range(fx.steps)])

    runner = fw.Runner(model, opt, gen.criterion, callbacks=[Before(), sam, After()])
    runner.fit(Loader(), epochs=1)
    torch.cuda.synchronize()
    return dict(rec=rec, sam=sam, ps=ps, fp=fp, fg=fg, offs=offs, seen=model.seen, order=order)


def _fixture_order_norms(fx, r, norms):
    """the callback's norms [slots, 2] (slots in param-group order) in the fixture's order (tensor by tensor)"""
    by_tensor = {i: norms[s0:s0 + cnt] for i, (s0, cnt) in zip(r["order"], r["sam"].slot_ranges)}
    return torch.cat([by_tensor[i] for i in range(len(fx.shapes))]).cpu().double()


@pytest.mark.parametrize("case", CASES)
def test_callback_follows_the_reference_trajectory(dev, case):
    """the three recorded cases (the reference callback layer-wise and unit-wise over torch SGD, unit-wise over its own AdamLayerwise with recipe
    49's values) with the native callback over the native optimizers: eps, the parameters the second forward saw and the parameters after every
    step within 1.5 x the reference's own float32 error + 4 * 2^-24 * max|ref| of the reference's float64 run; gn and wn per slot within
    4 * 2^-24 relative; every step makes two forwards, the first included.  The callback never touches the gaps of the flat buffers."""
    fx = Fixture(case)
    r = _run_fixture(fx, dev)
    rec, sam = r["rec"], r["sam"]
    assert [b - a for a, b in zip([0] + rec["forwards"], rec["forwards"])] == fx.forwards == [2, 2, 2] and sam.forwards == 3
    assert len(sam._segs) == 1 and sam.coef.numel() == sum(fx.slot_counts)
    worst = 0.0
    for k in range(fx.steps):
        eps = torch.cat([rec["eps"][k][r["offs"][i]:r["offs"][i] + fx.sizes[i]] for i in range(len(fx.sizes))])
        worst = max(worst, fx.check(k, rec["step"][k], "step"), fx.check(k, eps, "eps"), fx.check(k, r["seen"][2 * k + 1], "pert"))
        got = _fixture_order_norms(fx, r, rec["norms"][k])
        for what, col, ref in (("gn", 0, fx.gn[k]), ("wn", 1, fx.wn[k])):
            ref = torch.from_numpy(ref)
            rel = ((got[:, col] - ref).abs() / ref).max().item()
            print(f"{case} step {k + 1}: {what} worst relative error {rel:.3e} over {ref.numel()} slots")
            assert rel <= 4 * U, (case, what, k, rel)
    print(f"{case}: worst native error / max(reference-fp32 error, floor) {worst:.2f}")
    fp, fg = r["fp"], r["fg"]
    gap = torch.ones_like(fp, dtype=torch.bool)
    for o, s in zip(r["offs"], fx.sizes):
        gap[o:o + s] = False
    assert gap.any() and torch.isnan(fg[gap]).all() and torch.isfinite(fp[~gap]).all()
    for before, after in rec["fp_pairs"]:  # across the callback the gaps keep their bits; the tensors come back to within rounding
        assert torch.equal(before.view(torch.int32)[gap], after.view(torch.int32)[gap]) and not torch.equal(before, after)
    if fx.cls != "SGD":  # (the native SGD merges neighbouring ranges and sweeps the 64-element gaps between them; the layer-wise step does not)
        assert (fp[gap] == SENTINEL).all()
    assert (sam.eps_flat[gap[:sam.eps_flat.numel()]] == 0).all()


@pytest.mark.parametrize("case", CASES)
def test_placement_is_bitwise(dev, case):
    """every tensor in a parameter / gradient storage of its own (six launch sets, one coefficient launch over all of them) gives the parameters
    of the flat-buffer run bit for bit after every step, the same eps and the same norms"""
    fx = Fixture(case)
    a, b = _run_fixture(fx, dev), _run_fixture(fx, dev, separate=True)
    assert len(a["sam"]._segs) == 1 and len(b["sam"]._segs) == 6
    for k in range(fx.steps):
        assert torch.equal(a["rec"]["step"][k], b["rec"]["step"][k])
        flat = torch.cat([a["rec"]["eps"][k][a["offs"][i]:a["offs"][i] + fx.sizes[i]] for i in a["order"]])
        assert torch.equal(flat, torch.cat(b["rec"]["eps"][k])) and torch.equal(a["rec"]["norms"][k], b["rec"]["norms"][k])


def test_parameters_that_do_not_fit_raise(dev):
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd.callbacks import SAM

    def state_of(p, **kw):
        sam = SAM(**kw)
        sam.set_state(fw.RunnerState(model=None, optimizer=torch.optim.SGD([p], lr=0.1), criterion=None))
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
    p = torch.nn.Parameter(torch.zeros(6, 4, device=dev).t())  # dense, but dim 0 is the innermost stride
    p.grad = torch.zeros(6, 4, device=dev).t()
    with pytest.raises(RuntimeError, match="outermost"):
        state_of(p, unitwise=True).on_after_backward()


# ---- the callback inside Runner on the real models ------------------------------------------------------------------------------------------
def _model(kind):
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.models import resnet50

    if kind == "bresnet50-bf16":
        return BResNet50(dtype="bf16").cuda()
    return resnet50(dtype=kind.split("-")[1]).cuda()


_STAGES = ("sam_unit_sumsq", "sam_lw_sumsq", "sam_lw_coef", "sam_lw_perturb", "sam_restore")


_COUNTED = _STAGES + ("sam_sumsq", "sam_scale", "sam_perturb")


@pytest.mark.parametrize("unitwise", [False, True])
@pytest.mark.parametrize("kind", ["resnet50-fp32", "resnet50-bf16", "bresnet50-bf16"])
def test_three_runner_steps_on_the_real_model(dev, kind, unitwise, monkeypatch):
    """N = 4 at 64 px, AdamLayerwise with recipe 49's values, a spy before and one after SAM: num_batches_tracked reads 2, 4, 6 (every step is
    perturbed); the parameters the second forward saw are p0 + eps_flat and the callback leaves that minus eps_flat, bit for bit; the padding
    of the flat array never changes; 4 launches a step layer-wise, 5 unit-wise; loss and parameters stay finite.  fp32 unit-wise: the
    coefficients of the stem (rows of 147) and of layer4.2.conv2 (rows of 4608: two pieces each) against torch on the same arrays."""
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.callbacks import SAM
    from sota_imagenet_amd.losses import CrossEntropyLoss

    calls = H.count_launches(monkeypatch, _COUNTED)
    m = _model(kind)
    params = list(m.parameters())
    opt = optim.AdamLayerwise([{"params": params}], lr=1e-3, betas=(0.9, 0.995), weight_decay=2e-2)
    sam = SAM(unitwise=unitwise, rho=0.001)
    pad = H.padding_mask(m)
    pad0 = m.flat_params[pad].clone()
    nbt = next(b for n, b in m.named_buffers() if n.endswith("num_batches_tracked"))
    log = dict(seen=[], p0=[], g1=[], after=[], g_cb=[], eps=[], coef=[], nbt=[], finite=[])
    m.register_forward_pre_hook(lambda mod, inp: log["seen"].append(mod.flat_params.clone()))

    class Before(fw.Callback):
        def on_after_backward(self):
            log["p0"].append(m.flat_params.clone())
            log["g1"].append(m.flat_grads.clone())

    class After(fw.Callback):
        def on_after_backward(self):
            log["after"].append(m.flat_params.clone())
            log["g_cb"].append(m.flat_grads.clone())
            log["eps"].append(sam.eps_flat.clone())
            log["coef"].append(sam.coef.clone())

        def on_batch_end(self):
            log["nbt"].append(int(nbt))
            log["finite"].append(bool(torch.isfinite(m.flat_params).all()) and bool(torch.isfinite(self.state.loss_meter.val)))

    runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[Before(), sam, After()])
    runner.fit(H.Loader(), epochs=1)
    torch.cuda.synchronize()
    assert log["nbt"] == [2, 4, 6] and all(log["finite"]) and math.isfinite(runner.state.loss_meter.avg)
    assert len(log["seen"]) == 6 and sam.forwards == 3 and len(sam._segs) == 1
    per_step = list(_STAGES[1:] if not unitwise else _STAGES)
    assert calls == per_step * 3, calls[:8]
    weights = [p for p in params if p.ndim > 1]
    assert sam.coef.numel() == (sum(p.shape[0] for p in weights) + len(params) - len(weights) if unitwise else len(params))
    for k in range(3):
        p0, eps = log["p0"][k], torch.zeros_like(log["p0"][k])
        eps[:log["eps"][k].numel()] = log["eps"][k]
        assert torch.equal(log["seen"][2 * k], p0)
        assert (eps[pad] == 0).all() and (eps[~pad] != 0).float().mean().item() > 0.5 and torch.isfinite(eps).all()
        assert torch.equal(log["seen"][2 * k + 1], p0 + eps)
        assert torch.equal(log["after"][k], (p0 + eps) - eps)
        g1, g_cb = log["g1"][k][~pad], log["g_cb"][k][~pad]
        assert torch.isfinite(g_cb).all() and not torch.equal(g_cb, g1)
        print(f"{kind} unitwise={unitwise} step {k + 1}: max |eps| {eps.abs().max().item():.3e}  coef {log['coef'][k].min().item():.3e} .. "
              f"{log['coef'][k].max().item():.3e}")
    assert torch.equal(m.flat_params[pad], pad0) and not torch.equal(m.flat_params, log["p0"][0])
    if kind == "resnet50-fp32" and unitwise:
        names = [n for n, _ in m.named_parameters()]
        for name, rows in (("conv1.weight", 147), ("layer4.2.conv2.weight", 4608)):
            j = names.index(name)
            p = params[j]
            off = (p.data_ptr() - m.flat_params.data_ptr()) // 4
            s0, cnt = sam.slot_ranges[j]
            assert cnt == p.shape[0] and p.numel() // cnt == rows
            for k in range(3):
                w = log["p0"][k][off:off + p.numel()].double().view(cnt, rows)
                g = log["g1"][k][off:off + p.numel()].double().view(cnt, rows)
                want = w.pow(2).sum(1).sqrt().clamp_min(WN_FLOOR) / g.pow(2).sum(1).sqrt().clamp_min(GN_FLOOR)
                rel = ((log["coef"][k][s0:s0 + cnt].double() - want).abs() / want).max().item()
                print(f"{name} step {k + 1}: coef worst relative error {rel:.3e}")
                assert rel <= 4 * U  # two norms and a quotient, each rounded once to float32


# ---- smoke: train.py and the data-parallel wrapper --------------------------------------------------------------------------------------------
def test_train_py_runs_the_smoke_config(dev, tmp_path, monkeypatch):
    """train.py on nov-adam_sam-unit_test: the native callback is built from the reference's target, perturbs in every step with five launches,
    and the losses are finite"""
    from sota_imagenet_amd import callbacks

    made = []
    init = callbacks.SAM.__init__
    monkeypatch.setattr(callbacks.SAM, "__init__", lambda self, *a, **k: (made.append(self), init(self, *a, **k))[1])
    calls = H.count_launches(monkeypatch, _COUNTED)
    _, _, _, losses = H.run_smoke_config("nov-adam_sam-unit_test", tmp_path, ["run.fp16=false", "random_seed=0", "data.pool=2"])
    assert len(made) == 1 and (made[0].rho, made[0].unitwise) == (0.001, True) and made[0].forwards > 0
    assert calls[:5] == list(_STAGES) and len(calls) == 5 * made[0].forwards
    print("nov-adam_sam-unit_test train losses:", losses, " SAM steps:", made[0].forwards)
    assert losses and all(math.isfinite(x) for x in losses) and torch.isfinite(made[0].coef).all()


_DDP_SAM_CHECK = r"""
import os, torch, torch.distributed as dist
from sota_imagenet_amd import fit_wrapper as fw
from sota_imagenet_amd.callbacks import SAM
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
sam = SAM(unitwise=True, rho=0.001)
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
# every step reduces the first gradient (the norms are those of the mean gradient) AND the second one
assert len(plan) >= 3 and logs[0] == plan + plan and logs[1] == plan + plan, (logs, plan)
assert sam.forwards == 2 and torch.isfinite(m.flat_params).all() and torch.isfinite(sam.coef).all()
print(f"SAM-LW-DDP-OK rank {rank} coef {float(sam.coef.min()):.6g} .. {float(sam.coef.max()):.6g}")
dist.barrier()
dist.destroy_process_group()
"""


def test_single_rank_under_the_native_rccl_wrapper(dev):
    """two Runner steps over FlatBucketDDP on a 1-rank RCCL communicator: the second forward goes through the wrapper, so the second gradient is
    reduced like the first (the communicator's log shows the bucket plan twice in every step)"""
    path = os.path.join(ROOT, "tests", "_sam_lw_ddp_check.py")
    with open(path, "w") as f:
        f.write(_DDP_SAM_CHECK)
    try:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", PYTHONPATH=ROOT)
        out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                              "--master-port", "29547", path], capture_output=True, text=True, env=env, timeout=600)
    finally:
        os.remove(path)
    assert out.returncode == 0 and "SAM-LW-DDP-OK rank 0" in out.stdout, (out.stdout[-800:], out.stderr[-2500:])
