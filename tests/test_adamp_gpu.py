"""Native AdamP (csrc/optim_adamp.hip, optim.AdamP) on the MI355X against the torch restatement of adamp.AdamP.step (tests/adamp_common.py; the
fixture tests/golden/adamp_ref_trajectories.npz recorded from it on the CPU).  The `adamp` package is not available to this project: the rule is
written down from memory of the public package and parity is unpinned against the package itself.

Yardstick, stored in the fixture and never computed from the code under test: the rule of this family (tests/optim_harness.py, within_yardstick)
— FACTOR = 1.5 times the restatement's own float32 error plus a floor of 4 * 2^-24 of the largest parameter magnitude.  At model scale the same rule with the restatement's
float32 run as the yardstick.  The update kernel alone is compared bit for bit with the float32 restatement that is handed the device's own
coefficients."""
import copy
import ctypes
import math
import os
import sys

import pytest
import torch

import optim_harness as H
from adamp_common import CASES, Fixture, Restated, slot_rows
from optim_harness import NAN, U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture_opt(fx, dev, values=None):
    from sota_imagenet_amd import optim

    ps, fp, fg, _ = H.flat_params(fx.sizes, fx.shapes, fx.split(fx.p0) if values is None else values, dev, fx.order)
    groups = [{"params": [ps[i] for i in idx], "weight_decay": wd} for idx, wd in zip(fx.groups, fx.wds)]
    return optim.AdamP(groups, lr=fx.lrs[0], **fx.hyper), ps, fp, fg


def _fixture_steps(fx, opt, ps, steps, grad_scale=1.0, each=None):
    opt.grad_scale = grad_scale
    for k in steps:
        for g in opt.param_groups:
            g["lr"] = fx.lrs[k]
        H.set_grads(ps, fx.split(fx.grads[k]), 1.0 / grad_scale)  # (exact: a power of two)
        opt.step()
        if each:
            each(k)
    torch.cuda.synchronize()


# ---- 1. trajectories --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_steps_follow_the_restated_trajectory(dev, case):
    """four steps on the fixture's inputs, gradients and lr ramp in one flat array: at every step projection_modes equals the stored modes and
    every tensor meets the stored yardstick; the same again with grad_scale = 0.5 on doubled gradients.  The gaps are never touched."""
    fx = Fixture(case)
    worst = 0.0
    for gs in (1.0, 0.5):
        opt, ps, fp, fg = _fixture_opt(fx, dev)

        def each(k):
            nonlocal worst
            modes = opt.projection_modes
            assert modes.is_cuda and modes.dtype == torch.int32
            assert [int(x) for x in modes.cpu()] == [int(fx.modes[k, i]) for i in fx.order], f"{case} step {k + 1}: modes"
            worst = max(worst, fx.check(k, [p.detach() for p in ps], f"{case} grad_scale={gs}"))

        _fixture_steps(fx, opt, ps, range(4), gs, each)
        gaps = H.gaps(ps, fp)
        assert gaps.any() and (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all() and torch.isfinite(fp).all()
        assert all(opt.state[p]["step"] == 4 and type(opt.state[p]["step"]) is int for p in ps)
        assert [c for _, c in opt.slot_ranges] == [slot_rows(ps[i]).shape[0] for i in fx.order]
    print(f"{case}: worst native / restated-fp32 error ratio {worst:.2f}")
    # the moments after the last step against the restatement's float32 state
    for key in ("exp_avg", "exp_avg_sq"):
        for i, (p, want) in enumerate(zip(ps, fx.split(fx.state4[key]))):
            got = opt.state[p][key].cpu()
            # (per step and side at most three roundings of the moment's magnitude, the coefficient's included: 4 * (3 + 3) * 2^-24)
            assert got.shape == p.shape and ((got - want).abs() <= 24 * U * want.abs().max()).all(), f"{case} {key} tensor {i}"


# ---- the tensors of tests 2 to 4 --------------------------------------------------------------------------------------------------------------
SMALL = [(8, 3, 7, 7), (2, 2 * 4096 + 808), (7, 1), (5, 3), (1, 33), (1, 4100), (3, 4), (4097,), (5,), (1,)]
SMALL_MODES = [1, 1, 0, 2, 1, 1, 0, 0, 0, 0]  # what the gradients below are built for


def _small_problem(dev, seed):
    from adamp_common import GEN

    gen = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=gen) * (0.02 * 2.0 ** (i % 3)) for i, s in enumerate(SMALL)]
    ps, fp, fg, _ = H.flat_params([math.prod(s) for s in SMALL], SMALL, vals, dev)
    kinds = {1: "channel", 2: "layer", 0: "none"}

    def grads(k):
        """gradients that put the projection on per unit, per layer and off, built like the fixture's (the recorder's make_grad) from the
        parameters as they are now"""
        return [GEN.make_grad(kinds[m] if len(s) > 1 else "1d", p.detach().cpu(), gen) * (1.0 + k) for p, s, m in zip(ps, SMALL, SMALL_MODES)]

    return vals, grads, ps, fp, fg


def _per_tensor(opt, t):
    return [t[s0:s0 + cnt].clone() for s0, cnt in opt.slot_ranges]


# ---- 2. stage (a) -----------------------------------------------------------------------------------------------------------------------------
def test_unit_sums_equal_the_float64_sums(dev):
    """147-long units at every alignment, a unit of three pieces, f32x4 covering several units ((7,1), (5,3)), dim 0 of 1 with one and with two
    pieces, NaN in every gap of the gradient, a non-zero first and second moment (the second step), nesterov, grad_scale 0.5: the four sums of
    every piece, summed per slot, equal the float64 sums over the float32 operands the kernel documents to 1e-12 relative (sum g*p and sum
    p*u, which cancel, relative to the sum of the magnitudes); stage (a) writes none of p, g, m, v"""
    from adamp_common import native_direction
    from sota_imagenet_amd import ops, optim

    vals, grads, ps, fp, fg = _small_problem(dev, seed=21)
    h = dict(betas=(0.8, 0.95), eps=1e-5, nesterov=True)
    opt = optim.AdamP(ps, lr=1e-3, weight_decay=1e-2, **h)
    opt.grad_scale = 0.5
    H.set_grads(ps, grads(0))
    opt.step()
    H.set_grads(ps, grads(1))
    torch.cuda.synchronize()
    seg, = opt._segs
    before = [t.clone() for t in (seg.p, seg.g, seg.m, seg.v)]
    partial = torch.full_like(opt._partial, NAN)
    (gi, a, b, k), = seg.sums
    assert (a, b, k) == (0, opt._sum_pieces.shape[0], 0) and b == 8 + 6 + 7 + 5 + 1 + 2 + 3
    ops.adamp_unit_sums(seg.p, seg.g, seg.m, seg.v, opt._sum_pieces[a:b], partial[k:k + b - a], opt._coef.shape[0], 2, grad_scale=0.5, **h)
    torch.cuda.synchronize()
    for t, t0 in zip((seg.p, seg.g, seg.m, seg.v), before):
        assert torch.equal(t, t0) or (torch.isnan(t) == torch.isnan(t0)).all() and torch.equal(torch.nan_to_num(t), torch.nan_to_num(t0))
    assert torch.isfinite(partial[:b]).all() and torch.isnan(partial[b:]).all()  # the entries of the 1-D tensors are not written
    slots, part = opt._slots.cpu(), partial.cpu()
    worst = 0.0
    for p, (s0, cnt) in zip(ps, opt.slot_ranges):
        if p.dim() <= 1:
            continue
        pc, g = p.detach().cpu(), p.grad.cpu()
        ge, _, _, u = native_direction(pc, g, opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu(), dict(h), 2, 0.5)
        P, G, Uu = slot_rows(pc).double(), slot_rows(ge).double(), slot_rows(u).double()
        want = torch.stack([(G * G).sum(1), (P * P).sum(1), (G * P).sum(1), (P * Uu).sum(1)], 1)
        scale = torch.stack([(G * G).sum(1), (P * P).sum(1), (G * P).abs().sum(1), (P * Uu).abs().sum(1)], 1)
        got = torch.stack([part[int(f):int(f) + int(c)].sum(0) for f, c in slots[s0:s0 + cnt]])
        worst = max(worst, ((got - want).abs() / scale).max().item())
    print(f"unit sums: worst relative error {worst:.3e}")
    assert worst <= 1e-12


# ---- 3. stage (c), element by element -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("nesterov", [False, True], ids=["adam", "nesterov"])
def test_update_equals_the_float32_restatement_bit_for_bit(dev, nesterov, ema):
    """two steps (the second with non-zero moments), grad_scale 0.5, all three modes present: the float32 restatement, handed the device's own
    coef / wdf of each step, gives the native parameters, both moments and the moving average bit for bit — items inside one slot (the
    3-piece unit, the 1-D tensors) and items that span units (147-long units, (7,1), (5,3)); the _ema form gives the same p as the plain one"""
    from sota_imagenet_amd import optim

    vals, grads, ps, fp, fg = _small_problem(dev, seed=22)
    h = dict(betas=(0.9, 0.99), eps=1e-6, nesterov=nesterov, wd_ratio=0.25)
    opt = optim.AdamP(ps, lr=1e-3, weight_decay=0.05, **h)
    opt.grad_scale = 0.5
    r = Restated(h, vals, [0] * len(vals), [0.05], torch.float32, native=True)
    decay = 0.9 if ema else None
    if ema:
        fe = fp.clone()
        opt.attach_ema(fp, fe, decay)
        r.ema = [v.clone() for v in vals]
    for k, lr in enumerate((1e-3, 3e-3)):
        opt.param_groups[0]["lr"] = lr
        gk = grads(k)
        H.set_grads(ps, gk)
        opt.step()
        torch.cuda.synchronize()
        modes = [int(x) for x in opt.projection_modes.cpu()]
        assert modes == SMALL_MODES, modes
        coef, wdf = _per_tensor(opt, opt._coef), list(opt._wdf.clone())
        assert all(len(torch.unique(c[:, 0])) == c.shape[0] for c, m in zip(coef, modes) if m == 1)   # one coefficient pair per unit
        assert all(len(torch.unique(c, dim=0)) == 1 and c[0, 0] != 1 for c, m in zip(coef, modes) if m == 2)  # the layer's pair in every slot
        assert all((c == torch.tensor([1.0, 0.0], device=dev)).all() for c, m in zip(coef, modes) if m == 0)
        assert [float(w) for w in wdf] == [float(torch.tensor(1 - lr * 0.05 * (0.25 if m else 1.0), dtype=torch.float64).float()) for m in modes]
        r.step(gk, [lr], grad_scale=0.5, coef=coef, wdf=wdf, ema_decay=decay)
        for i, p in enumerate(ps):
            what = f"step {k + 1} tensor {i} {tuple(p.shape)} mode {modes[i]}"
            assert torch.equal(p.detach().cpu(), r.p[i]), f"{what}: parameters"
            assert torch.equal(opt.state[p]["exp_avg"].cpu(), r.st[i]["exp_avg"]), f"{what}: first moment"
            assert torch.equal(opt.state[p]["exp_avg_sq"].cpu(), r.st[i]["exp_avg_sq"]), f"{what}: second moment"
            if ema:
                o = (p.data_ptr() - fp.data_ptr()) // 4
                assert torch.equal(fe[o:o + p.numel()].cpu().view(p.shape), r.ema[i]), f"{what}: moving average"
    gaps = H.gaps(ps, fp)
    assert (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all()
    if ema:
        assert (fe[gaps] == 0).all()


# ---- 4. records that point outside ----------------------------------------------------------------------------------------------------------------
def test_records_outside_the_arrays_are_skipped(dev):
    """pieces, items, slot records and tensor records that do not lie inside the arrays of the launch: the kernels skip them and no array
    changes (a good record next to them is processed)"""
    from sota_imagenet_amd import ops
    from sota_imagenet_amd.item_plan import pack_records

    n = 256
    p, g, m, v = (torch.full((n,), x, device=dev) for x in (1.0, 2.0, 0.5, 0.25))
    kw = dict(betas=(0.9, 0.999), eps=1e-8)
    bad_pieces = pack_records([(-4, 8, 0), (n - 4, 8, 0), (0, 0, 0), (0, 4097, 0), (0, 8, 2), (0, 8, -1), (1 << 40, 8, 0), (0, 8, 0)], dev)
    partial = torch.full((8, 4), 7.0, dtype=torch.float64, device=dev)
    ops.adamp_unit_sums(p, g, m, v, bad_pieces, partial, 2, 1, **kw)
    torch.cuda.synchronize()
    assert (partial[:7] == 0).all() and partial[7, 0].item() == 8 * 4.0 and partial[7, 1].item() == 8.0  # skipped pieces sum to zero
    # stage (b): a tensor record past the slots, slot records past partial[]
    slots = torch.tensor([[0, 1], [6, 4], [-1, 1], [0, 0]], dtype=torch.int32, device=dev)
    decide = torch.tensor([[3, 2, 8, 1], [-1, 1, 8, 1], [0, 1, 0, 1], [1, 1, 8, 1], [2, 2, 8, 1], [0, 1, 8, 1]], dtype=torch.int32, device=dev)
    coef = torch.full((4, 2), 9.0, device=dev)
    wdf, mode = torch.full((6,), 9.0, device=dev), torch.full((6,), 9, dtype=torch.int32, device=dev)
    ops.adamp_coef(partial, slots, decide, coef, wdf, mode, 1e-3, 1e-2)
    torch.cuda.synchronize()
    assert (coef[1:] == 9).all() and (wdf[:5] == 9).all() and (mode[:5] == 9).all()
    assert mode[5].item() in (0, 1, 2) and (coef[0] != 9).all() and wdf[5].item() != 9
    # stage (c)
    p0 = p.clone()
    items = pack_records([(-4, 8, 0), (n - 4, 8, 0), (0, 0, 0), (0, 4100, 0), (0, 8, 1), (0, 8, -1), (2, 8, 0), (64, 8, 0)], dev)
    # the first seven items are bad under any tensor record; the last is good, unless its tensor record is not: unit_len 0, a negative slot,
    # a tensor that starts behind the item, a slot past coef[] (3 + 8, and (64 - 0) / 8 = 8 with slot0 = 0)
    for rec in ((0, 0, 0), (0, 8, -1), (128, 8, 0), (0, 8, 3), (0, 8, 0)):
        ops.adamp_update(p, g, m, v, items, pack_records([rec], dev), coef, wdf[:1], 1, 1e-3, **kw)
    torch.cuda.synchronize()
    assert torch.equal(p, p0) and (g == 2.0).all() and (m == 0.5).all() and (v == 0.25).all()
    ops.adamp_update(p, g, m, v, items, pack_records([(64, 8, 0)], dev), coef, wdf[:1], 1, 1e-3, **kw)  # the last item alone is good
    torch.cuda.synchronize()
    assert (p[64:72] != 1.0).all() and torch.equal(p[:64], p0[:64]) and torch.equal(p[72:], p0[72:]) and (m[64:72] != 0.5).all()


# ---- 5. resume ------------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_bit_for_bit(dev):
    """state_dict() carries the package's layout (step: int, exp_avg, exp_avg_sq in the parameter's shape); loaded into a fresh instance it
    continues the trajectory bit for bit; differing step counts inside a group are refused"""
    fx = Fixture("adamp_alt")
    opt, ps, _, _ = _fixture_opt(fx, dev)
    _fixture_steps(fx, opt, ps, range(2))
    sd = copy.deepcopy(opt.state_dict())
    mid = [p.detach().cpu().clone() for p in ps]
    assert sorted(sd["state"]) == list(range(8))
    for j, i in enumerate(fx.order):
        st = sd["state"][j]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and st["step"] == 2 and type(st["step"]) is int
        assert all(tuple(st[k].shape) == fx.shapes[i] and st[k].dtype == torch.float32 for k in ("exp_avg", "exp_avg_sq"))
    assert set(sd["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "delta", "wd_ratio", "nesterov", "params"}
    _fixture_steps(fx, opt, ps, range(2, 4))
    want = torch.cat([p.detach().reshape(-1) for p in ps])
    opt2, ps2, _, _ = _fixture_opt(fx, dev, mid)
    opt2.load_state_dict(copy.deepcopy(sd))
    _fixture_steps(fx, opt2, ps2, range(2, 4))
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in ps2]), want) and all(opt2.state[p]["step"] == 4 for p in ps2)
    opt3, ps3, _, _ = _fixture_opt(fx, dev, mid)  # without the state the steps differ
    _fixture_steps(fx, opt3, ps3, range(2, 4))
    assert not torch.equal(torch.cat([p.detach().reshape(-1) for p in ps3]), want)
    bad = copy.deepcopy(sd)
    bad["state"][1]["step"] = 5
    opt4, _, _, _ = _fixture_opt(fx, dev, mid)
    with pytest.raises(ValueError, match="different step counts"):
        opt4.load_state_dict(bad)


# ---- 6. the whole model ---------------------------------------------------------------------------------------------------------------------------
STAGES = ["adamp_unit_sums", "adamp_coef", "adamp_update"]
KW = dict(weight_decay=1e-2, eps=1e-8)


def _model_opt(groups_of=None):
    return H.model_opt("AdamP", KW, 1e-3, groups_of)


def test_two_steps_at_model_scale(dev, monkeypatch):
    """two steps on a real resnet50 flat array (161 tensors, alignment gaps, FC padding; NaN in the gradient's padding) on random gradients
    against the float64 restatement on the CPU, tensor by tensor, with the restatement's float32 run as the yardstick; the modes equal the
    float64 run's wherever its decisions have a margin of 2; 3 launches a step, at most 5 with filter_from_wd"""
    m, opt = _model_opt()
    params = list(m.parameters())
    assert len(params) == 161
    p0 = [p.detach().cpu().clone() for p in params]
    r64 = Restated(KW, p0, [0] * 161, [KW["weight_decay"]], torch.float64)
    r32 = Restated(KW, p0, [0] * 161, [KW["weight_decay"]], torch.float32)
    calls = H.count_launches(monkeypatch, STAGES)
    worst = 0.0
    for k, lr in enumerate((1e-3, 2e-3)):
        m.flat_grads.copy_(H.grads_for(m, 41 + k))
        opt.param_groups[0]["lr"] = lr
        opt.zero_grad()
        del calls[:]
        opt.step()
        torch.cuda.synchronize()
        assert calls == ["adamp_unit_sums", "adamp_coef", "adamp_update"]
        grads = [p.grad.detach().cpu().clone() for p in params]
        r64.step(grads, [lr])
        r32.step(grads, [lr])
        modes = [int(x) for x in opt.projection_modes.cpu()]
        assert modes == r64.modes, f"step {k + 1}: modes"
        for i, p in enumerate(params):
            yard = (r32.p[i].double() - r64.p[i]).abs().max().item()
            worst = max(worst, H.within_yardstick(p, r64.p[i], yard, f"step {k + 1} tensor {i} {tuple(p.shape)} mode {modes[i]}", floor_in_ratio=True,
                                                  yard_name="restated fp32"))
    print(f"model scale: worst native error / max(restated-fp32 error, floor) {worst:.2f}; modes 0/1/2: {[modes.count(x) for x in (0, 1, 2)]}")
    mask = H.padding_mask(m)
    assert mask.any() and (m.flat_params[mask] == 0).all() and torch.isnan(m.flat_grads[mask]).all() and torch.isfinite(m.flat_params).all()
    assert all((p.detach().cpu() != q).any() for p, q in zip(params, p0))
    # the recipe's two groups
    sys.path.insert(0, ROOT)
    import train

    m2, opt2 = _model_opt(lambda mm: train.filter_from_weight_decay(mm, ["bn", "bias"]))
    m2.flat_grads.copy_(H.grads_for(m2, 43))
    del calls[:]
    opt2.zero_grad()
    opt2.step()
    torch.cuda.synchronize()
    assert len(calls) <= 5 and calls == ["adamp_unit_sums", "adamp_coef", "adamp_coef", "adamp_update", "adamp_update"]
    assert (m2.flat_params[H.padding_mask(m2)] == 0).all() and torch.isfinite(m2.flat_params).all()
    assert all(opt2.state[p]["step"] == 1 for p in m2.parameters())


def test_model_ema_inside_the_step_kernel_matches_the_callback(dev):
    """ModelEma (train.py:111-112) under AdamP: the average advanced by the update kernel (attach_ema) equals the callback's own lerp after
    every batch within the rule of this file, and the parameters are the same bits either way"""
    e_a, e_b = H.ema_matches_callback(_model_opt, 1e-4)
    # the callback's lerp may fuse ema + w*(p - ema) into one rounding where the kernel makes two: at most one ulp of the average, 2 * 2^-24 of
    # its magnitude, in each of the 3 steps
    assert (e_a - e_b).abs().max().item() <= 3 * 2 * U * e_b.abs().max().item()


# ---- 7. entry points ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch(dev):
    """on real device arrays: every listed bad argument returns MI355_E_ARG (-1), and no array has changed afterwards"""
    from sota_imagenet_amd import native, ops
    from sota_imagenet_amd.item_plan import pack_records

    L, P = native.lib(), ctypes.c_void_p
    n = 64
    p, g, m, v, e = (torch.full((n,), x, device=dev) for x in (1.0, 2.0, 3.0, 4.0, 5.0))
    items, tens, pieces = (pack_records([r], dev) for r in ((0, n, 0), (0, 16, 0), (0, 16, 0)))
    slots = torch.tensor([[0, 1]] * 4, dtype=torch.int32, device=dev)
    decide = torch.tensor([[0, 4, 16, 1]], dtype=torch.int32, device=dev)
    partial = torch.full((4, 4), 6.0, dtype=torch.float64, device=dev)
    coef, wdf, mode = torch.full((4, 2), 7.0, device=dev), torch.full((1,), 8.0, device=dev), torch.full((1,), 9, dtype=torch.int32, device=dev)
    q = lambda t, off=0: P(t.data_ptr() + off)  # noqa: E731
    st = native.cur_stream()
    inf, nan = float("inf"), float("nan")

    def sums(pp=q(p), vv=q(v), pc=q(pieces), pt=q(partial), n_pieces=1, ns=4, b1=0.9, eps=1e-8, step=1, gs=1.0):
        return L.mi355_adamp_unit_sums(pp, q(g), q(m), vv, n, pc, n_pieces, ns, b1, 0.999, eps, step, 0, gs, pt, st)

    def cf(pt=q(partial), sl=q(slots), dc=q(decide), cc=q(coef), ww=q(wdf), mm=q(mode), n_partial=4, ns=4, nt=1, lr=1e-3, wd=1e-2, eps=1e-8,
           delta=0.1, ratio=0.1):
        return L.mi355_adamp_coef(pt, n_partial, sl, ns, dc, nt, cc, ww, mm, lr, wd, eps, delta, ratio, st)

    def update(pp=q(p), vv=q(v), ee=None, it=q(items), tn=q(tens), cc=q(coef), ww=q(wdf), n_items=1, nt=1, ns=4, lr=1e-3, b2=0.999, eps=1e-8,
               step=1, gs=1.0, decay=0.9):
        args = (n, it, n_items, tn, nt, cc, ns, ww, lr, 0.9, b2, eps, step, 0, gs)
        if ee is None:
            return L.mi355_adamp_update(pp, q(g), q(m), vv, *args, st)
        return L.mi355_adamp_update_ema(pp, q(g), q(m), vv, ee, *args, decay, st)

    bad = [sums(pp=None), sums(vv=q(v, 4)), sums(pc=q(pieces, 8)), sums(pt=q(partial, 4)), sums(n_pieces=0), sums(ns=0), sums(b1=1.0),
           sums(eps=-1.0), sums(step=0), sums(gs=nan),
           cf(pt=None), cf(mm=None), cf(sl=q(slots, 4)), cf(dc=q(decide, 8)), cf(cc=q(coef, 4)), cf(ww=q(wdf, 2)), cf(n_partial=0), cf(ns=0),
           cf(nt=0), cf(lr=-1.0), cf(wd=nan), cf(eps=inf), cf(delta=-1.0), cf(delta=nan), cf(ratio=-0.1), cf(ratio=inf),
           update(pp=None), update(cc=None), update(vv=q(v, 4)), update(it=q(items, 8)), update(tn=q(tens, 8)), update(ee=q(e, 4)),
           update(cc=q(coef, 4)), update(n_items=0), update(nt=0), update(ns=0), update(lr=nan), update(b2=1.0), update(eps=-1.0),
           update(step=0), update(gs=inf), update(ee=q(e), decay=1.5),
           L.mi355_adamp_update_ema(q(p), q(g), q(m), q(v), None, n, q(items), 1, q(tens), 1, q(coef), 4, q(wdf), 1e-3, 0.9, 0.999, 1e-8, 1, 0, 1.0,
                                    0.9, st)]
    assert bad == [-1] * len(bad)
    torch.cuda.synchronize()
    for t, x in ((p, 1.0), (g, 2.0), (m, 3.0), (v, 4.0), (e, 5.0), (partial, 6.0), (coef, 7.0), (wdf, 8.0), (mode, 9)):
        assert (t == x).all()
    with pytest.raises(ValueError):  # the wrappers of ops.py check what they are given as well
        ops.adamp_unit_sums(p, g, m, v, pieces, partial[:1, :2], 4, 1)
    with pytest.raises(ValueError):
        ops.adamp_coef(partial, slots, decide, coef[:2], wdf, mode, 1e-3, 1e-2)
    with pytest.raises(ValueError):
        ops.adamp_update(p, g, m, v[:32], items, tens, coef, wdf, 1, 1e-3)
    assert sums() == 0 and cf() == 0 and update() == 0  # and the good calls launch
    torch.cuda.synchronize()
    assert partial[0, 1].item() == 16.0 and mode.item() in (0, 1, 2) and (p != 1.0).all()


# ---- 8. smoke -------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_runs_the_smoke_config(dev, tmp_path, monkeypatch):
    """train.py on adamp_test: the native class is built and stepped, the two epochs' losses are finite and decreasing over the run, and the
    log shows how many tensors took mode 0 / 1 / 2 at the last step (printed, not asserted: which mode a bf16 BatchNorm net's convolutions
    take is not known until it is run)"""
    from sota_imagenet_amd import optim

    made = []
    build = optim.AdamP._build_plans

    def spy(self):
        made.append(self)
        return build(self)

    monkeypatch.setattr(optim.AdamP, "_build_plans", spy)
    _, _, run, losses = H.run_smoke_config("adamp_test", tmp_path, ["run.fp16=false", "random_seed=0", "data.pool=2", "log.save_optim=true"])
    assert made and all(type(o) is optim.AdamP for o in made)
    modes = [int(x) for x in made[-1].projection_modes.cpu()]
    print("adamp_test train losses:", losses, "| tensors in mode 0 / 1 / 2 at the last step:", [modes.count(x) for x in (0, 1, 2)])
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]
    ck = torch.load(os.path.join(run, "model.chpn"), map_location="cpu")
    per_param = list(ck["optimizer"]["state"].values())
    assert len(per_param) == 161 and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and s["step"] > 0 for s in per_param)
