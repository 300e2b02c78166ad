"""Native MyNovograd / NovogradApex with unitwise_norm=True (csrc/optim_lw.hip, optim._Layerwise) on the MI355X against trajectories recorded
from the reference's own classes (tests/golden/layerwise_unit_ref_trajectories.npz, written by tests/golden/make_layerwise_unit_golden.py on
the CPU).

Yardstick, stored in the fixture and never computed from the code under test: the rule of this family (tests/optim_harness.py, within_yardstick:
1.5 times the reference's own float32 error plus a floor of 4 * 2^-24 of the largest parameter magnitude).  At model scale the same rule
with the float32 run of the restated rule (tests/layerwise_unit_common.py) as the yardstick.  The update kernel alone is compared bit for bit
with the float32 restatement that is handed the native denominators."""
import copy
import ctypes
import math
import os
import sys

import pytest
import torch

import optim_harness as H
from layerwise_unit_common import CASES, UnitFixture, UnitRestated, slot_rows
from optim_harness import U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(fx, dev, grad_scale=1.0, steps=6, separate=False):
    ps, groups, fp, fg, offs = H.fixture_problem(fx, dev, separate=separate)
    opt = H.make_opt(fx, groups, fx.lrs[0])
    opt.grad_scale = grad_scale
    traj = []
    for k in range(steps):
        for g in opt.param_groups:
            g["lr"] = fx.lrs[k]
        H.set_grads(ps, fx.split(fx.grads[k]), 1.0 / grad_scale)  # (exact: a power of two)
        opt.step()
        traj.append(H.gather(ps).clone())
    torch.cuda.synchronize()
    return traj, opt, ps, fp, fg


# ---- 1. trajectories --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_steps_follow_the_reference_trajectory(dev, case):
    """six steps on the fixture's inputs, gradients and lr ramp, every step and tensor against the stored yardstick; the same again with
    grad_scale = 0.5 on doubled gradients.  The gaps of the flat buffers are never touched: zero in p, NaN in g.  The second moment after
    step 5, taken through state_dict(), equals the fixture's float64 state to 4 * 2^-24 relative."""
    fx = UnitFixture(case)
    worst = 0.0
    for gs in (1.0, 0.5):
        traj, opt, ps, fp, fg = _run(fx, dev, grad_scale=gs)
        for k, got in enumerate(traj):
            worst = max(worst, fx.check(k, got, f"{case} grad_scale={gs}"))
        gaps = H.gaps(ps, fp)
        assert gaps.any() and (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all() and torch.isfinite(fp).all()
        assert all(opt.state[p]["step"] == 6 and type(opt.state[p]["step"]) is int for p in ps)
    print(f"{case}: worst native / reference-fp32 error ratio {worst:.2f}")
    assert (traj[-1].cpu() - fx.p0).abs().max().item() > 1e-3
    _, opt5, ps5, _, _ = _run(fx, dev, steps=5)
    sd = opt5.state_dict()
    order = [i for idx in fx.groups for i in idx]
    want = fx.split(fx.state5[fx.v_key])
    for j, i in enumerate(order):
        got = sd["state"][j][fx.v_key].cpu().reshape(-1)
        rel = ((got.double() - want[i].double()).abs() / want[i].double().abs()).max().item()
        print(f"{case} tensor {i}: second moment after step 5, worst relative distance {rel:.3e}")
        assert rel <= 4 * U


# ---- the tensors of tests 2 to 4 --------------------------------------------------------------------------------------------------------------
def _small_shapes():
    from sota_imagenet_amd import ops

    W = ops.lw_item_elems()
    return W, [(64, 3, 7, 7), (2, 2 * W + 808), (7, 1), (5, 3), (1, 33), (3, 4), (W + 1,), (5,), (1,)]


def _small_problem(dev, separate=False, seed=11):
    W, shapes = _small_shapes()
    sizes = [math.prod(s) for s in shapes]
    gen = torch.Generator().manual_seed(seed)
    vals = [(torch.randn(s, generator=gen) * (10.0 ** (i % 3 - 1))).view(shape) for i, (s, shape) in enumerate(zip(sizes, shapes))]
    grads = [[(torch.randn(s, generator=gen) * (10.0 ** ((i + k) % 3 - 2))).view(shape) for i, (s, shape) in enumerate(zip(sizes, shapes))]
             for k in range(2)]
    ps, fp, fg, offs = H.flat_params(sizes, shapes, vals, dev, separate=separate)
    return W, shapes, vals, grads, ps, fp, fg


def _per_slot(opt, t):
    """a per-slot device array of the optimizer, split per planned tensor"""
    return [t[s0:s0 + cnt].clone() for s0, cnt in opt.slot_ranges]


# ---- 2. per-slot sums -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["gradient", "parameter"])
def test_per_slot_sums_equal_the_float64_sums(dev, source):
    """147-long units at every alignment with items spanning dozens of units; a unit of three pieces with items inside one unit and one across
    the boundary; f32x4 covering several units ([7,1], [5,3]); shape[0] == 1; whole vectors; 1-D tensors of W + 1, 5 and 1 elements — in one
    flat buffer with NaN in every gap of the gradient: S of every slot equals the float64 sum of squares to 1e-12 relative, for the gradient
    (NovogradApex, grad_scale 0.5) and the parameter (MyNovograd) as source"""
    from sota_imagenet_amd import optim

    W, shapes, vals, grads, ps, fp, fg = _small_problem(dev)
    H.set_grads(ps, grads[0])
    if source == "gradient":
        opt, scale, src = optim.NovogradApex(ps, lr=1e-3, betas=(0.9, 0.99), unitwise_norm=True), 0.5, grads[0]
    else:
        opt, scale, src = optim.MyNovograd(ps, lr=1e-3, unitwise_norm=True), 1.0, vals
    opt.grad_scale = 0.5
    opt.step()
    torch.cuda.synchronize()
    assert [c for _, c in opt.slot_ranges] == [64, 2, 7, 5, 1, 3, 1, 1, 1] and opt._sums.numel() == 85
    got = opt._sums.cpu()
    want = torch.cat([slot_rows((t * scale).double()).pow(2).sum(1) for t in src])
    rel = ((got - want).abs() / want).max().item()
    print(f"{source}: per-slot sums, worst relative error {rel:.3e}; pieces {opt._pieces.shape[0]}, whole items {opt._whole.shape[0]}")
    assert rel <= 1e-12
    assert opt._pieces.shape[0] == 85 and opt._whole.shape[0] == 5 and opt._partial.numel() == 90
    for t in (opt._sums, opt._partial, opt._den, opt._v, fp, *[opt.state[p][opt._m_key] for p in ps]):
        assert torch.isfinite(t).all()
    gaps = H.gaps(ps, fp)
    assert (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all()
    assert all((p.detach().cpu() != v).any() for p, v in zip(ps, vals))  # every tensor was updated
    # the second moment follows the NORM, sqrt(S), from ema_norm_init, and the views show one value per slot in the parameter's shape
    b2 = 0.99
    v = (1e-3 * b2 + (1 - b2) * want.sqrt()).float()
    assert ((opt._v.cpu() - v).abs() <= 2 * U * v).all()
    for p, (s0, cnt) in zip(ps, opt.slot_ranges):
        sv = opt.state[p][opt._v_key]
        assert sv.shape == p.shape and sv.stride() == (((1,) + (0,) * (p.dim() - 1)) if p.dim() > 1 else (0,))
        assert torch.equal(slot_rows(sv)[:, 0], opt._v[s0:s0 + cnt])


# ---- 3. the update kernel, element by element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("cls,wd_eps", [("NovogradApex", None), ("NovogradApex", 0.01), ("MyNovograd", None)])
def test_update_equals_the_float32_restatement_bit_for_bit(dev, cls, wd_eps, ema):
    """two steps on the tensors of the sums test (the second with a non-zero first moment), grad_scale 0.5: the float32 restatement, handed
    the native denominators of each step (they differ unit by unit), gives the native parameters, first moments and moving average bit for
    bit — rules 0 and 1, wd_eps on and off, with and without the average"""
    from sota_imagenet_amd import optim

    W, shapes, vals, grads, ps, fp, fg = _small_problem(dev, seed=12)
    kw = dict(betas=(0.9, 0.99), weight_decay=0.02, unitwise_norm=True)
    if wd_eps is not None:
        kw["wd_eps"] = wd_eps
    opt = getattr(optim, cls)(ps, lr=1e-2, **kw)
    opt.grad_scale = 0.5
    r = UnitRestated(cls, kw, vals, [0] * len(vals), [0.02], torch.float32, native=True)
    decay = 0.9 if ema else None
    if ema:
        fe = fp.clone()
        opt.attach_ema(fp, fe, decay)
        r.ema = [v.clone() for v in vals]
    for k, lr in enumerate((1e-2, 3e-2)):
        opt.param_groups[0]["lr"] = lr
        H.set_grads(ps, grads[k])
        opt.step()
        torch.cuda.synchronize()
        den = _per_slot(opt, opt._den)
        assert all(len(torch.unique(d)) == d.numel() for d in den[:4])  # one denominator per unit, all different
        r.step(grads[k], [lr], den=den, grad_scale=0.5, ema_decay=decay)
        for i, p in enumerate(ps):
            assert torch.equal(p.detach().cpu(), r.p[i]), f"{cls} step {k + 1} tensor {i} {tuple(p.shape)}: parameters"
            assert torch.equal(opt.state[p][opt._m_key].cpu(), r.m[i]), f"{cls} step {k + 1} tensor {i} {tuple(p.shape)}: first moment"
            if ema:
                o = (p.data_ptr() - fp.data_ptr()) // 4
                assert torch.equal(fe[o:o + p.numel()].cpu().view(p.shape), r.ema[i]), f"{cls} step {k + 1} tensor {i}: moving average"
    gaps = H.gaps(ps, fp)
    assert (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all()
    if ema:
        assert (fe[gaps] == 0).all()


# ---- 4. placement and replay ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["NovogradApex", "MyNovograd"])
def test_placement_and_replay_are_bitwise(dev, cls):
    """the same tensors in separately allocated storages (one launch set per storage pair) give the parameters of the flat-buffer run bit for
    bit, and a second flat-buffer run repeats them bit for bit"""
    from sota_imagenet_amd import optim

    def run(separate):
        W, shapes, vals, grads, ps, fp, fg = _small_problem(dev, separate=separate, seed=13)
        opt = getattr(optim, cls)(ps, lr=1e-2, betas=(0.9, 0.99), weight_decay=0.02, unitwise_norm=True)
        out = []
        for k in range(2):
            H.set_grads(ps, grads[k])
            opt.step()
            out.append(H.gather(ps).clone())
        torch.cuda.synchronize()
        return out, opt

    a, opt_a = run(False)
    b, _ = run(False)
    s, opt_s = run(True)
    assert len(opt_a._segs) == 1 and len(opt_s._segs) == 9
    for k in range(2):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], s[k])
    assert torch.equal(opt_a._v, opt_s._v) and torch.equal(opt_a._sums, opt_s._sums)


# ---- 5. one step at model scale ---------------------------------------------------------------------------------------------------------------
KINDS = {
    "nov_unit": ("NovogradApex", dict(betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01, unitwise_norm=True), 1e-2),
    "mynov_unit": ("MyNovograd", dict(betas=(0.9, 0.99), weight_decay=0.0002, unitwise_norm=True), 1e-2),
}


def _model_opt(kind, groups_of=None):
    return H.model_opt(*KINDS[kind], groups_of)


STAGES = ["lw_sumsq", "lw_coef", "lw_update", "lw_unit_sumsq", "lw_unit_coef", "lw_unit_update"]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_step_at_model_scale(dev, monkeypatch, kind):
    """one step on a real resnet50 flat array (161 tensors, 27,667 slots, alignment gaps, FC padding; NaN in the gradient's padding) against
    the float64 restatement on the CPU, tensor by tensor, with the restatement's own float32 run as the yardstick; 4 launches, 1 + 1 + 2 + 2
    with filter_from_wd; every tensor moved and the parameter padding stays zero"""
    cls, kw, lr = KINDS[kind]
    m, opt = _model_opt(kind)
    params = list(m.parameters())
    assert len(params) == 161
    p0 = [p.detach().cpu().clone() for p in params]
    calls = H.count_launches(monkeypatch, STAGES)
    H.flat_steps(m, opt, [31], lr)
    assert calls == ["lw_unit_sumsq", "lw_sumsq", "lw_unit_coef", "lw_unit_update"]
    assert opt._den.numel() == 27667 and opt._whole.shape[0] == 107
    mask = H.padding_mask(m)
    assert mask.any() and (m.flat_params[mask] == 0).all() and torch.isnan(m.flat_grads[mask]).all() and torch.isfinite(m.flat_params).all()
    grads = [p.grad.detach().cpu().clone() for p in params]
    wd = kw["weight_decay"]
    r64 = UnitRestated(cls, kw, p0, [0] * 161, [wd], torch.float64)
    r32 = UnitRestated(cls, kw, p0, [0] * 161, [wd], torch.float32)
    r64.step(grads, [lr])
    r32.step(grads, [lr])
    worst, moved = 0.0, 0
    for i, p in enumerate(params):
        yard = (r32.p[i].double() - r64.p[i]).abs().max().item()
        worst = max(worst, H.within_yardstick(p, r64.p[i], yard, f"{kind} tensor {i} {tuple(p.shape)}", floor_in_ratio=True, yard_name="restated fp32"))
        moved += int((p.detach().cpu() != p0[i]).any())
    print(f"{kind}: worst native error / max(restated-fp32 error, floor) over 161 tensors {worst:.2f}")
    assert moved == 161
    # the recipe's two groups
    sys.path.insert(0, ROOT)
    import train

    m2, opt2 = _model_opt(kind, lambda mm: train.filter_from_weight_decay(mm, ["bn", "bias"]))
    del calls[:]
    H.flat_steps(m2, opt2, [32], lr)
    assert calls == ["lw_unit_sumsq", "lw_sumsq", "lw_unit_coef", "lw_unit_coef", "lw_unit_update", "lw_unit_update"]
    assert (m2.flat_params[H.padding_mask(m2)] == 0).all() and torch.isfinite(m2.flat_params).all()
    assert all(opt2.state[p]["step"] == 1 for p in m2.parameters())


# ---- 6. resume and state layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_state_layout_resume_and_the_load_tolerance(dev, case):
    """state_dict() carries the reference's keys and dense shapes (recorded in the fixture); loading it into a fresh optimizer continues bit
    for bit; the reference's float64 state after five steps loads and the sixth step lands on the reference's; a dense state with one-ulp
    jitter inside units loads, a spread beyond 2^-23 / (1 - beta2) is refused, and a layer-wise state (one value per tensor) loads"""
    fx = UnitFixture(case)
    order = [i for idx in fx.groups for i in idx]  # state_dict index -> fixture tensor
    traj, opt, ps, _, _ = _run(fx, dev, steps=3)
    sd = copy.deepcopy(opt.state_dict())
    assert sorted(sd["state"]) == list(range(len(order)))
    for j, i in enumerate(order):
        st = sd["state"][j]
        assert sorted(st) == fx.state_keys and st["step"] == 3
        for key, shapes in fx.state_shapes.items():
            assert list(st[key].shape) == shapes[i] and st[key].dtype == torch.float32 and st[key].is_contiguous()
        rows = slot_rows(st[fx.v_key])
        assert (rows == rows[:, :1]).all()  # dense, one value per unit
        sv = opt.state[ps[i]][fx.v_key]
        assert sv.stride() == (((1,) + (0,) * (sv.dim() - 1)) if sv.dim() > 1 else (0,))
    assert len(torch.unique(slot_rows(sd["state"][0][fx.v_key])[:, 0])) == 16

    def three_more(o, pp):
        for k in range(3, 6):
            for g in o.param_groups:
                g["lr"] = fx.lrs[k]
            H.set_grads(pp, fx.split(fx.grads[k]))
            o.step()
        torch.cuda.synchronize()
        return H.gather(pp).clone()

    want = three_more(opt, ps)
    ps2, groups2, _, _, _ = H.fixture_problem(fx, dev, p_flat0=traj[2].cpu())
    opt2 = H.make_opt(fx, groups2, fx.lrs[3])
    opt2.load_state_dict(copy.deepcopy(sd))
    assert torch.equal(three_more(opt2, ps2), want) and all(opt2.state[p]["step"] == 6 for p in ps2)
    ps3, groups3, _, _, _ = H.fixture_problem(fx, dev, p_flat0=traj[2].cpu())  # without the state the steps differ
    assert not torch.equal(three_more(H.make_opt(fx, groups3, fx.lrs[3]), ps3), want)

    # the reference's own state after five steps
    def from_reference(mutate=None):
        ps4, groups4, _, _, _ = H.fixture_problem(fx, dev, p_flat0=fx.p64[4].float())
        opt4 = H.make_opt(fx, groups4, fx.lrs[5])
        state = {}
        for j, i in enumerate(order):
            state[j] = {key: fx.split(t)[i].view(fx.shapes[i]).clone() for key, t in fx.state5.items()}
            state[j]["step"] = 5
        if mutate:
            mutate(state)
        pg = copy.deepcopy(opt4.state_dict()["param_groups"])
        opt4.load_state_dict({"state": state, "param_groups": pg})
        for g in opt4.param_groups:
            g["lr"] = fx.lrs[5]
        H.set_grads(ps4, fx.split(fx.grads[5]))
        opt4.step()
        torch.cuda.synchronize()
        return H.gather(ps4), opt4, ps4

    got, opt4, ps4 = from_reference()
    fx.check(5, got, f"{case} step 6 from the reference's state")
    assert all(opt4.state[p]["step"] == 6 for p in ps4)

    def jitter(state):  # one ulp up on every other element behind the first of each unit: what the reference's float32 run shows
        for st in state.values():
            rows = slot_rows(st[fx.v_key])
            rows[:, 1::2] = torch.nextafter(rows[:, 1::2], torch.full_like(rows[:, 1::2], math.inf))

    got_j, _, _ = from_reference(jitter)
    assert torch.equal(got_j, got)  # the first element of every unit is kept

    def too_wide(state):
        rows = slot_rows(state[0][fx.v_key])
        rows[3, -1] *= 1 + 4 * 2.0 ** -23 / (1 - fx.hyper["betas"][1])

    with pytest.raises(ValueError, match="one value per unit"):
        from_reference(too_wide)

    def layerwise(state):  # one value per tensor, as the layer-wise classes keep it
        for st in state.values():
            st[fx.v_key] = torch.full_like(st[fx.v_key], 0.25)

    _, opt_l, ps_l = from_reference(layerwise)
    assert (opt_l._v != 0.25).all() and all(opt_l.state[p]["step"] == 6 for p in ps_l)


# ---- 7. moving average ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_model_ema_inside_the_step_kernel_matches_the_callback(dev, kind):
    """ModelEma (train.py:111-112) under the unit-wise optimizers: the average advanced by the update kernel (attach_ema) equals the
    callback's own lerp after every batch, and the parameters are the same bits either way"""
    H.ema_matches_callback(lambda: _model_opt(kind), KINDS[kind][2] * 0.1)


# ---- 8. entry points --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch(dev):
    """on real device arrays: every listed bad argument returns MI355_E_ARG (-1), and no array has changed afterwards"""
    from sota_imagenet_amd import native, ops
    from sota_imagenet_amd.item_plan import pack_records

    L, P = native.lib(), ctypes.c_void_p
    n = 64
    p, g, m, e = (torch.full((n,), x, device=dev) for x in (1.0, 2.0, 3.0, 4.0))
    items, tens, pieces = (pack_records([r], dev) for r in ((0, n, 0), (0, 16, 0), (0, 16, 0)))
    slots = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
    partial, sums = torch.full((4,), 5.0, dtype=torch.float64, device=dev), torch.full((4,), 6.0, dtype=torch.float64, device=dev)
    v, den = torch.full((4,), 7.0, device=dev), torch.full((4,), 8.0, device=dev)
    q = lambda t, off=0: P(t.data_ptr() + off)  # noqa: E731
    st = native.cur_stream()
    inf, nan = float("inf"), float("nan")

    def sumsq(src=q(p), pc=q(pieces), pt=q(partial), n_pieces=1, ns=4, scale=1.0):
        return L.mi355_lw_unit_sumsq(src, n, pc, n_pieces, ns, scale, pt, st)

    def coef(pt=q(partial), sl=q(slots), vv=q(v), dd=q(den), ss=q(sums), n_partial=4, ns=1, b2=0.99, eps=1e-8):
        return L.mi355_lw_unit_coef(pt, n_partial, sl, ns, vv, dd, ss, b2, eps, st)

    def update(rule=0, pp=q(p), gg=q(g), mm=q(m), ee=None, it=q(items), tn=q(tens), dd=q(den), n_items=1, nt=1, ns=4, b1=0.9, lr=1e-3, wd=0.0,
               soft=0, wd_eps=0.0, gs=1.0, decay=0.9):
        args = (n, it, n_items, tn, nt, dd, ns, b1, lr, wd, soft, wd_eps, gs)
        if ee is None:
            return L.mi355_lw_unit_update(rule, pp, gg, mm, *args, st)
        return L.mi355_lw_unit_update_ema(rule, pp, gg, mm, ee, *args, decay, st)

    bad = [sumsq(src=None), sumsq(src=q(p, 4)), sumsq(pc=q(pieces, 8)), sumsq(pt=q(partial, 4)), sumsq(n_pieces=0), sumsq(ns=0), sumsq(scale=nan),
           coef(pt=None), coef(vv=None), coef(sl=q(slots, 4)), coef(ss=q(sums, 4)), coef(dd=q(den, 2)), coef(ns=0), coef(n_partial=0),
           coef(b2=1.0), coef(b2=-0.1), coef(eps=-1.0), coef(eps=inf),
           update(pp=None), update(dd=None), update(gg=q(g, 4)), update(it=q(items, 8)), update(tn=q(tens, 8)), update(ee=q(e, 4)),
           update(rule=2), update(rule=-1), update(n_items=0), update(nt=0), update(ns=0), update(b1=1.0), update(b1=-0.5), update(lr=-1.0),
           update(lr=nan), update(wd=inf), update(rule=1, soft=1), update(soft=1, wd_eps=nan), update(gs=inf), update(ee=q(e), decay=1.5),
           L.mi355_lw_unit_update_ema(0, q(p), q(g), q(m), None, n, q(items), 1, q(tens), 1, q(den), 4, 0.9, 1e-3, 0.0, 0, 0.0, 1.0, 0.9, st)]
    assert bad == [-1] * len(bad)
    torch.cuda.synchronize()
    for t, x in ((p, 1.0), (g, 2.0), (m, 3.0), (e, 4.0), (partial, 5.0), (sums, 6.0), (v, 7.0), (den, 8.0)):
        assert (t == x).all()
    # the wrappers of ops.py check what they are given as well
    with pytest.raises(ValueError):
        ops.lw_unit_coef(partial, slots, v[:2], den[:1], sums[:1], 0.99, 1e-8)
    with pytest.raises(ValueError):
        ops.lw_unit_sumsq(p, pieces, partial[:2], 4)
    assert sumsq() == 0 and coef() == 0 and update() == 0  # and the good calls launch
    torch.cuda.synchronize()
    assert abs(partial[0].item() - 16.0) < 1e-12 and sums[0].item() == partial[0].item() and (p[:n] != 1.0).all()


# ---- 9. smoke -----------------------------------------------------------------------------------------------------------------------------------
def test_train_py_runs_the_smoke_config(dev, tmp_path, monkeypatch):
    """train.py on my-nov-unit_test: the native class is built with unitwise_norm and planned, the losses are finite, the checkpoint carries
    the reference's state layout and evaluates after a resume"""
    from sota_imagenet_amd import optim

    name, cls, keys = "my-nov-unit_test", optim.MyNovograd, {"step", "ema_grad", "ema_norm"}
    made = []
    build = cls._build_unit_plans

    def spy(self, entries):
        made.append(self)
        return build(self, entries)

    monkeypatch.setattr(cls, "_build_unit_plans", spy)
    _, _, run, losses = H.run_smoke_config(name, tmp_path, ["run.fp16=false", "random_seed=0", "data.pool=2", "log.save_optim=true"],
                                           resume_eval=True)
    assert made and all(type(o) is cls and o.unitwise_norm is True for o in made)
    print(name, "train losses:", losses)
    assert losses and all(math.isfinite(x) for x in losses)
    ck = torch.load(os.path.join(run, "model.chpn"), map_location="cpu")
    per_param = list(ck["optimizer"]["state"].values())
    assert len(per_param) == 161 and all(set(s) == keys and s["step"] > 0 for s in per_param)
    assert all(s["ema_norm"].shape == s["ema_grad"].shape and s["ema_norm"].is_contiguous() for s in per_param)
