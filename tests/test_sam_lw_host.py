"""SAM (sharpness-aware minimization with per-tensor or per-output-unit norms) on the host: the reference's targets resolve to the native
callback, the smoke config composes, accumulate_steps != 1 is refused, the documented rules — restated in float64 torch (tests/sam_lw_common.py)
— reproduce the trajectories that the reference's own callback recorded in tests/golden/sam_lw_ref_trajectories.npz, the plan over the real
ResNet-50 layout covers every unit once with pieces that stay inside it, and the new C-ABI entries refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from plan_common import resnet50_table
from sam_lw_common import CASES, GN_FLOOR, WN_FLOOR, Fixture, restate_fixture
from sota_imagenet_amd import config as C
from sota_imagenet_amd import native


def test_reference_targets_resolve_to_the_native_callback():
    from sota_imagenet_amd import callbacks, fit_wrapper

    for target in ("src.callbacks.SAM", "sota_imagenet.callbacks.SAM"):
        assert C.resolve_target(target) is callbacks.SAM
        assert C.CALLBACK_TARGET_ALIASES[target] == "sota_imagenet_amd.callbacks.SAM"
        assert target not in C.TARGET_ALIASES and target not in C.LAYERWISE_TARGET_ALIASES
    clb = C.call({"_target_": "src.callbacks.SAM"})
    assert isinstance(clb, fit_wrapper.Callback) and (clb.unitwise, clb.rho, clb.eps, clb.eps_2) == (False, 0.01, 1e-5, 1e-3)
    assert clb.coef is None and clb.norms is None and clb.eps_flat is None and clb.forwards == 0
    clb = C.call({"_target_": "src.callbacks.SAM", "rho": 0, "unitwise": True})  # the recipe file writes rho: 0
    assert (clb.unitwise, clb.rho) == (True, 0)
    for bad in (dict(rho=-1e-3), dict(rho=float("inf")), dict(rho=float("nan"))):
        with pytest.raises(ValueError):
            callbacks.SAM(**bad)


def test_smoke_config_composes_with_the_callback_first():
    from sota_imagenet_amd import callbacks, fit_wrapper, optim

    cfg = C.compose(None, ["+hydra_exp=nov-adam_sam-unit_test"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "src.optimizers.AdamLayerwise" and got == dict(weight_decay=2e-2, betas=[0.9, 0.995], lr=0)
    assert C.to_plain(cfg.run.extra_callbacks) == [{"_target_": "src.callbacks.SAM", "rho": 0.001, "unitwise": True},
                                                   {"_target_": "pytorch_tools.fit_wrapper.callbacks.Callback"}]
    made = [C.call(c) for c in cfg.run.extra_callbacks]
    assert type(made[0]) is callbacks.SAM and (made[0].rho, made[0].unitwise) == (0.001, True) and type(made[1]) is fit_wrapper.Callback
    assert cfg.log.exp_name == "nov-adam_sam-unit_test" and cfg.debug is True and cfg.loader.image_size == 64 and cfg.loader.batch_size == 16
    assert type(C.call(cfg.optim, [{"params": [torch.nn.Parameter(torch.zeros(4))]}])) is optim.AdamLayerwise
    plain, with_sam = C.to_plain(C.compose(None, ["+hydra_exp=nov-adam_test"])), C.to_plain(cfg)
    for d in (plain, with_sam):
        d["run"].pop("extra_callbacks")
        d["log"].pop("exp_name")
    assert plain == with_sam


def test_accumulate_steps_other_than_one_is_refused():
    from sota_imagenet_amd import callbacks, fit_wrapper

    clb = callbacks.SAM(unitwise=True)
    clb.set_state(fit_wrapper.RunnerState(accumulate_steps=2))
    with pytest.raises(NotImplementedError, match="SAM: accumulate_steps"):
        clb.on_begin()
    clb.set_state(fit_wrapper.RunnerState(accumulate_steps=1))
    clb.on_begin()


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference_trajectory(case):
    """gn and wn per slot, eps, the parameters at the second forward and after the optimizer step, every step and tensor, to 1e-12 relative;
    every step is perturbed (two forwards); both floors are hit where the generator put them"""
    fx = Fixture(case)
    got = restate_fixture(fx, torch.float64)
    assert fx.forwards == [2, 2, 2] == [g[5] for g in got] and fx.steps == 3
    assert fx.gn.shape == fx.wn.shape == (3, sum(fx.slot_counts)) and sum(fx.slot_counts) == (6 if case == "layer_sgd" else 97)
    for k in range(fx.steps):
        gn, wn, eps, pert, step, _ = got[k]
        for what, a, b in (("gn", gn, fx.gn[k]), ("wn", wn, fx.wn[k])):
            b = torch.from_numpy(b)
            assert ((a - b).abs() <= 1e-12 * b).all(), (case, what, k)
        assert torch.equal(gn == GN_FLOOR, torch.from_numpy(fx.gn[k] == GN_FLOOR)) and torch.equal(wn == WN_FLOOR, torch.from_numpy(fx.wn[k] == WN_FLOOR))
        for what, a, b in (("eps", eps, fx.eps[k]), ("pert", pert, fx.pert(k)), ("step", step, fx.p_step[k])):
            for i, (x, y) in enumerate(zip(fx.split(a), fx.split(b))):
                rel = ((x - y).abs().max() / y.abs().max().clamp_min(1e-300)).item()
                assert rel <= 1e-12, (case, what, k, i, rel)
        assert all(t.abs().max() > 0 for t in fx.split(fx.eps[k]))  # every tensor is perturbed, the first step included
    s2, s4 = fx.slot_offs[2], fx.slot_offs[4]
    assert (fx.gn[:, s2:fx.slot_offs[3]] == GN_FLOOR).all() and (fx.wn[:, s2:fx.slot_offs[3]] > WN_FLOOR).all()  # tensor 2: gn on its floor
    assert (fx.gn[:, s4] == GN_FLOOR).all() and (fx.wn[:, s4] == WN_FLOOR).all()                                 # tensor 4: both
    if fx.unitwise:
        row = fx.slot_offs[3] + 4
        assert fx.wn[0, row] == WN_FLOOR and fx.gn[0, row] > GN_FLOOR and (fx.wn[0, fx.slot_offs[3]:s4] == WN_FLOOR).sum() == 1
    assert (got[-1][4] - fx.p0.double()).abs().max().item() > 1e-3  # the steps moved the parameters


def _resnet50_tensors(unitwise, base=(1 << 20, 1 << 30)):
    from sota_imagenet_amd.callbacks import SAM

    table, total = resnet50_table()
    sizes = [int(np.prod(shape)) for _, _, shape in table]
    tensors = [(base[0], base[1], off, n, SAM.unit_len(shape, (n // shape[0],) + (1,) * (len(shape) - 1), unitwise))
               for (_, off, shape), n in zip(table, sizes)]
    return table, total, sizes, tensors


@pytest.mark.parametrize("unitwise", [False, True])
def test_plan_covers_every_unit_once_on_the_resnet50_layout(unitwise):
    """161 tensors in one storage pair.  The item table is SAMOriginal's.  Unit-wise: the pieces cover every element of every ndim > 1 tensor
    exactly once and nothing else, no piece crosses a unit or exceeds a work item, a 4608-element row is two pieces; slots = sum of shape[0]
    over the 54 weights + 107; every slot's partial sums are consecutive and every entry belongs to exactly one slot.  Layer-wise: no pieces,
    161 slots."""
    from sota_imagenet_amd.callbacks import SAM, SAMOriginal

    table, total, sizes, tensors = _resnet50_tensors(unitwise)
    W = int(native.lib().mi355_lw_item_elems())
    tab = SAM.plan_tables(tensors, W)
    items0, _, pairs0 = SAMOriginal.plan_tables([(pb, gb, off, n, len(shape)) for (pb, gb, off, n, _), (_, _, shape) in zip(tensors, table)], W)
    assert tab["items"] == items0 and len(tab["pairs"]) == 1 and tab["pairs"][0][:4] == pairs0[0][:4] and tab["pairs"][0][-1] == pairs0[0][-1]
    lo = min(off for _, off, _ in table)
    weights = [t for t, (_, _, shape) in enumerate(table) if len(shape) > 1]
    assert len(weights) == 54
    n_slots = (sum(table[t][2][0] for t in weights) + 107) if unitwise else 161
    assert len(tab["slots"]) == n_slots and (not unitwise or n_slots == 27560 + 107)
    # tensor records: start, unit length, first slot; the slots are numbered tensor by tensor
    nxt = 0
    for t, (start, u, s0) in enumerate(tab["tensors"]):
        shape = table[t][2]
        assert start == table[t][1] - lo and s0 == nxt and u == (sizes[t] // shape[0] if unitwise and len(shape) > 1 else sizes[t])
        nxt += sizes[t] // u
    assert nxt == n_slots
    cover = np.zeros(total, dtype=np.uint8)
    per_slot = {}
    for k, (off, ln, slot) in enumerate(tab["pieces"]):
        assert 1 <= ln <= W
        t = max(i for i in weights if tab["tensors"][i][2] <= slot)  # (slot0 grows with the tensor index)
        start, u, s0 = tab["tensors"][t]
        j = slot - s0
        assert 0 <= j < table[t][2][0] and start + j * u <= off and off + ln <= start + (j + 1) * u  # inside ONE unit
        cover[lo + off: lo + off + ln] += 1
        per_slot.setdefault(slot, []).append(k)
    real = np.zeros(total, dtype=bool)
    for t in (weights if unitwise else []):
        real[table[t][1]: table[t][1] + sizes[t]] = True
    assert (cover[real] == 1).all() and (cover[~real] == 0).all() and bool(tab["pieces"]) == unitwise
    # the whole-tensor items: those of the other tensors, in the order of the item table
    whole_t = [t for t in range(161) if not (unitwise and t in weights)]
    assert tab["whole"] == [it for it in tab["items"] if it[2] in whole_t]
    (_, _, _, _, (pa, pb), (wa, wb), k0, _), = tab["pairs"]
    assert (pa, pb, wa, wb, k0) == (0, len(tab["pieces"]), 0, len(tab["whole"]), 0)
    used = np.zeros(len(tab["pieces"]) + len(tab["whole"]), dtype=np.uint8)
    for slot, (first, count) in enumerate(tab["slots"]):
        assert count >= 1
        used[first:first + count] += 1
        if slot in per_slot:
            assert per_slot[slot] == list(range(first, first + count))
    assert (used == 1).all()
    for t in whole_t:  # a whole-tensor slot's entries are its items, behind the pieces
        first, count = tab["slots"][tab["tensors"][t][2]]
        assert [it[2] for it in tab["whole"][first - pb: first - pb + count]] == [t] * count == [t] * ((sizes[t] + W - 1) // W)
    if unitwise:
        t = next(i for i, (name, _, _) in enumerate(table) if name == "layer4.2.conv2.weight")
        assert tab["tensors"][t][1] == 4608 and tab["slots"][tab["tensors"][t][2]][1] == 2
        first = tab["slots"][tab["tensors"][t][2] + 1][0]
        assert [p[1] for p in tab["pieces"][first:first + 2]] == [W, 4608 - W]
        stem = next(i for i, (name, _, _) in enumerate(table) if name == "conv1.weight")
        assert tab["tensors"][stem][1] == 147 and any(p[0] % 4 for p in tab["pieces"] if p[2] in range(tab["tensors"][stem][2], tab["tensors"][stem][2] + 64))


def test_fixture_tensors_in_storages_of_their_own():
    """each of the fixture's six tensors in its own parameter / gradient storage: one launch set per tensor, offsets counted from its own start,
    the partial sums of the pairs back to back; row 36 of [37, 113] straddles the item boundary at 4096"""
    from sota_imagenet_amd.callbacks import SAM

    fx = Fixture("unit_sgd")
    W = int(native.lib().mi355_lw_item_elems())
    order = [i for idx in fx.groups for i in idx]
    tensors = [(4096 * (i + 1), 1 << 30 | 4096 * (i + 1), 0, fx.sizes[i], fx.sizes[i] // fx.shapes[i][0] if len(fx.shapes[i]) > 1 else fx.sizes[i])
               for i in order]
    tab = SAM.plan_tables(tensors, W)
    assert len(tab["pairs"]) == 6 and len(tab["slots"]) == 16 + 32 + 10 + 37 + 2 and len(tab["items"]) == 7
    k = 0
    for j, (lo, hi, i0, i1, (pa, pb), (wa, wb), k0, ts) in enumerate(tab["pairs"]):
        shape = fx.shapes[order[j]]
        assert (lo, hi, ts, k0) == (0, fx.sizes[order[j]], [j], k)
        assert (pb - pa, wb - wa) == ((shape[0], 0) if len(shape) > 1 else (0, 1))
        k += pb - pa + wb - wa
    assert [(o, ln) for o, ln, t in tab["items"] if t == 3] == [(0, 4096), (4096, 85)] and 36 * 113 < 4096 < 37 * 113


def test_a_parameter_whose_dim_0_is_not_outermost_is_refused():
    from sota_imagenet_amd.callbacks import SAM

    w = torch.zeros(6, 4).t()  # shape [4, 6], strides (1, 4): dense, but a row is not a contiguous run
    with pytest.raises(RuntimeError, match="outermost"):
        SAM.unit_len(w.shape, w.stride(), True)
    assert SAM.unit_len(w.shape, w.stride(), False) == 24
    krsc = torch.zeros(8, 3, 3, 5).permute(0, 3, 1, 2)  # an OIHW view over KRSC memory, as the flat models hold their conv weights
    assert SAM.unit_len(krsc.shape, krsc.stride(), True) == 45
    assert SAM.unit_len((7,), (1,), True) == 7 and SAM.unit_len((1, 9), (1, 1), True) == 9
    with pytest.raises(ValueError, match="whole number of units"):
        SAM.plan_tables([(0, 1 << 20, 0, 10, 3)], 4096)


P = ctypes.c_void_p


def test_bad_arguments_return_status_not_crash():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    A = 4096
    E = -1  # MI355_E_ARG
    inf, nan = float("inf"), float("nan")

    def sumsq(p=A, g=A, items=A, partial=A, n_items=1, nt=1, gs=1.0):
        return L.mi355_sam_lw_sumsq(P(p), P(g), 64, P(items), n_items, nt, gs, P(partial), None)

    assert sumsq(p=0) == E and "null" in native.last_error()
    assert sumsq(g=0) == E and "null" in native.last_error()
    assert sumsq(items=0) == E and "null" in native.last_error()
    assert sumsq(partial=0) == E and "null" in native.last_error()
    assert sumsq(g=A + 4) == E and "aligned" in native.last_error()
    assert sumsq(items=A + 8) == E and "aligned" in native.last_error()
    assert sumsq(partial=A + 8) == E and "aligned" in native.last_error()
    assert sumsq(n_items=0) == E and "n_items" in native.last_error()
    assert sumsq(nt=0) == E and "n_tensors" in native.last_error()
    assert sumsq(gs=inf) == E and "grad_scale" in native.last_error()
    assert sumsq(gs=nan) == E and "grad_scale" in native.last_error()

    def unit(p=A, g=A, pieces=A, partial=A, n_pieces=1, ns=1, gs=1.0, tpp=64):
        return L.mi355_sam_unit_sumsq(P(p), P(g), 64, P(pieces), n_pieces, ns, gs, P(partial), tpp, None)

    assert unit(p=0) == E and "null" in native.last_error()
    assert unit(pieces=0) == E and "null" in native.last_error()
    assert unit(partial=0) == E and "null" in native.last_error()
    assert unit(p=A + 4) == E and "aligned" in native.last_error()
    assert unit(pieces=A + 8) == E and "aligned" in native.last_error()
    assert unit(partial=A + 8) == E and "aligned" in native.last_error()
    assert unit(n_pieces=0) == E and "n_pieces" in native.last_error()
    assert unit(ns=0) == E and "n_slots" in native.last_error()
    assert unit(gs=nan) == E and "grad_scale" in native.last_error()
    for tpp in (0, 32, 128, 512):
        assert unit(tpp=tpp) == E and "threads_per_piece" in native.last_error()

    def coef(partial=A, n=1, slots=A, ns=1, c=A, norms=A):
        return L.mi355_sam_lw_coef(P(partial), n, P(slots), ns, P(c), P(norms), None)

    assert coef(partial=0) == E and "null" in native.last_error()
    assert coef(slots=0) == E and "null" in native.last_error()
    assert coef(c=0) == E and "null" in native.last_error()
    assert coef(norms=0) == E and "null" in native.last_error()
    assert coef(partial=A + 8) == E and "aligned" in native.last_error()
    assert coef(slots=A + 4) == E and "aligned" in native.last_error()
    assert coef(c=A + 2) == E and "aligned" in native.last_error()
    assert coef(norms=A + 4) == E and "aligned" in native.last_error()
    assert coef(n=0) == E and "n_partial" in native.last_error()
    assert coef(ns=0) == E and "n_slots" in native.last_error()

    def perturb(p=A, g=A, eps=A, items=A, tensors=A, c=A, n_items=1, nt=1, ns=1, rho=0.01, gs=1.0):
        return L.mi355_sam_lw_perturb(P(p), P(g), P(eps), 64, P(items), n_items, P(tensors), nt, P(c), ns, rho, gs, None)

    assert perturb(eps=0) == E and "null" in native.last_error()
    assert perturb(tensors=0) == E and "null" in native.last_error()
    assert perturb(c=0) == E and "null" in native.last_error()
    assert perturb(p=A + 8) == E and "aligned" in native.last_error()
    assert perturb(eps=A + 4) == E and "aligned" in native.last_error()
    assert perturb(tensors=A + 8) == E and "aligned" in native.last_error()
    assert perturb(c=A + 2) == E and "aligned" in native.last_error()
    assert perturb(n_items=0) == E and "n_items" in native.last_error()
    assert perturb(nt=0) == E and "n_tensors" in native.last_error()
    assert perturb(ns=0) == E and "n_slots" in native.last_error()
    assert perturb(rho=-0.01) == E and "rho" in native.last_error()
    assert perturb(rho=nan) == E and "rho" in native.last_error()
    assert perturb(rho=inf) == E and "rho" in native.last_error()
    assert perturb(gs=nan) == E and "grad_scale" in native.last_error()
