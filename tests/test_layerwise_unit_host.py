"""unitwise_norm=True of MyNovograd / NovogradApex on the host: the unit-wise plan (item_plan.plan_units under optim._Layerwise.plan_unit_tables)
covers every parameter element exactly once on hand-made layouts and on the ResNet-50 layout, its slots are consecutive group by group; the
fixture recorded from the reference's own classes is consistent with the rule as this project documents it; recipe 48's optim node resolves,
the two new config files carry its values, and the C-ABI prototypes parse and refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import layerwise_common
from layerwise_unit_common import CASES, UnitFixture, restate_fixture, slot_rows
from plan_common import resnet50_table
from sota_imagenet_amd import config as C
from sota_imagenet_amd import native
from sota_imagenet_amd.item_plan import plan_units, unit_len

W = 4096
PB, GB = 1 << 20, 1 << 30


def _tensors(layout, group_of=None):
    """layout: [(offset, shape)] -> plan_unit_tables' input, all in one storage pair"""
    out = []
    for i, (off, shape) in enumerate(layout):
        n = int(np.prod(shape))
        u = unit_len(shape, (n // shape[0],) + (1,) * (len(shape) - 1), True, "test")
        out.append((PB, GB, off, n, group_of[i] if group_of else 0, u))
    return out


def _check_cover(tab, tensors, total):
    """every element of every tensor lies in exactly one piece or whole item and in exactly one work item; nothing else is covered; every
    piece lies in one unit and carries that unit's slot; a slot's partial entries are consecutive and are its own"""
    pieces, whole, slots, items = tab["pieces"], tab["whole"], tab["slots"], tab["items"]
    cover, icover = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
    owner = [None] * (len(pieces) + len(whole))  # partial entry -> slot
    lo = min(t[2] for t in tensors)
    assert len(tab["pairs"]) == 1 and tab["pairs"][0][6] == 0
    for k, (off, ln, slot) in enumerate(pieces):
        t = max(i for i, r in enumerate(tab["tensors"]) if r[2] <= slot)
        start, u, s0 = tab["tensors"][t]
        assert 1 <= ln <= W and u < tensors[t][3]
        j = slot - s0
        assert start + j * u <= off and off + ln <= start + (j + 1) * u  # inside ONE unit
        cover[lo + off: lo + off + ln] += 1
        owner[k] = slot
    for k, (off, ln, t) in enumerate(whole):
        start, u, s0 = tab["tensors"][t]
        assert u == tensors[t][3] and start <= off and off + ln <= start + u and off % 4 == 0
        cover[lo + off: lo + off + ln] += 1
        owner[len(pieces) + k] = s0
    for off, ln, t in items:
        icover[lo + off: lo + off + ln] += 1
    real = np.zeros(total, dtype=bool)
    for _, _, off, n, *_ in tensors:
        real[off: off + n] = True
    assert (cover[real] == 1).all() and (cover[~real] == 0).all() and (icover == cover).all()
    assert sorted(s for s in owner) == sorted(s for s, (first, count) in enumerate(slots) for _ in range(count))
    for s, (first, count) in enumerate(slots):
        assert count >= 1 and owner[first: first + count] == [s] * count
    assert len(slots) == sum(t[3] // t[5] for t in tensors)


def test_plan_on_hand_made_layouts():
    from sota_imagenet_amd.optim import _Layerwise

    layout = [(0, (64, 3, 7, 7)), (9408, (2, 2 * W + 808)), (9408 + 4 * W + 1616, (7, 1)), (27424, (5, 3)), (27456, (1, 33)), (27520, (3, 4)),
              (27584, (W + 1,)), (27584 + W + 64, (5,)), (27584 + W + 128, (1,))]
    tensors = _tensors(layout, [0, 0, 0, 0, 0, 0, 1, 1, 1])
    total = 27584 + W + 192
    tab = _Layerwise.plan_unit_tables(tensors, W)
    _check_cover(tab, tensors, total)
    assert [r[1] for r in tab["tensors"]] == [147, 2 * W + 808, 1, 3, 33, 4, W + 1, 5, 1]
    assert [r[2] for r in tab["tensors"]] == [0, 64, 66, 73, 78, 79, 82, 83, 84] and len(tab["slots"]) == 85
    # a unit of three pieces, cut at multiples of W from the unit's start; the 1-D tensor of W + 1 elements is two whole items
    assert tab["slots"][64] == (64, 3) and [p[1] for p in tab["pieces"][64:67]] == [W, W, 808] and tab["slots"][82][1] == 2
    assert [p[0] % 4 for p in tab["pieces"][:4]] == [0, 3, 2, 1]  # the stem's rows start at every alignment
    # shape[0] == 1: the unit is the whole tensor, which goes with the whole-tensor items
    assert len(tab["pieces"]) == 64 + 6 + 7 + 5 + 3 and len(tab["whole"]) == 5 and tab["slots"][78] == (85, 1) and tab["slots"][82] == (86, 2)
    assert tab["groups"] == [(0, 0, 82), (1, 82, 85)]
    (lo, hi, i0, i1, pc, wh, k0, ts, by_group), = tab["pairs"]
    assert (lo, hi, i0, i1, pc, wh, k0, ts) == (0, total - 63, 0, len(tab["items"]), (0, 85), (0, 5), 0, list(range(9)))
    n0 = len([it for it in tab["items"] if it[2] < 6])
    assert by_group == [(0, 0, n0), (1, n0, len(tab["items"]))]
    # groups interleaved in memory, consecutive in the table: the table follows param-group order
    order = [0, 6, 1, 7, 2, 8, 3, 4, 5]
    tab2 = _Layerwise.plan_unit_tables([tensors[i] for i in order], W)
    assert [r[2] for r in tab2["tensors"]] == [0, 64, 65, 67, 68, 75, 76, 81, 82]
    # a group's slots are runs of the order given
    assert [(gi, b - a) for gi, a, b in tab2["groups"]] == [(0, 64), (1, 1), (0, 2), (1, 1), (0, 7), (1, 1), (0, 9)]


def test_plan_on_the_resnet50_layout():
    """27,667 slots = 26,560 filters + 1000 FC rows + 107 one-dimensional tensors; with train.filter_from_weight_decay's two groups the slots
    of each group are consecutive"""
    from sota_imagenet_amd.optim import _Layerwise

    table, total = resnet50_table()
    assert len(table) == 161
    two = sorted(range(161), key=lambda i: len(table[i][2]) <= 1)  # group 0: the weights, group 1: the 1-D tensors, each in model order
    for order, group_of in ((list(range(161)), lambda i: 0), (two, lambda i: int(len(table[i][2]) <= 1))):
        tensors = _tensors([(table[i][1], table[i][2]) for i in order], [group_of(i) for i in order])
        tab = _Layerwise.plan_unit_tables(tensors, W)
        _check_cover(tab, tensors, total)
        shapes = [table[i][2] for i in order]
        filters = sum(s[0] for s in shapes if len(s) == 4)
        rows = sum(s[0] for s in shapes if len(s) == 2)
        one_d = sum(1 for s in shapes if len(s) <= 1)
        assert (filters, rows, one_d, len(tab["slots"])) == (26560, 1000, 107, 27667)
        assert len(tab["whole"]) == 107 and len(tab["pieces"]) == sum(s[0] * -(-int(np.prod(s[1:])) // W) for s in shapes if len(s) > 1)
        groups = tab["groups"]
        assert groups == ([(0, 0, 27667)] if order is not two else [(0, 0, 27560), (1, 27560, 27667)])
        assert sum(e - b for _, b, e in tab["pairs"][0][8]) == len(tab["items"])
    # on this layout nearly every work item of the weights spans more than one unit: the element-by-element form is the hot path
    span = sum(1 for off, ln, t in tab["items"] if tab["tensors"][t][1] < tensors[t][3]
               and (off - tab["tensors"][t][0]) // tab["tensors"][t][1] != (off - tab["tensors"][t][0] + ln - 1) // tab["tensors"][t][1])
    weights = sum(1 for _, _, t in tab["items"] if tab["tensors"][t][1] < tensors[t][3])
    assert span > 0.5 * weights


def test_the_unit_rule_is_item_plans_and_sam_uses_it():
    from sota_imagenet_amd.callbacks import SAM

    assert unit_len((64, 3, 7, 7), (147, 1, 21, 3), True, "X") == 147 and unit_len((7,), (1,), True, "X") == 7
    assert unit_len((64, 3, 7, 7), (147, 1, 21, 3), False, "X") == 9408 and unit_len((1, 9), (1, 1), True, "X") == 9
    w = torch.zeros(4, 6).t()
    with pytest.raises(RuntimeError, match="MyNovograd: unitwise needs dim 0"):
        unit_len(w.shape, w.stride(), True, "MyNovograd")
    with pytest.raises(RuntimeError, match="SAM: unitwise needs dim 0"):
        SAM.unit_len(w.shape, w.stride(), True)
    t = [(PB, GB, 0, 12, 3), (PB, GB, 64, 5, 5)]
    assert SAM.plan_tables(t, W) == plan_units(t, W)


@pytest.mark.parametrize("case", CASES)
def test_fixture_is_consistent_with_the_documented_rule(case):
    """the float64 restatement reproduces every recorded p64 to 1e-12 relative; the recorded state is one value per unit (16 distinct ones over
    tensor 0) within the recorded spread; the float32 run's spread stays inside the bound load_state_dict allows; the trajectory is not the
    layer-wise one"""
    fx = UnitFixture(case)
    assert torch.equal(fx.p0, layerwise_common._PROBLEM[0]) and fx.hyper["unitwise_norm"] is True
    got, r = restate_fixture(fx, torch.float64)
    for k in range(6):
        for i, (a, b) in enumerate(zip(fx.split(got[k]), fx.split(fx.p64[k]))):
            rel = ((a - b).abs().max() / b.abs().max()).item()
            assert rel <= 1e-12, (case, k, i, rel)
    assert fx.vs_layerwise > 1e-3 and fx.yard.shape == (6, 5) and 1e-9 < fx.yard.max() < 2e-7
    v5 = fx.split(fx.state5[fx.v_key])
    rows0 = slot_rows(v5[0].view(fx.shapes[0]))
    assert len(torch.unique(rows0[:, 0])) == 16
    assert all(len(torch.unique(v5[i])) == 1 for i in (1, 4))
    assert sorted(fx.state_keys) == sorted(["step", fx.v_key, fx.m_key])
    assert fx.state_shapes[fx.v_key] == [list(s) for s in fx.shapes]
    bound = 2.0 ** -23 / (1 - fx.hyper["betas"][1])
    assert fx.spread.shape == (2, 5) and fx.spread[0].max() < 1e-15 and fx.spread[1].max() <= bound
    # the documented float32 arithmetic lands within the rule the GPU test applies (figures: DESIGN.md section 14)
    nat, _ = restate_fixture(fx, torch.float32, native=True)
    for k in range(6):
        fx.check(k, nat[k], f"{case} float32 restatement")


def test_recipe_48_resolves_and_the_config_files_carry_its_values():
    from sota_imagenet_amd import optim

    assert C.resolve_target("src.optimizers.MyNovograd") is optim.MyNovograd and C.resolve_target("src.optimizers.NovogradApex") is optim.NovogradApex
    kw = dict(weight_decay=0.0002, betas=[0.9, 0.99], lr=0, unitwise_norm=True)
    cfg = C.compose(None, ["+hydra_exp=r50_my-nov-unit"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "src.optimizers.MyNovograd" and got == kw
    assert cfg.loader.batch_size == 192 and cfg.loader.image_size == 224 and cfg.loader.color_twist_prob == 0.3
    assert cfg.run.ema_decay == 0.9993 and cfg.criterion.smoothing == 0.1 and cfg.log.exp_name == "r50_my-nov-unit"
    lr = [0.0001, 0.05]
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 5, lr, "linear"), (5, 90, [lr[1], 0], "cos")]
    assert all(cb["_target_"] == "pytorch_tools.fit_wrapper.callbacks.Callback" for cb in cfg.run.extra_callbacks)  # OrthoInitClb is left out
    cfg = C.compose(None, ["+hydra_exp=my-nov-unit_test"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "src.optimizers.MyNovograd" and got == kw
    assert cfg.log.exp_name == "my-nov-unit_test" and cfg.debug is True and cfg.loader.image_size == 64
    # there is no CPU path: the node instantiates on CUDA parameters only, and says so otherwise
    with pytest.raises(NotImplementedError, match="unitwise_norm=True has no CPU path"):
        C.call(cfg.optim, [{"params": [torch.nn.Parameter(torch.zeros(4))]}])
    o = optim.MyNovograd([torch.nn.Parameter(torch.zeros(4))])
    with pytest.raises(NotImplementedError, match="no CPU path"):
        o.unitwise_norm = True
        o.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3, 2))]})
    for cls, flag in ((optim.AdamLayerwise, "weight_adapt"), (optim.MyAdai, "per_layer")):
        with pytest.raises(NotImplementedError, match=flag):
            cls([torch.nn.Parameter(torch.zeros(4))], **{flag: flag == "weight_adapt"})


P = ctypes.c_void_p


def test_prototypes_parse_and_bad_arguments_return_status():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    A = 4096
    for name in ("mi355_lw_unit_sumsq", "mi355_lw_unit_coef", "mi355_lw_unit_update", "mi355_lw_unit_update_ema"):
        assert getattr(L, name).restype is ctypes.c_int

    def sumsq(src=A, pieces=A, partial=A, n_pieces=1, ns=1, scale=1.0):
        return L.mi355_lw_unit_sumsq(P(src), 64, P(pieces), n_pieces, ns, scale, P(partial), None)

    assert sumsq(src=0) == -1 and "null" in native.last_error()
    assert sumsq(src=A + 4) == -1 and "aligned" in native.last_error()
    assert sumsq(pieces=A + 8) == -1 and "aligned" in native.last_error()
    assert sumsq(partial=A + 4) == -1 and "aligned" in native.last_error()
    assert sumsq(n_pieces=0) == -1 and "n_pieces" in native.last_error()
    assert sumsq(ns=0) == -1 and "n_slots" in native.last_error()
    assert sumsq(scale=float("inf")) == -1 and "scale" in native.last_error()

    def coef(partial=A, slots=A, v=A, den=A, sums=A, n_partial=1, ns=1, b2=0.99, eps=1e-8):
        return L.mi355_lw_unit_coef(P(partial), n_partial, P(slots), ns, P(v), P(den), P(sums), b2, eps, None)

    assert coef(v=0) == -1 and "null" in native.last_error()
    assert coef(den=0) == -1 and "null" in native.last_error()
    assert coef(slots=A + 4) == -1 and "aligned" in native.last_error()
    assert coef(sums=A + 4) == -1 and "aligned" in native.last_error()
    assert coef(v=A + 2) == -1 and "aligned" in native.last_error()
    assert coef(ns=0) == -1 and "n_slots" in native.last_error()
    assert coef(n_partial=0) == -1 and "n_partial" in native.last_error()
    assert coef(b2=1.0) == -1 and "beta2" in native.last_error()
    assert coef(b2=-0.1) == -1 and "beta2" in native.last_error()
    assert coef(eps=-1e-3) == -1 and "eps" in native.last_error()
    assert coef(eps=float("nan")) == -1 and "eps" in native.last_error()

    def update(rule=0, p=A, g=A, m=A, ema=None, items=A, tens=A, den=A, n_items=1, nt=1, ns=1, b1=0.9, lr=1e-3, wd=0.0, soft=0, wd_eps=0.0,
               gs=1.0, decay=0.9):
        args = (64, P(items), n_items, P(tens), nt, P(den), ns, b1, lr, wd, soft, wd_eps, gs)
        if ema is None:
            return L.mi355_lw_unit_update(rule, P(p), P(g), P(m), *args, None)
        return L.mi355_lw_unit_update_ema(rule, P(p), P(g), P(m), P(ema), *args, decay, None)

    assert update(m=0) == -1 and "null" in native.last_error()
    assert update(den=0) == -1 and "null" in native.last_error()
    assert update(g=A + 8) == -1 and "aligned" in native.last_error()
    assert update(tens=A + 8) == -1 and "aligned" in native.last_error()
    assert update(ema=A + 4) == -1 and "aligned" in native.last_error()
    assert update(rule=2) == -1 and "rule" in native.last_error()
    assert update(rule=-1) == -1 and "rule" in native.last_error()
    assert update(n_items=0) == -1 and "n_items" in native.last_error()
    assert update(ns=0) == -1 and "n_slots" in native.last_error()
    assert update(b1=1.0) == -1 and "beta1" in native.last_error()
    assert update(lr=-1.0) == -1 and "lr" in native.last_error()
    assert update(lr=float("inf")) == -1 and "lr" in native.last_error()
    assert update(rule=1, soft=1) == -1 and "wd_eps" in native.last_error()
    assert update(gs=float("inf")) == -1 and "grad_scale" in native.last_error()
    assert update(ema=A, decay=1.5) == -1 and "ema_decay" in native.last_error()
    assert L.mi355_lw_unit_update_ema(0, P(A), P(A), P(A), None, 64, P(A), 1, P(A), 1, P(A), 1, 0.9, 1e-3, 0.0, 0, 0.0, 1.0, 0.9, None) == -1
    assert "null ema" in native.last_error()
