"""The weight penalties in the loss (losses.OrthoLoss / NormLoss, callbacks.OrthoLossClb / NormLossClb, csrc/ortho_loss.hip) on the host: the
planners over the recorded ResNet-50 layout, the work-item cut, the float64 restatement of tests/ortho_loss_common.py against the reference's own
record (tests/golden/ortho_loss_ref.npz), a plain float32 restatement inside the bounds, planted errors outside them, and the criterion algebra."""
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import ortho_loss_common as C
import plan_common
from sota_imagenet_amd import callbacks, config, item_plan, losses, ops

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def r50():
    table, total = plan_common.resnet50_table()
    return [(name, 0, off, shape) for name, off, shape in table], total


@pytest.fixture(scope="module")
def case():
    flat, table = C.make_case()
    mats, n_gram = item_plan.ortho_loss_mats(table, 1)
    Ws = [C.mat_of(flat, m) for m in mats]
    return flat, table, mats, n_gram, Ws


# ---- planners -----------------------------------------------------------------------------------------------------------------------------------
def test_planner_selects_the_reference_matrices_of_resnet50(r50):
    table, total = r50
    by_off = {off: name for name, _, off, _ in table}
    mats, n_gram = item_plan.ortho_loss_mats(table, 384)
    assert sorted(by_off[m[0]] for m in mats) == [f"layer4.{b}.conv{c}.weight" for b in range(3) for c in (1, 2)]
    assert n_gram == 6 * 512 * 512
    mats, n_gram = item_plan.ortho_loss_mats(table, 64)
    names = [by_off[m[0]] for m in mats]
    blocks = [(1, 3), (2, 4), (3, 6), (4, 3)]
    assert sorted(names) == sorted(["conv1.weight"] + [f"layer{l}.{b}.conv{c}.weight" for l, nb in blocks for b in range(nb) for c in (1, 2)])
    assert len(names) == 33 and not any("conv3" in n or "downsample" in n or n.startswith("fc") for n in names)
    assert [m[0] for m in mats] == sorted(m[0] for m in mats)
    g0 = 0
    for off, L, R, g in mats:
        assert g == g0 and R <= L and R >= 64 and off + R * L <= total
        g0 += R * R
    assert g0 == n_gram
    assert (64, 147) in [(m[2], m[1]) for m in mats] and max(m[1] for m in mats) == 4608 and max(m[2] for m in mats) == 512


def test_norm_loss_rows_of_resnet50(r50):
    table, _ = r50
    rows = item_plan.norm_loss_rows(table)
    want = [(off, shape[0], int(np.prod(shape)) // shape[0]) for name, _, off, shape in table if name.endswith(".weight") and int(np.prod(shape)) >= 64]
    assert rows == want and len(rows) == 107  # 53 convs, 53 BatchNorm weights, the FC
    by_off = {off: name for name, _, off, _ in table}
    names = [by_off[r[0]] for r in rows]
    assert "bn1.weight" in names and "fc.weight" in names and not any(n.endswith(".bias") for n in names)
    assert all(r[2] == 1 for r, n in zip(rows, names) if "bn" in n or "downsample.1" in n)
    extra = table + [("eca.weight", 0, 10 ** 8, (1, 1, 5)), ("bn.running_mean", 1, 10 ** 8 + 8, (64,)), ("small.weight", 0, 10 ** 8 + 80, (32,))]
    assert item_plan.norm_loss_rows(extra) == rows
    items, tensors = item_plan.norm_loss_items(rows, ops.NL_ITEM_ELEMS)
    assert len(tensors) == len(rows)
    for (off, R, L), (i0, cnt, rr) in zip(rows, tensors):
        mine = items[i0: i0 + cnt]
        assert rr == R and sum(c for _, _, c in mine) == R and all(ln == L for _, ln, _ in mine)
        assert [o for o, _, _ in mine] == [off + L * sum(c for _, _, c in mine[:k]) for k in range(cnt)]
    assert sum(c for _, c, _ in tensors) == len(items)


def test_tall_record_is_dropped_and_refused(case):
    flat, table, mats, n_gram, _ = case
    assert len(mats) == len(C.SHAPES) and [(m[2], m[1]) for m in mats] == C.SHAPES  # the (256, 64) entry of the table is gone
    assert mats[0][0] % 4 == 1
    assert not np.isfinite(flat[~C.mat_mask(len(flat), mats + [(table[-1][2], C.TALL[1], C.TALL[0])])]).any()
    with pytest.raises(ValueError):
        item_plan.ortho_loss_cut([(0, 64, 256, 0)], C.TILE, C.KSLAB)


def test_constants_agree_with_the_header():
    text = open(os.path.join(HERE, "..", "include", "mi355rn.h")).read()
    assert int(re.search(r"#define MI355_OL_TILE (\d+)", text).group(1)) == ops.OL_TILE == C.TILE
    assert int(re.search(r"#define MI355_OL_KSLAB (\d+)", text).group(1)) == ops.OL_KSLAB == C.KSLAB


# ---- the work-item cut ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["case", "r50"])
def test_cut_covers_every_tile_and_slab_once(which, case, r50):
    mats = case[2] if which == "case" else item_plan.ortho_loss_mats(r50[0], 64)[0]
    cut = item_plan.ortho_loss_cut(mats, C.TILE, C.KSLAB)
    assert [m[:4] for m in cut["mats"]] == list(mats)
    seen_items = set()
    for m, (off, L, R, g0, t0) in enumerate(cut["mats"]):
        nt, ns = -(-R // C.TILE), -(-L // C.KSLAB)
        cover = np.zeros((R, R), dtype=int)  # how often an entry of G is written: the tile and, off the diagonal, its mirror
        for ti in range(nt):
            for tj in range(ti + 1):
                t = t0 + ti * (ti + 1) // 2 + tj
                mm, tij, item0, n_slabs = cut["tiles"][t]
                assert (mm, tij & 0xffff, tij >> 16, n_slabs) == (m, ti, tj, ns)
                assert cut["items"][item0: item0 + ns] == [(t, j) for j in range(ns)]
                seen_items.update(range(item0, item0 + ns))
                r, c = slice(ti * C.TILE, min(R, (ti + 1) * C.TILE)), slice(tj * C.TILE, min(R, (tj + 1) * C.TILE))
                cover[r, c] += 1
                if ti != tj:
                    cover[c, r] += 1
        assert (cover == 1).all()
        assert ns * C.KSLAB >= L > (ns - 1) * C.KSLAB
        mine = [g for g in cut["gitems"] if g[0] == m]
        assert sorted(mine) == [(m, ti, tc, 0) for ti in range(nt) for tc in range(-(-L // C.TILE))]
    assert seen_items == set(range(len(cut["items"]))) and len(cut["tiles"]) == sum(-(-m[2] // C.TILE) * (-(-m[2] // C.TILE) + 1) // 2 for m in mats)
    assert len(cut["gitems"]) == len(set(cut["gitems"]))
    if which == "r50":
        assert len(cut["items"]) >= 4 * 256  # the Gram pass fills 256 CUs several times over
        big = [t for t in cut["tiles"] if cut["mats"][t[0]][1:3] == (4608, 512)]
        assert len(big) == 3 * 36 and all(t[3] == 9 for t in big)


# ---- the restatements ---------------------------------------------------------------------------------------------------------------------------------
def test_data_clear_the_gate(case):
    _, _, mats, _, Ws = case
    for mn in (C.MIN_NORM, 0.0):
        _, _, Fs, gates = C.ortho_loss64(Ws, mn)
        assert all(C.clearance(F, W.shape[0], mn) >= C.CLEAR for F, W in zip(Fs, Ws))
        if mn:
            assert [k for k, g in enumerate(gates) if not g] == [C.ORTHO, C.NEAR]
        else:
            assert [k for k, g in enumerate(gates) if not g] == [C.ORTHO]
    assert Fs[C.ORTHO] == 0.0 and abs(Fs[C.ZERO] - np.sqrt(8)) < 1e-12


def _stage_errors(Ws, got, total, min_norm, s):
    """the worst ratio error / bound per stage of an implementation's [(G, F, gate, coef, dw)] and total, each stage from what it stored before"""
    w = dict(G=0.0, F=0.0, coef=0.0, dw=0.0, gate=0.0, total=0.0)
    for W, (G, F, gate, coef, dw) in zip(Ws, got):
        ref, b = C.gram64(W)
        w["G"] = max(w["G"], C.worst(G, ref, b))
        Fr, bF = C.frob64(G)
        w["F"] = max(w["F"], C.worst(np.array([F]), np.array([Fr]), np.array([bF])))
        gr = C.gate64(C.frob64(ref.astype(np.float32))[0], W.shape[0], min_norm)
        w["gate"] = max(w["gate"], float(gate != gr) * np.inf if gate != gr else 0.0)
        cr, bc = C.coef64(F, gr)
        w["coef"] = max(w["coef"], C.worst(np.array([coef]), np.array([cr]), np.array([bc])))
        dr, bd = C.grad64(W, G, coef, s)
        w["dw"] = max(w["dw"], C.worst(dw, dr, bd))
    tr, bt = C.total64([g[1] for g in got], [C.gate64(float(g[1]), W.shape[0], min_norm) for g, W in zip(got, Ws)])
    w["total"] = C.worst(np.array([total]), np.array([tr]), np.array([bt]))
    return w


def test_float32_restatement_is_inside_the_bounds(case):
    _, _, _, _, Ws = case
    got, total = C.ortho_loss32(Ws, C.MIN_NORM, s=0.37)
    w = _stage_errors(Ws, got, total, C.MIN_NORM, 0.37)
    assert max(w.values()) <= 1.0, w
    assert got[C.ORTHO][1] == 0 and got[C.ORTHO][3] == 0 and not np.isnan(got[C.ORTHO][4]).any()
    assert (got[C.ZERO][4] == 0).all() and got[C.ZERO][2]


@pytest.mark.parametrize("plant, stage", [("transpose", "G"), ("slab", "G"), ("identity", "G"), ("two", "coef"), ("gate", "gate"), ("s", "dw")])
def test_planted_errors_exceed_the_bounds(case, plant, stage):
    _, _, _, _, Ws = case
    got, total = C.ortho_loss32(Ws, C.MIN_NORM, s=0.37, plant=plant)
    w = _stage_errors(Ws, got, total, C.MIN_NORM, 0.37)
    assert w[stage] > 1.0, (plant, w)


def test_restatement_matches_the_reference_record():
    z = np.load(os.path.join(HERE, "golden", "ortho_loss_ref.npz"))
    names = json.loads(str(z["names"]))
    mat = lambda n: z[f"w/{n}"].reshape(z[f"w/{n}"].shape[0], -1)  # noqa: E731
    seen = set()
    for k in (0, 1):
        st = json.loads(str(z[f"ortho/{k}/setting"]))
        table, off = [], 0
        for n in names:  # the module tree as a flat model's table: the planner must select what the reference's walk selected
            table.append((f"{n}.weight", 0, off, tuple(z[f"w/{n}"].shape)))
            off += z[f"w/{n}"].size
        mats, _ = item_plan.ortho_loss_mats(table, st["min_filters"])
        by_off = {t[2]: t[0][: -len(".weight")] for t in table}
        sel = [by_off[m[0]] for m in mats]
        assert sel == list(json.loads(str(z[f"ortho/{k}/F"])))
        loss, grads, Fs, gates = C.ortho_loss64([mat(n) for n in sel], st["min_norm"])
        contributed = json.loads(str(z[f"ortho/{k}/contributed"]))
        assert [n for n, g in zip(sel, gates) if g] == contributed
        seen.add(tuple(contributed))
        assert abs(loss - float(z[f"ortho/{k}/loss"])) <= 1e-12 * abs(loss)
        for n in names:
            ref = z[f"ortho/{k}/g/{n}"].reshape(mat(n).shape)
            got = grads[sel.index(n)] if n in sel else np.zeros_like(ref)
            assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), n
            assert n in contributed or not ref.any()
    assert len(seen) == 2  # one gate is open in one setting and closed in the other
    table = [(f"{n}.weight", 0, 0, tuple(z[f"w/{n}"].shape)) for n in names]
    sel = [names[i] for i, t in enumerate(table) if item_plan.norm_loss_rows([t])]
    assert sel == json.loads(str(z["norm/contributed"])) and "bn64" in sel and "fc" in sel and "bn32" not in sel and "eca" not in sel
    loss, _, _ = C.norm_loss64([mat(n) for n in sel])
    assert abs(loss - float(z["norm/loss"])) <= 1e-12 * abs(loss)
    for n in names:
        ref = z[f"norm/g/{n}"].reshape(mat(n).shape)
        got = C.norm_grad64(mat(n), 1.0)[0] if n in sel else np.zeros_like(ref)
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), n


# ---- the criterion algebra ----------------------------------------------------------------------------------------------------------------------------
class _Term(losses.Loss):
    def __init__(self, value):
        super().__init__()
        self.value, self.calls = value, []

    def forward(self, y_pred, y_true):
        self.calls.append((y_pred, y_true))
        return torch.tensor(self.value)


def test_sum_and_weighted_terms_see_the_same_arguments():
    ce, pen = _Term(2.0), _Term(5.0)
    crit = ce + pen * 0.1
    assert isinstance(crit, losses.Loss) and isinstance(losses.CrossEntropyLoss(smoothing=0.1), losses.Loss)
    a, b = torch.zeros(2, 3), torch.ones(2, 3)
    out = crit(a, b)
    assert abs(float(out) - 2.5) < 1e-6
    assert len(ce.calls) == len(pen.calls) == 1 and ce.calls[0][0] is a and pen.calls[0][0] is a and ce.calls[0][1] is b and pen.calls[0][1] is b
    assert abs(float((0.5 * pen + ce)(a, b)) - 4.5) < 1e-6
    with pytest.raises(ValueError):
        ce + 1.0
    with pytest.raises(ValueError):
        ce * pen
    crit += pen * 2
    assert abs(float(crit(a, b)) - 12.5) < 1e-6


def test_aliases_and_type_2():
    for mod in ("src", "sota_imagenet"):
        assert config.resolve_target(f"{mod}.callbacks.OrthoLossClb") is callbacks.OrthoLossClb
        assert config.resolve_target(f"{mod}.callbacks.NormLossClb") is callbacks.NormLossClb
    with pytest.raises(NotImplementedError):
        callbacks.OrthoLossClb(type=2)
    c = callbacks.OrthoLossClb(type=1, weight=0.001, min_filters=64, min_norm=0)
    assert c.weight == 0.001 and c.kwargs == dict(min_filters=64, min_norm=0)
    assert callbacks.OrthoLossClb().weight == 0.01 and callbacks.NormLossClb().weight == 1e-4


def test_term_is_appended_once():
    made = []

    class Clb(callbacks.OrthoLossClb):
        def _make_term(self):
            made.append(_Term(3.0))
            return made[-1]

    ce = _Term(1.0)
    clb = Clb(weight=0.5)
    clb.set_state(types.SimpleNamespace(criterion=ce, model=None))
    clb.on_begin()
    first = clb.state.criterion
    assert abs(float(first(None, None)) - 2.5) < 1e-6
    clb.on_begin()  # the next stage's fit
    assert clb.state.criterion is first and len(made) == 1
    bad = Clb()
    bad.set_state(types.SimpleNamespace(criterion=torch.nn.MSELoss(), model=None))
    with pytest.raises(TypeError):
        bad.on_begin()


def test_cpu_and_non_flat_models_are_refused():
    from sota_imagenet_amd.models import resnet50

    cpu = resnet50(dtype="fp32")
    torch_model = torch.nn.Sequential(torch.nn.Conv2d(3, 64, 3))
    for model in (cpu, torch_model):
        for make in (lambda m: losses.OrthoLoss(m, min_filters=64), losses.NormLoss):
            with pytest.raises(NotImplementedError):
                make(model)
        for clb in (callbacks.OrthoLossClb(), callbacks.NormLossClb()):
            clb.set_state(types.SimpleNamespace(criterion=losses.CrossEntropyLoss(), model=model))
            with pytest.raises(NotImplementedError):
                clb.on_begin()
            assert isinstance(clb.state.criterion, losses.CrossEntropyLoss)
