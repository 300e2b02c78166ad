"""Backward centred weight normalisation (sota_imagenet_amd.callbacks.WeightNorm, csrc/weight_norm.hip) without a GPU: the planner on the two
executors' tables, the cut of the rows into work items, the float64 restatement of the rule against the reference's recorded run, the target
table and the config files of recipe 14, the entry point's validation and the callback's refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import exec_gpu_common as E
import weight_norm_common as WN
from plan_common import resnet50_table
from sota_imagenet_amd import config as C
from sota_imagenet_amd import item_plan, native
from sota_imagenet_amd.fit_wrapper import RunnerState

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_LENS = {64, 128, 147, 256, 512, 576, 1024, 1152, 2048, 2304, 4608}


# ---- the planner -----------------------------------------------------------------------------------------------------------------------------------
def _check_resnet50_records(recs, table):
    """table: [(name, kind, off, shape)]"""
    assert len(recs) == 54  # 53 convolutions and the FC
    assert sum(rows for _, rows, _ in recs) == 27560 and sum(rows * L for _, rows, L in recs) == 25502912
    assert {L for _, _, L in recs} == ROW_LENS
    by_off = {off: (name, shape) for name, kind, off, shape in table if kind == 0}
    assert [r[0] for r in recs] == [off for _, kind, off, shape in table if kind == 0 and len(shape) >= 2]  # table order
    names = [by_off[r[0]][0] for r in recs]
    assert all(n.endswith(".weight") and ("conv" in n or "downsample.0" in n or n == "fc.weight") for n in names)
    assert "fc.bias" not in names and not any("bn" in n or "downsample.1" in n for n in names)  # no BatchNorm tensor, no bias
    for off, rows, L in recs:
        shape = by_off[off][1]
        assert rows == shape[0] and rows * L == int(np.prod(shape))
    assert recs[names.index("conv1.weight")][1:] == (64, 147) and recs[names.index("fc.weight")][1:] == (1000, 2048)  # without the padding rows
    spans = sorted((off, off + rows * L) for off, rows, L in recs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_records_of_the_recorded_resnet50_layout():
    table, total = resnet50_table()
    full = [(name, 0, off, shape) for name, off, shape in table] + [("bn1.running_mean", 1, 0, (64,)), ("stat.weight", 1, 64, (64, 64))]
    recs = item_plan.wnorm_records(full)
    _check_resnet50_records(recs, full)
    assert max(off + rows * L for off, rows, L in recs) <= total


def test_records_of_the_resnet50_model():
    m = E.resnet50()
    recs = item_plan.wnorm_records(m._table)
    _check_resnet50_records(recs, m._table)
    off = {name: off for name, kind, off, _ in m._table if kind == 0}["fc.weight"]
    assert m.fc.weight.shape == (1000, 2048) and (off, 1000, 2048) in recs


def test_records_of_the_bresnet50_model_hold_no_conv1d():
    m = E.bresnet50()
    recs = item_plan.wnorm_records(m._table)
    shapes = {off: shape for _, kind, off, shape in m._table if kind == 0}
    eca = [sh for sh in shapes.values() if len(sh) == 3]
    assert eca and all(int(np.prod(sh)) < 64 for sh in eca)  # the ECA weights exist, and fall under numel < 64 as in the reference
    assert all(len(shapes[r[0]]) in (2, 4) for r in recs)
    assert len(recs) == sum(len(sh) in (2, 4) for sh in shapes.values())
    assert (32, 27) in [r[1:] for r in recs]  # the deep stem's first convolution: numel 864, rows of 27


def test_hand_made_table():
    table = [("a.weight", 0, 0, (8, 4, 3, 3)), ("a.bn.weight", 0, 320, (64,)), ("a.bn.running_mean", 1, 0, (64,)), ("e.weight", 0, 384, (1, 1, 5)),
             ("fc.weight", 0, 448, (10, 32)), ("fc.bias", 0, 1472, (10,)), ("buf.weight", 1, 64, (8, 8)), ("tiny.weight", 0, 1536, (7, 9)),
             ("c1d.weight", 0, 1600, (4, 4, 5))]
    assert item_plan.wnorm_records(table) == [(0, 8, 36), (448, 10, 32), (1600, 4, 20)]  # ndim >= 2 and numel >= 64, parameters only


@pytest.mark.parametrize("W", [256, 4096, 5000])
def test_items_cover_every_record_exactly(W):
    recs = [(3, 5, 147), (1000, 4, 64), (2000, 130, 2), (3000, 1, 4608), (9000, 2, W), (9000 + 2 * W, 2, W + 1), (40000, W // 64 + 1, 64),
            (80000, 3, 20011), (200000, 7, 1)]
    items = item_plan.wnorm_items(recs, W)
    k = 0
    for off, rows, L in recs:
        per = max(1, W // L)
        mine = items[k:k + (rows + per - 1) // per]
        k += len(mine)
        assert all(i[1] == L and 1 <= i[2] <= per for i in mine)          # whole rows, at most max(1, W // row_len) of them
        assert all(i[2] == per for i in mine[:-1])                        # full items up to the last
        assert mine[0][0] == off and sum(i[2] for i in mine) == rows      # from the record's first row, exactly its rows
        assert all(b[0] == a[0] + a[1] * a[2] for a, b in zip(mine, mine[1:]))  # consecutive and disjoint
        # the cuts depend on (rows, row_len, W) alone: the same record elsewhere, and after other records, is cut alike
        moved = item_plan.wnorm_items([(off + 12345, rows, L)], W)
        assert [(f - 12345, ln, nr) for f, ln, nr in moved] == mine
        if L > W:
            assert all(i[2] == 1 for i in mine) and len(mine) == rows  # one row per item
    assert k == len(items)
    with pytest.raises(ValueError):
        item_plan.wnorm_items([(0, 0, 4)], W)
    with pytest.raises(ValueError):
        item_plan.wnorm_items([(0, 4, 0)], W)


def test_items_of_resnet50_and_their_packing():
    from sota_imagenet_amd import ops

    table, total = resnet50_table()
    recs = item_plan.wnorm_records([(name, 0, off, shape) for name, off, shape in table])
    items = item_plan.wnorm_items(recs, ops.WNORM_ITEM_ELEMS)
    assert sum(nr for _, _, nr in items) == 27560 and sum(L * nr for _, L, nr in items) == 25502912
    assert all(L * nr <= max(L, ops.WNORM_ITEM_ELEMS) for _, L, nr in items) and max(f + L * nr for f, L, nr in items) <= total
    ops.wnorm_check_items(items)
    t = item_plan.pack_records(items[:3])
    assert t.dtype == torch.int64 and tuple(t.shape) == (3, 2)
    raw = np.frombuffer(t.numpy().tobytes(), dtype=np.dtype([("first", "<i8"), ("row_len", "<i4"), ("n_rows", "<i4")]))
    assert [tuple(int(x) for x in r) for r in raw] == [tuple(i) for i in items[:3]]
    with pytest.raises(ValueError, match="overlaps"):
        ops.wnorm_check_items([(0, 16, 4), (63, 8, 1)])
    ops.wnorm_check_items([(64, 8, 1), (0, 16, 4)])  # any order, touching


def test_the_constants_of_host_and_kernel_agree():
    from sota_imagenet_amd import ops

    assert native.lib().mi355_wnorm_wave_row_max() == ops.WNORM_WAVE_ROW_MAX
    assert ops.WNORM_ITEM_ELEMS >= 4 * 64


# ---- the rule against the reference's recorded run -------------------------------------------------------------------------------------------------
def _fixture():
    return np.load(os.path.join(HERE, "golden", "weight_norm_ref.npz"))


def test_float64_rule_against_the_reference_fixture():
    z = _fixture()
    names, skipped = json.loads(bytes(z["names"])), json.loads(bytes(z["skipped"]))
    assert set(skipped) == {"eca", "bn32"} and "bn64" in names
    checked = 0
    for d in range(2):
        for name in names:
            b, f = z[f"d{d}/{name}/before"], z[f"d{d}/{name}/after"]
            if f"d{d}/{name}/bias_before" in z:
                assert np.array_equal(z[f"d{d}/{name}/bias_before"], z[f"d{d}/{name}/bias_after"])
            if name in skipped:
                assert b.size < 64 and np.array_equal(b, f)
                continue
            if name == "bn64":  # departure 1: the reference turns a BatchNorm weight of 64 channels into NaN
                assert b.shape == (64,) and np.isfinite(b).all() and np.isnan(f).all()
                continue
            x = b.reshape(b.shape[0], -1)
            M, N, Y = WN.rule64(x)
            ok = N[:, 0] > 0
            got = f.reshape(x.shape)
            assert np.isnan(got[~ok]).all() and np.isnan(Y[~ok]).all()  # a constant row: 0 / 0
            assert (~ok).sum() == (1 if name == "flat" else 0)
            r = WN.worst_ratio(got[ok], Y[ok], WN.reference_bound(x[ok], M[ok], N[ok], Y[ok]))
            assert r <= 1.0, (d, name, r)
            checked += 1
    assert checked == 10


def test_the_bounds_on_a_hand_computed_row():
    x = np.array([[1.0, 2.0, 3.0, 6.0]], dtype=np.float32)
    M, N, Y = WN.rule64(x)
    assert M[0, 0] == 3.0 and N[0, 0] == np.sqrt(14.0) and np.allclose(Y[0], np.array([-2, -1, 0, 3]) / np.sqrt(14.0), rtol=1e-15)
    nb, rb = WN.native_bound(M, N, Y), WN.reference_bound(x, M, N, Y)
    assert np.allclose(nb[0], 8 * WN.U * np.abs(Y[0]) + 12 * WN.U / np.sqrt(14.0), rtol=1e-15)
    assert np.allclose(rb[0] - nb[0], 4 * WN.U * 3.0 / np.sqrt(14.0), rtol=1e-12)  # G = 2 + log2 4, mean|x| = 3


# ---- targets and configs ---------------------------------------------------------------------------------------------------------------------------
def test_targets():
    from sota_imagenet_amd import callbacks

    assert C.WEIGHT_CALLBACK_TARGET_ALIASES == {"src.callbacks.WeightNorm": "sota_imagenet_amd.callbacks.WeightNorm",
                                                "sota_imagenet.callbacks.WeightNorm": "sota_imagenet_amd.callbacks.WeightNorm"}
    for spelling in C.WEIGHT_CALLBACK_TARGET_ALIASES:
        assert C.resolve_target(spelling) is callbacks.WeightNorm
    # the older tables hold no WeightNorm, and still resolve
    for tab in (C.TARGET_ALIASES, C.LAYERWISE_TARGET_ALIASES, C.CALLBACK_TARGET_ALIASES, C.ADAMP_TARGET_ALIASES, C.INIT_CALLBACK_TARGET_ALIASES,
                C.LOGGING_CALLBACK_TARGET_ALIASES, C.WEIGHT_HISTOGRAM_TARGET_ALIASES):
        assert not any("WeightNorm" in k for k in tab)
    assert C.resolve_target("src.callbacks.OrthoInitClb") is callbacks.OrthoInitClb
    assert C.resolve_target("src.callbacks.WeightDistributionTB") is callbacks.WeightDistributionTB
    assert C.resolve_target("torch.optim.AdamW").__module__ == "sota_imagenet_amd.optim"


def test_recipe_14_and_its_smoke_config():
    from sota_imagenet_amd import callbacks

    cfg = C.compose(None, ["+hydra_exp=r50_adamw_std"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "torch.optim._multi_tensor.AdamW" and got == dict(weight_decay=1e-2, eps=1e-6, lr=0)
    assert cfg.log.exp_name == "r50_adamw_std" and cfg.log.histogram is True and cfg.init_gamma == 1.7 and cfg.criterion.smoothing == 0.1
    assert cfg.loader.batch_size == 256 and cfg.loader.image_size == 224
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 8, [0, 0.01], "linear"), (8, 90, [0.01, 0], "cos")]
    want = [{"_target_": "src.callbacks.WeightNorm"}]
    assert C.to_plain(cfg.run.extra_callbacks) == want
    test = C.compose(None, ["+hydra_exp=adamw_std_test"])
    assert C.to_plain(test.run.extra_callbacks) == want and C.to_plain(test.optim) == C.to_plain(cfg.optim) and test.init_gamma == 1.7
    assert test.log.exp_name == "adamw_std_test" and test.log.histogram is True and test.debug is True
    assert test.loader.image_size == 64 and test.loader.batch_size == 16 and [(s["start"], s["end"]) for s in test.run.stages] == [(0, 1), (1, 2)]
    for c in (cfg, test):
        made = [C.call(cb) for cb in c.run.extra_callbacks]
        assert type(made[0]) is callbacks.WeightNorm and made[0].records == [] and made[0].launches == 0


def test_the_stale_keys_of_the_recipe_raise():
    from sota_imagenet_amd.callbacks import WeightNorm

    with pytest.raises(TypeError):
        WeightNorm(gamma=1.7)
    with pytest.raises(TypeError):
        C.call({"_target_": "src.callbacks.WeightNorm", "gamma": 1.7, "use_std": True})


def test_a_cpu_model_is_refused():
    from sota_imagenet_amd.callbacks import WeightNorm

    for model in (E.resnet50(), torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.Linear(8, 4))):
        before = [p.detach().clone() for p in model.parameters()]
        cb = WeightNorm()
        cb.set_state(RunnerState(model=model))
        for call in (cb.on_begin, cb.on_batch_end):
            with pytest.raises(NotImplementedError, match="no CPU path"):
                call()
        assert cb.launches == 0 and cb.status is None
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
        cb.state.is_train = False  # a validation batch asks nothing of the model
        cb.on_batch_end()


# ---- the entry point -------------------------------------------------------------------------------------------------------------------------------
P = ctypes.c_void_p


def test_entry_point_returns_status_on_bad_arguments():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    assert L.mi355_weight_norm_rows.restype is ctypes.c_int
    A = 4096

    def call(w=A, n=64, items=A, n_items=1, status=A):
        return L.mi355_weight_norm_rows(P(w), n, P(items), n_items, P(status), None)

    for bad in (dict(w=None), dict(items=None), dict(status=None), dict(w=A + 4), dict(w=A + 8), dict(items=A + 8), dict(status=A + 2), dict(n=0),
                dict(n_items=0), dict(n_items=(1 << 30) + 1)):
        assert call(**bad) == -1, bad
        assert "weight_norm_rows" in native.last_error()


def test_the_wrapper_checks_its_arguments_before_the_library_is_asked():
    from sota_imagenet_amd import ops

    items = [(0, 4, 2)]
    with pytest.raises(ValueError):  # a CPU array
        ops.weight_norm_rows_(torch.zeros(64), items, item_plan.pack_records(items))
