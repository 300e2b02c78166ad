"""WeightDistributionTB without a GPU: the edge table, the trimming, the values that lie in no bin, the callback's host rule against the numpy
restatement of weight_dist_common, log.histogram in train.py's callback list, the alias, the two configs that carry the switch, the plan over a
hand-made set of views, and the callback's gates."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import weight_dist_common as WD  # noqa: E402
from sota_imagenet_amd import callbacks, config as C, fit_wrapper as fw, item_plan, ops  # noqa: E402
from sota_imagenet_amd.fit_wrapper import RunnerState  # noqa: E402


# ---- the edges ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_edge_table():
    e = WD.EDGES
    assert e.dtype == np.float64 and e.shape == (WD.N_EDGES,) == (1549,) and WD.N_BINS == 1548
    assert (e > 0).sum() == (e < 0).sum() == WD.N_POS == 774 and e[774] == 0.0
    assert e[-1] == WD.E_LAST == 9.920775621859783e+19 and e[0] == -WD.E_LAST and e[775] == 1e-12
    assert (np.diff(e) > 0).all() and np.array_equal(e, -e[::-1])
    assert e[-1] * 1.1 >= 1e20  # the recurrence stops here
    # formed by the recurrence: a power differs from it in the last bits somewhere
    assert not np.array_equal(e[775:], 1e-12 * 1.1 ** np.arange(774))


def test_ops_edges_are_the_table_and_the_constants_agree():
    e = ops.tbbin_edges()
    assert e.dtype == np.float64 and np.array_equal(e, WD.EDGES)
    assert (ops.TBBIN_POS, ops.TBBIN_BINS, ops.TBBIN_NOBIN, ops.TBBIN_STATS) == (774, 1548, 1548, 5)
    assert ops.TBBIN_ROW % 4 == 0 and ops.TBBIN_ROW > ops.TBBIN_NOBIN
    text = open(os.path.join(ROOT, "sota_imagenet_amd", "csrc", "optim_wdist.hip")).read()
    for name, want in (("kPos", "774"), ("kBins", "2 * kPos"), ("kNoBin", "kBins"), ("kRow", str(ops.TBBIN_ROW)), ("kStats", str(ops.TBBIN_STATS))):
        assert f"constexpr int {name} = {want};" in text, name


def test_only_zero_is_a_float32_edge():
    e = WD.EDGES
    assert (e.astype(np.float32).astype(np.float64) == e).sum() == 1


# ---- trimming ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim", [WD.trim, lambda c: callbacks.tb_trim(np.asarray(c), WD.EDGES)], ids=["restatement", "callback"])
def test_trimming_on_hand_made_counts(trim):
    e = WD.EDGES
    c = np.zeros(1548, dtype=np.int64)
    with pytest.raises(ValueError):
        trim(c)
    c[0], c[2] = 4, 1  # support at bin 0: a zero is put in front
    assert trim(c) == (e[0:4].tolist(), [0, 4, 0, 1])
    c[:] = 0
    c[1547], c[1545] = 7, 2  # support at the last bin: the limits end with the last edge
    assert trim(c) == (e[1545:1549].tolist(), [0, 2, 0, 7])
    c[:] = 0
    c[800] = 3  # a single bin: its left neighbour and itself, two limits
    assert trim(c) == (e[800:802].tolist(), [0, 3])
    c[:] = 0
    c[0] = 5
    assert trim(c) == (e[0:2].tolist(), [0, 5])


def test_trimming_is_make_histogram_where_it_imports():
    try:
        from torch.utils.tensorboard.summary import make_histogram
    except Exception:
        pytest.skip("torch.utils.tensorboard does not import here (no tensorboard package)")
    rng = np.random.default_rng(0)
    for v in (rng.normal(size=1000), np.array(WD.EXAMPLE), np.zeros(5), -np.abs(rng.normal(size=77)) * 1e-3):
        h, want = make_histogram(v.astype(float), WD.EDGES.tolist()), WD.histogram(v)
        assert list(h.bucket_limit) == want["bucket_limits"] and [int(c) for c in h.bucket] == want["bucket_counts"]
        assert h.num == want["num"] and WD.same(h.min, want["min"]) and WD.same(h.sum, want["sum"])


# ---- counting ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_example_counts_eight():
    v = np.array(WD.EXAMPLE)
    c = WD.counts_of(v)
    assert c.sum() == 8
    assert c[774] == 3  # 0.0, -0.0 and 1e-13 lie in [0, 1e-12)
    assert c[773] == 1 and c[1547] == 1 and c[0] == 1  # -1e-13; the last edge (closed on the right); the first edge
    assert np.array_equal(callbacks.tb_host_counts(v, WD.EDGES), c)
    h = WD.histogram(v)
    assert h["num"] == 13 and h["min"] != h["min"] and h["max"] != h["max"] and h["sum"] != h["sum"]


def test_the_host_rule_is_np_histogram():
    """the callback's host rule (by position) against np.histogram: at every edge and its float64 neighbours, integers (the num_batches_tracked
    case), and a spread of magnitudes"""
    e = WD.EDGES
    rng = np.random.default_rng(1)
    spread = 10.0 ** rng.uniform(-14, 21, 5000) * rng.choice([-1.0, 1.0], 5000)
    v = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), np.arange(0.0, 300.0), spread, WD.EXAMPLE])
    assert np.array_equal(callbacks.tb_host_counts(v, e), WD.counts_of(v))
    ints = np.array([0, 1, 7, 5004], dtype=np.int64).astype(np.float64)
    assert np.array_equal(callbacks.tb_host_counts(ints, e), WD.counts_of(ints))


# ---- wiring ------------------------------------------------------------------------------------------------------------------------------------------
def test_log_histogram_selects_the_callback_in_train_py():
    import train

    on = train.histogram_callback(C.compose(None, ["+hydra_exp=nov_hist_test"]))
    assert type(on) is callbacks.WeightDistributionTB and on.last == {} and on.logged == 0
    off = train.histogram_callback(C.compose(None, ["+hydra_exp=nov_full_test"]))
    assert type(off) is fw.Callback
    off = train.histogram_callback(C.compose(None, ["+hydra_exp=nov_hist_test", "log.histogram=false"]))
    assert type(off) is fw.Callback
    text = open(os.path.join(ROOT, "train.py")).read()
    assert text.count("histogram_callback(cfg),") == 1  # the helper is what main() puts into the list


def test_the_alias_resolves():
    assert C.resolve_target("src.callbacks.WeightDistributionTB") is callbacks.WeightDistributionTB
    assert C.WEIGHT_HISTOGRAM_TARGET_ALIASES == {"src.callbacks.WeightDistributionTB": "sota_imagenet_amd.callbacks.WeightDistributionTB"}
    assert C.resolve_target("src.callbacks.GradDistributionTB") is callbacks.GradDistributionTB  # the tables before it still answer
    assert len(C.LOGGING_CALLBACK_TARGET_ALIASES) == 1
    assert type(C.call({"_target_": "src.callbacks.WeightDistributionTB"})) is callbacks.WeightDistributionTB


@pytest.mark.parametrize("name", ["nov_hist_test", "r50_nov_full"])
def test_the_configs_carry_the_switch(name):
    cfg = C.compose(None, [f"+hydra_exp={name}"])
    assert cfg.log.histogram is True
    assert [c["_target_"] for c in cfg.run.extra_callbacks] == ["src.callbacks.OrthoInitClb", "src.callbacks.GradDistributionTB"]


def test_nov_hist_test_is_nov_full_test_plus_the_switch():
    a, b = C.to_plain(C.compose(None, ["+hydra_exp=nov_hist_test"])), C.to_plain(C.compose(None, ["+hydra_exp=nov_full_test"]))
    assert a["log"].pop("histogram") is True and b["log"].pop("histogram") is False
    assert a["log"].pop("exp_name") == "nov_hist_test" and b["log"].pop("exp_name") == "nov_full_test"
    assert a == b


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_plan_covers_every_element_once_and_nothing_else():
    """two storages, an int64 entry between their views, views that start 1, 2 and 3 elements behind a 16-byte boundary, one longer than two work
    items: every element of every fp32 view lies in exactly one item of its launch, the gaps and the int64 entry in none"""
    W = 64
    s1, s2 = torch.zeros(1000), torch.zeros(300)
    nbt = torch.zeros(3, dtype=torch.int64)
    views = [s1[8:8 + 5], s2[1:1 + 130].view(10, 13), nbt[1], s1[21:21 + 2 * W + 5], s1[300:300 + W].view(4, 4, 4).permute(0, 2, 1), s2[142:143],
             s2[147:147 + 63]]
    records = [item_plan.dense_range(v) if v.dtype == torch.float32 else None for v in views]
    rows, launches, spans, n_items = item_plan.dist_plan(records, W)
    assert rows == [0, 1, 3, 4, 5, 6] and len(launches) == 2 and [l[0] for l in launches] == [s1.data_ptr(), s2.data_ptr()]
    assert sum(len(l[3]) for l in launches) == n_items and [l[4] for l in launches] == [0, len(launches[0][3])]
    seen = {s1.data_ptr(): np.zeros(1000, dtype=np.int64), s2.data_ptr(): np.zeros(300, dtype=np.int64)}
    owner = {s1.data_ptr(): np.full(1000, -1), s2.data_ptr(): np.full(300, -1)}
    per_row = [0] * len(rows)
    flat_items = []
    for base, lo, hi, items, i0 in launches:
        assert lo % 4 == 0 and lo >= 0
        for off, ln, row in items:
            assert 1 <= ln <= W and 0 <= off and off + ln <= hi - lo
            seen[base][lo + off: lo + off + ln] += 1
            owner[base][lo + off: lo + off + ln] = row
            per_row[row] += ln
            flat_items.append(row)
    want = {k: np.zeros_like(v) for k, v in seen.items()}
    for row, k in enumerate(rows):
        base, first, n = records[k]
        want[base][first: first + n] += 1
        assert (owner[base][first: first + n] == row).all() and per_row[row] == n == views[k].numel()
        i0, c = spans[row]
        assert flat_items[i0: i0 + c] == [row] * c and c == -(-n // W)  # the items of a row are consecutive in the shared per-item array
    for k in seen:
        assert np.array_equal(seen[k], want[k]) and seen[k].max() == 1
    assert any(records[k][1] % 4 == r for r in (1, 2, 3) for k in rows)


def test_a_plan_without_kernel_entries_is_empty():
    assert item_plan.dist_plan([None, None], 64) == ([], [], [], 0)


# ---- the callback's gates ------------------------------------------------------------------------------------------------------------------------------
def _on(model, **state):
    cb = callbacks.WeightDistributionTB()
    st = RunnerState(model=model)
    for k, v in state.items():
        setattr(st, k, v)
    cb.set_state(st)
    return cb


def test_cpu_tensors_raise_not_implemented():
    cb = _on(torch.nn.BatchNorm1d(3))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        cb.on_epoch_begin()


def test_the_gates(monkeypatch):
    cb = _on(torch.nn.Linear(2, 2))
    calls = []
    monkeypatch.setattr(cb, "log", lambda: calls.append(1))
    cb.on_epoch_begin()
    assert calls == [1]
    cb.state.rank = 1
    cb.on_epoch_begin()  # rank > 0 does nothing
    assert calls == [1] and cb.last == {}
    cb.state.rank = 0
    monkeypatch.setenv("RANK", "2")
    cb.on_epoch_begin()
    assert calls == [1]
    monkeypatch.delenv("RANK")
    cb.on_epoch_begin()
    cb.on_batch_end()  # only the epoch's begin logs
    cb.on_epoch_end()
    assert calls == [1, 1]
