"""WeightDistributionTB on the MI355X: the counting kernel of csrc/optim_wdist.hip against the numpy restatement of add_histogram's rule
(weight_dist_common: np.histogram over the 1549 default edges, the trimming, float64 statistics) — at every edge, over the item geometry, on values
outside the table and on all-equal arrays — its argument checks, the callback on a hand-made module, on the flat ResNet-50 and on BResNet-50, and
the smoke config with log.histogram through train.py.  Counts, limits, min and max are compared exactly; the two sums, which the kernel adds in
another order than numpy, within the worst-case bound of two float64 summations of n terms: 2 (n - 1) 2^-53 sum|x|."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import flat_layout  # noqa: E402
import weight_dist_common as WD  # noqa: E402
from flat_layout import _ops  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
U = 2.0 ** -53


def _draw(rng, n):
    """u uniform over [-14, 3]: both sides of the smallest edges, nothing outside the table"""
    return flat_layout._draw(rng, n, -14.0, 3.0)


def _layout(arrays, offsets=None, tail=9):
    """NaN everywhere between the arrays"""
    return flat_layout._layout(arrays, offsets, NAN, tail)


def _run(dev, flat, recs):
    """one launch over the records: (hist [n, ROW] int64, per tensor the rows of partial[])"""
    ops, item_plan = _ops()
    items, spans = item_plan.plan_items(recs, ops.lw_item_elems())
    hist = torch.zeros(len(recs), ops.TBBIN_ROW, dtype=torch.int32, device=dev)
    partial = torch.full((len(items), ops.TBBIN_STATS), 7.0, dtype=torch.float64, device=dev)
    ops.tbbin_hist(torch.from_numpy(flat).to(dev), item_plan.pack_records(items, dev), hist, partial)
    p = partial.cpu().numpy()
    return hist.cpu().numpy().astype(np.int64), [p[i0:i0 + c] for i0, c in spans]


def _stats(rows):
    """a tensor's statistics from its items, as the callback combines them: in table order, min and max NaN where a NaN was seen"""
    nan = bool(rows[:, 4].any())
    return dict(min=NAN if nan else float(rows[:, 0].min()), max=NAN if nan else float(rows[:, 1].max()), sum=float(np.cumsum(rows[:, 2])[-1]),
                sum_squares=float(np.cumsum(rows[:, 3])[-1]))


def _check_stats(got, x, what=""):
    """min and max exactly; the sums within the bound of two float64 summations in different orders (NaN and infinities as numpy has them)"""
    v = np.asarray(x).astype(np.float64).ravel()
    with np.errstate(invalid="ignore"):  # inf - inf is NaN, in numpy's sum as in the kernel's
        want = dict(min=float(v.min()), max=float(v.max()), sum=float(v.sum()), sum_squares=float(v.dot(v)))
    print(what, {k: (got[k], want[k]) for k in want})
    assert WD.same(got["min"], want["min"]) and WD.same(got["max"], want["max"]), what
    for key, mass in (("sum", np.abs(v).sum()), ("sum_squares", (v * v).sum())):
        if np.isfinite(want[key]):
            assert abs(got[key] - want[key]) <= 2 * (v.size - 1) * U * mass, (what, key, got[key], want[key])
        else:
            assert WD.same(got[key], want[key]), (what, key, got[key], want[key])


# ---- 1. the edges --------------------------------------------------------------------------------------------------------------------------------------
def test_counts_at_every_edge(dev):
    """for every non-zero edge float32(edge) and its two float32 neighbours, 0.0, -0.0 and the smallest denormals of both signs: no edge but 0 is a
    float32, so every one of these comparisons is decided by digits a float32 cannot hold"""
    ops, _ = _ops()
    e = WD.EDGES[WD.EDGES != 0].astype(np.float32)
    tiny = np.float32(1e-45)
    x = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)),
                        np.float32([0.0, -0.0]), np.array([tiny, -tiny], dtype=np.float32)])
    assert tiny > 0 and x.size == 3 * 1548 + 4
    hist, parts = _run(dev, *_layout([x]))
    want = WD.counts_of(x)
    assert np.array_equal(hist[0, :ops.TBBIN_BINS], want)
    assert hist[0, ops.TBBIN_NOBIN] == x.size - want.sum() == 2  # one float above the last edge, one below the first
    assert (hist[0, ops.TBBIN_NOBIN + 1:] == 0).all()
    # float32(1e-12) lies below 1e-12: [0, 1e-12) takes 0.0, -0.0, the denormal, that float and the one below it; [-1e-12, 0) the mirror images
    assert want[774] == 5 and want[773] == 3
    _check_stats(_stats(parts[0]), x, "edges")


# ---- 2. the item geometry ------------------------------------------------------------------------------------------------------------------------------
def test_item_geometry_gaps_and_reproducibility(dev):
    ops, _ = _ops()
    W = ops.lw_item_elems()
    rng = np.random.default_rng(2)
    sizes = (1, 3, W - 1, W, W + 1, 2 * W + 5, 2, 5)
    arrays = [_draw(rng, n) for n in sizes]
    offsets, end = [], 0
    for i, n in enumerate(sizes):  # first elements at 0, 1, 2, 3 (mod 4), a gap of NaN in front of every tensor but the first
        off = 0 if i == 0 else (end + 4 + 3) // 4 * 4 + i % 4
        offsets.append(off)
        end = off + n
    assert {o % 4 for o in offsets} == {0, 1, 2, 3}
    flat, recs = _layout(arrays, offsets)
    assert np.isnan(flat).sum() == flat.size - sum(sizes) > 0
    hist, parts = _run(dev, flat, recs)
    for t, a in enumerate(arrays):
        assert np.array_equal(hist[t, :ops.TBBIN_BINS], WD.counts_of(a)), t
        assert hist[t, ops.TBBIN_NOBIN] == 0 and hist[t, :ops.TBBIN_BINS].sum() == a.size  # no NaN of a gap was read
        assert len(parts[t]) == -(-a.size // W) and (parts[t][:, 4] == 0).all()
        _check_stats(_stats(parts[t]), a, f"tensor {t} ({a.size})")
    hist2, parts2 = _run(dev, flat, recs)
    assert np.array_equal(hist, hist2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts, parts2))  # bit for bit


# ---- 3. values outside the table -----------------------------------------------------------------------------------------------------------------------
def test_values_outside_the_table(dev):
    ops, _ = _ops()
    W = ops.lw_item_elems()
    rng = np.random.default_rng(3)
    last = np.float32(WD.E_LAST)
    around = np.float32([last, np.nextafter(last, np.float32(0)), np.nextafter(last, np.float32(np.inf))])
    planted = {
        "nan": np.float32([np.nan, np.inf, -np.inf, 1e30, -1e30]),
        "inf_both": np.float32([np.inf, -np.inf, 1e30]),
        "inf_up": np.float32([np.inf, 1e30]),
        "inf_down": np.float32([-np.inf, -1e30]),
        "big": np.concatenate([np.float32([1e30, -1e30, 3e38]), around, -around]),
        "only_nan": np.float32([np.nan]),
    }
    arrays = []
    for k, (name, p) in enumerate(planted.items()):
        a = _draw(rng, (W + 9, 50, 3 * W, 7, W, 1)[k])
        a[rng.choice(a.size, p.size, replace=False)] = p
        arrays.append(a)
    hist, parts = _run(dev, *_layout(arrays))
    for t, (name, a) in enumerate(zip(planted, arrays)):
        want = WD.counts_of(a)
        assert np.array_equal(hist[t, :ops.TBBIN_BINS], want), name
        assert hist[t, ops.TBBIN_NOBIN] == a.size - want.sum(), name
        got = _stats(parts[t])
        _check_stats(got, a, name)
    v = {name: _stats(parts[t]) for t, name in enumerate(planted)}
    assert v["nan"]["min"] != v["nan"]["min"] and v["nan"]["sum"] != v["nan"]["sum"]
    assert v["inf_both"]["min"] == -np.inf and v["inf_both"]["max"] == np.inf and v["inf_both"]["sum"] != v["inf_both"]["sum"]
    assert v["inf_up"]["sum"] == np.inf and v["inf_up"]["sum_squares"] == np.inf and v["inf_down"]["sum"] == -np.inf
    # float32(e_last) rounds below the edge: of the three floats around it only the upper one lies outside, on either side
    assert np.isfinite(v["big"]["sum_squares"]) and hist[4, ops.TBBIN_NOBIN] == 3 + 1 + 1
    assert hist[5, :ops.TBBIN_BINS].sum() == 0 and hist[5, ops.TBBIN_NOBIN] == 1
    with pytest.raises(ValueError):  # a histogram without a counted value, as upstream
        __import__("sota_imagenet_amd.callbacks", fromlist=["tb_trim"]).tb_trim(hist[5, :ops.TBBIN_BINS], WD.EDGES)


# ---- 4. all-equal arrays -------------------------------------------------------------------------------------------------------------------------------
def test_all_equal_arrays(dev):
    """W + 7 copies of 1.0 and of -1.0 (every lane of every wave on one bin: the single add of a wave), at an aligned and at an odd offset, and one
    with a single other value inside a wave"""
    ops, _ = _ops()
    n = ops.lw_item_elems() + 7
    one, minus = np.full(n, 1.0, dtype=np.float32), np.full(n, -1.0, dtype=np.float32)
    mixed = one.copy()
    mixed[777] = -2.5e-3
    arrays = [one, minus, one, mixed]
    flat, recs = _layout(arrays, [0, n + 5, 2 * n + 12 + 3, 3 * n + 24 + 2])
    hist, parts = _run(dev, flat, recs)
    for t, a in enumerate(arrays):
        want = WD.counts_of(a)
        assert np.array_equal(hist[t, :ops.TBBIN_BINS], want) and hist[t, ops.TBBIN_NOBIN] == 0, t
        assert (want > 0).sum() == (2 if t == 3 else 1)
        got = _stats(parts[t])
        _check_stats(got, a, f"all-equal {t}")
    assert _stats(parts[0])["sum"] == n and _stats(parts[1])["sum"] == -n and _stats(parts[1])["sum_squares"] == n  # integers: exact in any order


# ---- 5. argument checks --------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_foreign_records(dev):
    ops, item_plan = _ops()
    rng = np.random.default_rng(5)
    x = _draw(rng, 1000)
    src = torch.from_numpy(x).to(dev)
    edges = torch.from_numpy(WD.EDGES[775:].copy()).to(dev)
    items = item_plan.pack_records([(0, 1000, 0)], dev)
    hist = torch.zeros(2, ops.TBBIN_ROW, dtype=torch.int32, device=dev)
    partial = torch.full((8, ops.TBBIN_STATS), 7.0, dtype=torch.float64, device=dev)
    L = __import__("sota_imagenet_amd.native", fromlist=["lib"]).lib()
    good = [src.data_ptr(), 1000, items.data_ptr(), 1, 2, edges.data_ptr(), 774, hist.data_ptr(), partial.data_ptr(), None]

    def call(**kw):
        names = ["src", "n", "items", "n_items", "n_tensors", "edges", "n_edges", "hist", "partial", "stream"]
        return L.mi355_tbbin_hist(*[kw.get(k, v) for k, v in zip(names, good)])

    for k in ("src", "items", "edges", "hist", "partial"):
        assert call(**{k: None}) == -1, k
    assert call(src=src.data_ptr() + 4) == -1 and call(items=items.data_ptr() + 8) == -1 and call(hist=hist.data_ptr() + 8) == -1
    assert call(edges=edges.data_ptr() + 4) == -1 and call(partial=partial.data_ptr() + 4) == -1
    assert call(n_edges=773) == -1 and call(n_edges=775) == -1 and call(n_edges=1549) == -1
    assert call(n_items=0) == -1 and call(n_tensors=0) == -1
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0 and bool((partial == 7.0).all())
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.tbbin_hist(src[1:], items, hist, partial[:1])
    with pytest.raises(ValueError):
        ops.tbbin_hist(src, items[:0], hist, partial[:0])
    with pytest.raises(ValueError):
        ops.tbbin_hist(src, items, hist[:, :1548].contiguous(), partial[:1])
    with pytest.raises(ValueError):
        ops.tbbin_hist(src, items, hist, partial[:2])
    with pytest.raises(ValueError):
        ops.tbbin_hist(src.double(), items, hist, partial[:1])
    with pytest.raises(ValueError):
        ops.tbbin_hist(src.cpu(), items, hist, partial[:1])
    # records reaching past n, before 0, longer than an item or of a tensor outside the table are skipped: their entries stay as they were
    bad = [(990, 11, 1), (-4, 8, 1), (0, ops.lw_item_elems() + 1, 1), (1 << 40, 4, 1), (0, 0, 1), (0, 16, 2), (0, 16, -1)]
    table = item_plan.pack_records([(0, 1000, 0)] + bad, dev)
    hist.fill_(3)
    ops.tbbin_hist(src, table, hist, partial)
    got, p = hist.cpu().numpy().astype(np.int64), partial.cpu().numpy()
    assert np.array_equal(got[0, :ops.TBBIN_BINS], 3 + WD.counts_of(x)) and (got[1] == 3).all() and (got[0, ops.TBBIN_BINS:] == 3).all()
    assert (p[1:] == 7.0).all() and p[0, 0] == x.min() and p[0, 1] == x.max() and p[0, 4] == 0
    assert np.array_equal(src.cpu().numpy(), x)


# ---- 6. the callback -----------------------------------------------------------------------------------------------------------------------------------
def _compare(cb, logger, host, step):
    """`last` and the logger's calls against the restatement applied to the host copies"""
    assert list(cb.last) == ["model/" + n for n in host] and [c["tag"] for c in logger.calls] == list(cb.last)
    for call in logger.calls:
        v = host[call["tag"][len("model/"):]]
        want = WD.histogram(v)
        d = cb.last[call["tag"]]
        assert d["bucket_limits"] == want["bucket_limits"] and d["bucket_counts"] == want["bucket_counts"], call["tag"]
        assert d["num"] == want["num"] == v.size and call["step"] == step
        assert WD.same(d["min"], want["min"]) and WD.same(d["max"], want["max"]), call["tag"]
        v64 = v.astype(np.float64).ravel()
        for key, mass in (("sum", np.abs(v64).sum()), ("sum_squares", (v64 * v64).sum())):
            if np.isfinite(want[key]):
                assert abs(d[key] - want[key]) <= 2 * (v.size - 1) * U * mass, (call["tag"], key)
            else:
                assert WD.same(d[key], want[key]), (call["tag"], key)
        assert all(WD.same(call[k], d[k]) for k in ("min", "max", "num", "sum", "sum_squares"))
        assert call["bucket_limits"] == d["bucket_limits"] and call["bucket_counts"] == d["bucket_counts"]


def _state(model, step=19200):
    from sota_imagenet_amd.fit_wrapper import RunnerState

    st = RunnerState(model=model)
    st.global_sample_step, st.tb_logger = step, WD.Capture()
    return st


def _same_last(a, b):
    return list(a) == list(b) and all(
        np.array([a[t][k] for k in ("min", "max", "sum", "sum_squares")]).tobytes() == np.array([b[t][k] for k in ("min", "max", "sum", "sum_squares")]).tobytes()
        and a[t]["bucket_counts"] == b[t]["bucket_counts"] and a[t]["bucket_limits"] == b[t]["bucket_limits"] for t in a)


def test_callback_on_a_hand_made_module(dev):
    """every route of the plan in one small module: fp32 tensors of storages of their own, two views of one storage at odd offsets with NaN between
    them, an fp32 view with gaps (not dense: the host rule), int64 counters that are views of one array, a bf16 buffer, a tensor that holds a NaN"""
    from sota_imagenet_amd import callbacks

    rng = np.random.default_rng(6)
    m = torch.nn.Module()
    m.w = torch.nn.Parameter(torch.from_numpy(_draw(rng, 5000).reshape(50, 100)).to(dev))
    shared = torch.full((3000,), NAN, device=dev)
    shared[5:5 + 1001] = torch.from_numpy(_draw(rng, 1001)).to(dev)
    shared[1011:1011 + 77] = torch.from_numpy(_draw(rng, 77)).to(dev)
    m.register_buffer("a", shared[5:5 + 1001])
    m.register_buffer("b", shared[1011:1011 + 77].view(7, 11))
    strided = torch.from_numpy(_draw(rng, 64)).to(dev)
    m.register_buffer("gaps", strided[::2])
    nbt = torch.tensor([0, 3, 5004, 17], dtype=torch.int64, device=dev)
    m.register_buffer("n0", nbt[0])
    m.register_buffer("n2", nbt[2])
    m.register_buffer("n3", nbt[3])
    m.register_buffer("bf", torch.from_numpy(_draw(rng, 33)).to(dev).to(torch.bfloat16))
    with_nan = torch.from_numpy(_draw(rng, 300)).to(dev)
    with_nan[17] = NAN
    m.register_buffer("bad", with_nan)
    cb = callbacks.WeightDistributionTB()
    st = _state(m, 640)
    cb.set_state(st)
    cb.on_epoch_begin()
    host = {n: t.detach().float().cpu().numpy() if t.dtype == torch.bfloat16 else t.detach().cpu().numpy() for n, t in m.state_dict().items()}
    assert list(host) == ["w", "a", "b", "gaps", "n0", "n2", "n3", "bf", "bad"]
    _compare(cb, st.tb_logger, host, 640)
    assert len(cb._plan.rows) == 4 and len(cb._plan.launches) == 3  # w, a + b, bad; the other five by the host rule
    assert cb.last["model/n2"]["min"] == 5004.0 and cb.last["model/bad"]["min"] != cb.last["model/bad"]["min"]
    with torch.no_grad():
        m.bad.fill_(NAN)
    with pytest.raises(ValueError, match="bad"):  # no counted value: add_histogram raises too
        cb.on_epoch_begin()
    with pytest.raises(NotImplementedError, match="no CPU path"):
        cpu = callbacks.WeightDistributionTB()
        cpu.set_state(_state(torch.nn.Linear(2, 2)))
        cpu.on_epoch_begin()


def _seeded_flat_model(m, seed):
    """parameters and running statistics from a seeded generator, NaN in everything that no tensor covers (alignment gaps, the FC padding rows),
    the counters distinct integers"""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for flat, tensors in ((m._flat_params, list(m.parameters())), (m._flat_buffers, [b for b in m.buffers() if b.dtype == torch.float32])):
            h = np.full(flat.numel(), NAN, dtype=np.float32)
            for t in tensors:
                off = (t.data_ptr() - flat.data_ptr()) // 4
                assert 0 <= off and off + t.numel() <= flat.numel()
                h[off: off + t.numel()] = rng.normal(size=t.numel()).astype(np.float32) * np.float32(10.0 ** rng.uniform(-4, 0))
            flat.copy_(torch.from_numpy(h).to(flat.device))
        m._nbt.copy_(torch.arange(5000, 5000 + m._nbt.numel(), device=m._nbt.device))


def _callback_on(m, dev):
    from sota_imagenet_amd import callbacks

    _seeded_flat_model(m, 7)
    names = list(m.state_dict())
    cb = callbacks.WeightDistributionTB()
    st = _state(m)
    cb.set_state(st)
    cb.on_epoch_begin()
    host = {n: t.detach().cpu().numpy() for n, t in m.state_dict().items()}
    assert list(host) == names and cb.logged == 1
    _compare(cb, st.tb_logger, host, 19200)
    assert sum(d["num"] for d in cb.last.values()) == sum(v.size for v in host.values())
    first, plan, calls = cb.last, cb._plan, len(st.tb_logger.calls)
    cb.on_epoch_begin()
    assert cb._plan is plan and cb.logged == 2 and cb.last is not first and _same_last(first, cb.last)  # the plan was built once
    st.rank = 1
    cb.on_epoch_begin()
    assert cb.logged == 2 and len(st.tb_logger.calls) == 2 * calls  # rank 1 logs nothing
    return cb, names


def test_callback_on_resnet50(dev):
    from sota_imagenet_amd.models import resnet50

    cb, names = _callback_on(resnet50(dtype="fp32").cuda(), dev)
    assert len(names) == 320 and sum(n.endswith("num_batches_tracked") for n in names) == 53
    assert len(cb._plan.launches) == 2 and len(cb._plan.rows) == 267 and len(cb._plan.gathers) == 1  # flat parameters, flat buffers; one gather
    assert cb.last["model/" + [n for n in names if n.endswith("num_batches_tracked")][1]]["min"] == 5001.0


# ---- 7. BResNet-50 -------------------------------------------------------------------------------------------------------------------------------------
def test_callback_on_bresnet50(dev):
    from sota_imagenet_amd.bresnet import BResNet50

    cb, names = _callback_on(BResNet50(dtype="fp32").cuda(), dev)
    assert len(cb._plan.rows) + len(cb._plan.where) == len(names) and len(cb._plan.rows) >= 161


# ---- 8. train.py ---------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_logs_the_weight_histograms(dev, tmp_path, monkeypatch):
    """nov_hist_test.yaml through train.py: log.histogram puts the callback into the list, both debug epochs run and log, and `last` holds one tag
    per state_dict entry whose num values add up to the model's element count"""
    sys.path.insert(0, ROOT)
    import train
    from sota_imagenet_amd import callbacks

    made = []
    init = callbacks.WeightDistributionTB.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    monkeypatch.setattr(callbacks.WeightDistributionTB, "__init__", spy)
    logdir = os.path.relpath(str(tmp_path), ROOT)
    val_loss, metrics = train.main(["+hydra_exp=nov_hist_test", f"log.dir={logdir}", "random_seed=0", "data.pool=2"])
    assert val_loss == val_loss and 0.0 <= metrics["Acc@1"].avg <= 100.0
    assert len(made) == 1 and made[0].logged == 2
    sd = made[0].state.model.state_dict()
    assert list(made[0].last) == ["model/" + n for n in sd] and len(sd) == 320
    assert sum(d["num"] for d in made[0].last.values()) == sum(t.numel() for t in sd.values())
    assert all(len(d["bucket_limits"]) == len(d["bucket_counts"]) >= 2 and sum(d["bucket_counts"]) <= d["num"] for d in made[0].last.values())
