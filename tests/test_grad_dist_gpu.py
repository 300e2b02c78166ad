"""GradDistributionTB on the MI355X: the two kernels of csrc/optim_hist.hip against numpy (np.bincount over the bins of grad_dist_common, the
counting formula), the fixture recorded from the reference's own callback, the callback on the flat ResNet-50 under AdamW and NovogradApex, and
recipe 46's complete smoke config through train.py.  Every comparison is on exact integers."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import flat_layout  # noqa: E402
import grad_dist_common as G  # noqa: E402
from flat_layout import _ops  # noqa: E402
from optim_harness import NAN, grads_for  # noqa: E402

pytestmark = pytest.mark.gpu
GAP = 7.0e3  # fills everything between the records; no record below holds a value of its bin, which must stay empty


def _draw(rng, n):
    """u uniform over [-18, 2], so nothing reaches GAP's bin"""
    return flat_layout._draw(rng, n, -18.0, 2.0)


def _layout(arrays, offsets=None, fill=GAP, tail=9):
    return flat_layout._layout(arrays, offsets, fill, tail)


def _hist_of(dev, flat, recs, hist=None, index=None, n_tensors=None):
    ops, item_plan = _ops()
    items, _ = item_plan.plan_items(recs, ops.lw_item_elems(), index)
    if hist is None:
        hist = torch.zeros(n_tensors or len(recs), 512, dtype=torch.int32, device=dev)
    ops.absbin_hist(torch.from_numpy(flat).to(dev), item_plan.pack_records(items, dev), hist)
    return hist


def _gap_bin():
    return int(G.bin_of(np.float32([GAP]))[0])


# ---- 1. absbin_hist ------------------------------------------------------------------------------------------------------------------------------------
def test_hist_sizes_around_the_item_and_gaps(dev):
    """1, 4095, 4096, 4097 and 3*4096 + 5 elements — below, at and above one work item, tails that are no multiple of 4, more than one workgroup
    per tensor — with the gaps between them holding a value whose bin no record uses"""
    rng = np.random.default_rng(1)
    arrays = [_draw(rng, n) for n in (1, 4095, 4096, 4097, 3 * 4096 + 5)]
    assert _ops()[0].lw_item_elems() == 4096
    flat, recs = _layout(arrays)
    got = _hist_of(dev, flat, recs).cpu().numpy()
    want = np.stack([G.hist(a) for a in arrays])
    assert np.array_equal(got, want)
    assert got[:, _gap_bin()].sum() == 0 and want.sum() == sum(a.size for a in arrays)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_hist_odd_element_offsets(dev, shift):
    """tensors that start 1, 2 and 3 elements behind a 16-byte boundary: the scalar head, the vector body and the tail, and tensors shorter than the
    head"""
    rng = np.random.default_rng(10 + shift)
    sizes = (1, 2, 3, 5, 259, 4096, 4099, 2 * 4096 + 2)
    arrays = [_draw(rng, n) for n in sizes]
    offsets, end = [], 0
    for n in sizes:
        off = (end + 4 + 3) // 4 * 4 + shift
        offsets.append(off)
        end = off + n
    flat, recs = _layout(arrays, offsets)
    got = _hist_of(dev, flat, recs).cpu().numpy()
    assert np.array_equal(got, np.stack([G.hist(a) for a in arrays])) and got[:, _gap_bin()].sum() == 0


def test_hist_all_equal_full_contention(dev):
    """3 * 4096 equal values (every lane of every wave on one bin), at an aligned and at an odd offset, and one with a single other value inside"""
    a = np.full(3 * 4096, -3.7e-4, dtype=np.float32)
    b = a.copy()
    b[5000] = 2.0
    flat, recs = _layout([a, a, b], [0, 3 * 4096 + 7, 6 * 4096 + 16])
    got = _hist_of(dev, flat, recs).cpu().numpy()
    k, k2 = int(G.bin_of(a[:1])[0]), int(G.bin_of(np.float32([2.0]))[0])
    want = np.zeros((3, 512), dtype=np.int64)
    want[:, k] = 3 * 4096
    want[2, k], want[2, k2] = 3 * 4096 - 1, 1
    assert np.array_equal(got, want)


def test_hist_every_bin_and_the_special_values(dev):
    e = G.edges()
    per_bin = np.concatenate([[e[0] / 2], (e[:-1].astype(np.float64) + e[1:]) / 2, [e[-1] * 2]]).astype(np.float32)  # one value inside each bin
    assert np.array_equal(G.bin_of(per_bin), np.arange(512))
    special = np.float32([0.0, -0.0, 1e-40, -1e-42, -1.0, -1e-17, -3e3, np.inf, -np.inf, np.nan, 3.4e38, -e[7], e[300]])
    x = np.concatenate([per_bin * np.where(np.arange(512) % 2, -1, 1).astype(np.float32), special])
    got = _hist_of(dev, *_layout([x], fill=0.0))[0].cpu().numpy()
    want = G.hist(x)
    assert np.array_equal(got, want) and want[0] == 1 + 5 and want[511] == 1 + 4 and (want >= 1).all()


def test_hist_skips_records_outside_the_array_and_adds(dev):
    """records reaching past n, before 0, longer than an item or of a tensor outside the table are skipped: their rows stay as they were; a second
    launch ADDS"""
    ops, item_plan = _ops()
    rng = np.random.default_rng(3)
    x = _draw(rng, 1000)
    src = torch.from_numpy(x).to(dev)
    bad = [(990, 11, 1), (-4, 8, 1), (0, 4097, 1), (1 << 40, 4, 1), (0, 0, 1), (0, 16, 2), (0, 16, -1)]
    items = item_plan.pack_records([(0, 1000, 0)] + bad, dev)
    hist = torch.full((2, 512), 7, dtype=torch.int32, device=dev)
    ops.absbin_hist(src, items, hist)
    got = hist.cpu().numpy()
    assert np.array_equal(got[0], 7 + G.hist(x)) and (got[1] == 7).all()
    ops.absbin_hist(src, items, hist)
    assert np.array_equal(hist.cpu().numpy()[0], 7 + 2 * G.hist(x))
    assert np.array_equal(src.cpu().numpy(), x)


def test_hist_two_storages_fill_one_table(dev):
    rng = np.random.default_rng(4)
    a, b, c = _draw(rng, 5000), _draw(rng, 77), _draw(rng, 4097)
    flat1, recs1 = _layout([a, c])
    flat2, recs2 = _layout([b], [3])
    hist = _hist_of(dev, flat1, recs1, index=[0, 2], n_tensors=3)
    _hist_of(dev, flat2, recs2, hist=hist, index=[1])
    assert np.array_equal(hist.cpu().numpy(), np.stack([G.hist(a), G.hist(b), G.hist(c)]))


def test_hist_error_returns(dev):
    ops, item_plan = _ops()
    src = torch.zeros(64, device=dev)
    items = item_plan.pack_records([(0, 64, 0)], dev)
    hist = torch.zeros(1, 512, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.absbin_hist(src[1:], items, hist)
    with pytest.raises(RuntimeError, match="misaligned"):
        ops.absbin_hist(src, items, torch.zeros(513, dtype=torch.int32, device=dev)[1:].view(1, 512))
    with pytest.raises(ValueError):
        ops.absbin_hist(src, items[:0], hist)
    with pytest.raises(ValueError):
        ops.absbin_hist(src, items, torch.zeros(1, 511, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.absbin_hist(src, items, hist.long())
    with pytest.raises(ValueError):
        ops.absbin_hist(src.double(), items, hist)
    with pytest.raises(ValueError):
        ops.absbin_hist(src.cpu(), items, hist)
    L = __import__("sota_imagenet_amd.native", fromlist=["lib"]).lib()
    assert L.mi355_absbin_hist(None, 64, items.data_ptr(), 1, 1, hist.data_ptr(), None) == -1
    assert L.mi355_absbin_hist(src.data_ptr(), 64, items.data_ptr(), 0, 1, hist.data_ptr(), None) == -1
    assert L.mi355_absbin_hist(src.data_ptr(), 64, items.data_ptr(), 1, 0, hist.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0


# ---- 2. subsample_counts -------------------------------------------------------------------------------------------------------------------------------
def _counts(dev, hists, rep, s):
    ops, _ = _ops()
    counts = torch.full((512,), -5, dtype=torch.int64, device=dev)
    ops.subsample_counts(torch.from_numpy(np.asarray(hists, dtype=np.int32)).to(dev), torch.tensor(rep, dtype=torch.int32, device=dev), s, counts,
                         rep_host=rep)
    return counts.cpu().numpy()


@pytest.mark.parametrize("n_tensors", [1, 8, 9, 161])
def test_subsample_counts_against_the_formula(dev, n_tensors):
    """s = 1, 3, 10 and larger than every tensor; one tensor, as many as there are waves, one more, and as many as ResNet-50 has; rep > 1"""
    rng = np.random.default_rng(n_tensors)
    hists = np.zeros((n_tensors, 512), dtype=np.int64)
    for t in range(n_tensors):
        k = rng.integers(0, 512, int(rng.integers(1, 40)))
        hists[t, k] = rng.integers(1, 5000, len(k))
    hists[0, :] = 0
    hists[0, [0, 511]] = [3, 1]  # the first and the last bin
    ones = [1] * n_tensors
    rep = [int(r) for r in rng.choice([1, 1, 9, 64, 2359296], n_tensors)]
    for s in (1, 3, 10, int(hists.sum(axis=1).max()) * 3):
        assert np.array_equal(_counts(dev, hists, ones, s), G.formula(hists, s)), s
        got = _counts(dev, hists, rep, s)
        assert np.array_equal(got, G.formula(hists, s, rep)), s
        assert got.sum() == G.kept_total(hists.sum(axis=1) * np.asarray(rep), s)


def test_subsample_counts_beyond_32_bits(dev):
    """counts of a tensor near 2^31 elements with rep near 2^31: the products and sums are 64-bit"""
    hists = np.zeros((2, 512), dtype=np.int64)
    hists[0, [5, 200]] = [2 ** 31 - 1, 1]
    hists[1, 100] = 2 ** 30
    rep = [1, 2 ** 31 - 1]
    for s in (1, 7):
        assert np.array_equal(_counts(dev, hists, rep, s), G.formula(hists, s, rep))


def test_subsample_counts_error_returns(dev):
    ops, _ = _ops()
    hist = torch.zeros(2, 512, dtype=torch.int32, device=dev)
    hist[:, 9] = 4
    rep = torch.ones(2, dtype=torch.int32, device=dev)
    counts = torch.zeros(512, dtype=torch.int64, device=dev)
    for s in (0, -3):
        with pytest.raises(RuntimeError, match="subsample"):
            ops.subsample_counts(hist, rep, s, counts)
    with pytest.raises(ValueError, match="rep"):
        ops.subsample_counts(hist, rep, 3, counts, rep_host=[1, 0])
    with pytest.raises(ValueError):
        ops.subsample_counts(hist, rep[:1], 3, counts)
    with pytest.raises(ValueError):
        ops.subsample_counts(hist, rep, 3, counts[:511])
    with pytest.raises(ValueError):
        ops.subsample_counts(hist.long(), rep, 3, counts)
    assert int(counts.sum()) == 0
    # rep lives on the device: a multiplicity below 1 that the host never saw makes every count the impossible value
    ops.subsample_counts(hist, torch.tensor([1, 0], dtype=torch.int32, device=dev), 3, counts)
    assert (counts.cpu().numpy().astype(np.uint64) == ops.ABSBIN_BAD_REP).all()
    ops.subsample_counts(hist, rep, 3, counts)
    assert counts.cpu().numpy()[9] == 2 and int(counts.sum()) == 2  # ceil((ceil(4/3) + ceil(4/3)) / 3) = ceil(4 / 3)


# ---- 3. the fixture on the device ----------------------------------------------------------------------------------------------------------------------
def test_fixture_counts_equal_the_reference_recorded_bins(dev):
    """the reference's own callback, recorded on the CPU (tests/golden/grad_dist_ref.npz): the device's counts are the bin counts of what it handed
    to add_histogram, for every tag and subsample"""
    ops, _ = _ops()
    fx = G.Fixture()
    for tag in G.TAGS:
        arrays = fx.inputs[tag]
        offsets, end = [], 0
        for i, a in enumerate(arrays):  # every other tensor at an odd offset
            off = (end + 4 + 3) // 4 * 4 + (i % 4)
            offsets.append(off)
            end = off + a.size
        hist = _hist_of(dev, *_layout(arrays, offsets, fill=NAN))
        assert np.array_equal(hist.cpu().numpy(), np.stack([G.hist(a) for a in arrays]))
        rep = torch.ones(len(arrays), dtype=torch.int32, device=dev)
        for s in G.SUBSAMPLES:
            counts = torch.zeros(512, dtype=torch.int64, device=dev)
            ops.subsample_counts(hist, rep, s, counts)
            want = np.bincount(G.bin_of_log(fx.recorded[(tag, s)]), minlength=512)
            assert np.array_equal(counts.cpu().numpy(), want), (tag, s)


# ---- 4. the callback -----------------------------------------------------------------------------------------------------------------------------------
class _Capture:
    def __init__(self):
        self.calls = []

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None):
        self.calls.append(dict(tag=tag, min=min, max=max, num=num, sum=sum, sum_squares=sum_squares, limits=bucket_limits, counts=bucket_counts,
                               step=global_step))


CASES = {
    "adamw": ("AdamW", dict(lr=1e-3, weight_decay=2e-2)),
    "nov": ("NovogradApex", dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01)),
    "nov_unit": ("NovogradApex", dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.002, wd_eps=0.01, unitwise_norm=True)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_callback_on_resnet50(dev, case):
    """models.resnet50 (flat arrays) after one optimizer step on synthetic gradients (NaN in the padding, which must not be counted): the tags and
    the step are the reference's, the counts are the formula applied to host copies of the same arrays, num is exact, and a second call repeats
    the counts bit for bit.  NovogradApex shows exp_avg_sq broadcast from one value per tensor (or per output unit)"""
    from sota_imagenet_amd import callbacks, optim
    from sota_imagenet_amd.fit_wrapper import RunnerState
    from sota_imagenet_amd.models import resnet50

    cls, kw = CASES[case]
    m = resnet50(dtype="fp32").cuda()
    opt = getattr(optim, cls)([{"params": list(m.parameters())}], **kw)
    opt.attach_model(m)
    m.flat_grads.copy_(grads_for(m, 3))
    opt.zero_grad()
    opt.step()
    s = 10
    cb = callbacks.GradDistributionTB(log_every=50, subsample=s)
    st = RunnerState(model=m, optimizer=opt)
    st.step, st.is_train, st.global_sample_step, st.tb_logger = 100, True, 19200, _Capture()
    cb.set_state(st)
    cb.on_batch_end()
    assert cb.logged == 1 and list(cb.last) == list(G.TAGS) and [c["tag"] for c in st.tb_logger.calls] == list(G.TAGS)
    host = {"optim/exp_avg_log": [v["exp_avg"].cpu().numpy() for v in opt.state.values()],
            "optim/exp_avg_sq_log": [v["exp_avg_sq"].cpu().numpy() for v in opt.state.values()],
            "optim/model_params_log": [p.detach().cpu().numpy() for p in m.parameters()]}
    sq = [v["exp_avg_sq"] for v in opt.state.values()]
    reps = [(_ops()[1].hist_records(t)[3], t.numel(), t.shape[0] if t.dim() > 1 else 1) for t in sq]
    if case == "adamw":  # dense views
        assert all(rep == 1 for rep, n, rows in reps)
    elif case == "nov":  # one stored value per tensor
        assert all(rep == n for rep, n, rows in reps) and any(n > 1 for rep, n, rows in reps)
    else:  # one stored value per output unit of the tensors with more than one dimension
        assert all(rep == n // rows for rep, n, rows in reps) and any(1 < rep < n for rep, n, rows in reps)
    limits = _ops()[0].absbin_log10_limits()
    for call in st.tb_logger.calls:
        tag = call["tag"]
        want = G.formula([G.hist_fast(a) for a in host[tag]], s)
        limits_got, counts = cb.last[tag]
        assert np.array_equal(counts, want), tag
        assert call["counts"] == want.tolist() and call["limits"] == limits.tolist() and np.array_equal(limits_got, limits)
        assert call["step"] == 19200 and call["num"] == int(want.sum()) == G.kept_total([a.size for a in host[tag]], s)
        nz = np.nonzero(want)[0]
        assert call["min"] == (-15.0 if nz[0] == 0 else limits[nz[0] - 1]) and call["max"] == limits[nz[-1]]
        assert want[511] == 0  # no NaN of the padding was counted
    first = {tag: c.copy() for tag, (_, c) in cb.last.items()}
    plan = cb._tags
    cb.on_batch_end()
    assert cb._tags is plan and cb.logged == 2  # the plan was built once
    assert all(np.array_equal(first[tag], cb.last[tag][1]) for tag in G.TAGS)
    st.step = 101
    cb.on_batch_end()
    st.step, st.is_train = 150, False
    cb.on_batch_end()
    assert cb.logged == 2


def test_train_py_runs_recipe_46_complete(dev, tmp_path, monkeypatch):
    """nov_full_test.yaml through train.py: OrthoInitClb and GradDistributionTB from the config, the histograms taken every 5th of the 10 debug steps
    of both epochs, and `last` holds the three tags with the exact number of kept values"""
    sys.path.insert(0, ROOT)
    import train
    from sota_imagenet_amd import callbacks

    made = []
    init = callbacks.GradDistributionTB.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    monkeypatch.setattr(callbacks.GradDistributionTB, "__init__", spy)
    logdir = os.path.relpath(str(tmp_path), ROOT)
    val_loss, metrics = train.main(["+hydra_exp=nov_full_test", f"log.dir={logdir}", "random_seed=0", "data.pool=2"])
    assert val_loss == val_loss and 0.0 <= metrics["Acc@1"].avg <= 100.0
    assert len(made) == 1 and made[0].log_every == 5 and made[0].logged == 4
    assert list(made[0].last) == list(G.TAGS)
    numels = [p.numel() for p in made[0].state.model.parameters()]
    for tag in G.TAGS:
        limits, counts = made[0].last[tag]
        assert counts.sum() == G.kept_total(numels, 10) and counts[511] == 0 and len(limits) == 512
