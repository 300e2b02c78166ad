"""GradDistributionTB without a GPU: the bins (Python, the kernels' header and the powers of two of grad_dist_common agree), the counting formula
against the sorts it replaces, the fixture recorded from the reference's own callback against the formula, item_plan.hist_records, the alias, the two
new configs and the callback's gates."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import grad_dist_common as G  # noqa: E402
from sota_imagenet_amd import callbacks, config as C, item_plan, ops  # noqa: E402
from sota_imagenet_amd.fit_wrapper import RunnerState  # noqa: E402


# ---- the bins ----------------------------------------------------------------------------------------------------------------------------------------
def _bits(k):
    return np.array([k << ops.ABSBIN_SHIFT], dtype=np.uint32).view(np.float32)[0]


def test_k0_is_the_smallest_edge_above_the_reference_clamp():
    assert ops.ABSBIN_K0 == (77 << 3) + 2 == 618 and ops.ABSBIN_BINS == 512 and ops.ABSBIN_SHIFT == 20
    assert _bits(ops.ABSBIN_K0) > 1e-15 >= _bits(ops.ABSBIN_K0 - 1)
    assert _bits(ops.ABSBIN_K0) == np.float32(2.0 ** -50 * 1.25)
    assert _bits(ops.ABSBIN_K0 + 511) == np.float32(2.0 ** 14 * 1.125)


def test_edges_increase_and_agree_with_the_powers_of_two():
    e = ops.absbin_edges()
    assert e.dtype == np.float32 and e.shape == (511,) and (np.diff(e) > 0).all() and np.isfinite(e).all()
    assert np.array_equal(e, G.edges())
    lim = ops.absbin_log10_limits()
    assert lim.dtype == np.float64 and lim.shape == (512,) and (np.diff(lim) > 0).all() and lim[0] > -15
    assert np.array_equal(lim[:-1], np.log10(e.astype(np.float64)))


def test_python_and_header_constants_agree():
    text = open(os.path.join(ROOT, "sota_imagenet_amd", "csrc", "absbin.h")).read()
    vals = {k: eval(v, {}) for k, v in re.findall(r"constexpr int (kAbsBin\w+) = ([^;]+);", text)}  # noqa: S307 (integer expressions of our own header)
    assert vals == {"kAbsBinBins": ops.ABSBIN_BINS, "kAbsBinShift": ops.ABSBIN_SHIFT, "kAbsBinK0": ops.ABSBIN_K0}


def test_the_bit_rule_is_the_edge_rule():
    """bin = clamp((bits without sign >> 20) - K0, 0, 511), restated on uint32, against searchsorted over the edges — at the edges themselves, one
    ulp either side of them, and for zeros, -0.0, denormals, infinities and NaN"""
    e = ops.absbin_edges()
    x = np.concatenate([e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(np.inf)), -e,
                        np.array([0.0, -0.0, 1e-40, -1e-45, 1e-15, 1.2e-15, np.inf, -np.inf, np.nan, 3e38, 1.0, -2.5], dtype=np.float32)])
    key = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    by_bits = np.clip((key >> ops.ABSBIN_SHIFT).astype(np.int64) - ops.ABSBIN_K0, 0, 511)
    assert np.array_equal(by_bits, G.bin_of(x))
    assert G.bin_of(np.float32([0.0, -0.0, 1e-40, 1e-15, np.inf, np.nan])).tolist() == [0, 0, 0, 0, 511, 511]
    assert np.array_equal(G.hist_fast(x), G.hist(x))


# ---- the counting formula ----------------------------------------------------------------------------------------------------------------------------
def _random_tensors(rng, n_tensors, max_numel, ties):
    out = []
    for _ in range(n_tensors):
        n = int(rng.integers(1, max_numel + 1))
        x = (10.0 ** rng.uniform(-18.0, 4.0, n)).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)
        if ties:
            x = rng.choice(x[: max(1, n // 7)], n)
        x[rng.uniform(size=n) < 0.1] = 0.0
        out.append(x)
    return out


@pytest.mark.parametrize("s", [1, 2, 3, 7, 10, 5000])
@pytest.mark.parametrize("ties", [False, True])
def test_sort_route_equals_formula(s, ties):
    rng = np.random.default_rng(100 * s + ties)
    for trial in range(4):
        ts = _random_tensors(rng, int(rng.integers(1, 9)), 3000, ties) + [np.float32([0.5]), np.zeros(3, np.float32)]
        got, want = G.formula_of(ts, s), G.sort_route(ts, s)
        assert np.array_equal(got, want), (s, ties, trial)
        assert got.sum() == G.kept_total([t.size for t in ts], s)


def test_formula_with_rep_counts_a_broadcast_state():
    rng = np.random.default_rng(7)
    vals = (10.0 ** rng.uniform(-12, 2, 6)).astype(np.float32)
    shown = [np.full(n, v, dtype=np.float32) for n, v in zip([1, 9, 64, 147, 4097, 30], vals)]
    unit = (10.0 ** rng.uniform(-12, 2, 5)).astype(np.float32)
    shown.append(np.repeat(unit, 12))
    hists = [G.hist(v) for v in vals] + [G.hist(unit)]
    rep = [1, 9, 64, 147, 4097, 30, 12]
    for s in (1, 3, 10, 100):
        assert np.array_equal(G.formula(hists, s, rep), G.sort_route(shown, s))


def test_fixture_recorded_values_give_the_formula_counts():
    fx = G.Fixture()
    log_edges = np.log10(G.edges().astype(np.float64))
    for tag in G.TAGS:
        assert any(x.size < 10 for x in fx.inputs[tag]) and any(x.ndim == 0 for x in fx.inputs[tag])
        assert any(x.size > 1 and (x == x.ravel()[0]).all() for x in fx.inputs[tag]) and any((x == 0).any() for x in fx.inputs[tag])
        for s in G.SUBSAMPLES:
            v = fx.recorded[(tag, s)]
            assert v.dtype == np.float32 and v.min() >= -15 and len(v) == G.kept_total([x.size for x in fx.inputs[tag]], s)
            for chunk in np.array_split(v.astype(np.float64), 32):
                assert np.abs(chunk[:, None] - log_edges[None, :]).min() >= 1e-5
            assert np.array_equal(np.bincount(G.bin_of_log(v), minlength=G.NB), G.formula_of(fx.inputs[tag], s)), (tag, s)
    big = np.concatenate([np.abs(x).ravel() for x in fx.inputs[G.TAGS[2]]])
    assert big.max() > 1e2 and 0 < big[big > 0].min() < 1e-19 and (fx.recorded[(G.TAGS[2], 1)] == -15).any()


# ---- hist_records ------------------------------------------------------------------------------------------------------------------------------------
class _FakeCuda:
    """a CPU tensor that says it is on the device: hist_records reads addresses, shapes and strides only"""

    def __init__(self, t):
        self.t = t

    is_cuda = True

    def __getattr__(self, k):
        return getattr(self.t, k)


@pytest.fixture
def as_cuda(monkeypatch):
    monkeypatch.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, _FakeCuda)))
    return _FakeCuda


def test_hist_records_dense_broadcast_and_unit_views(as_cuda):
    flat = torch.zeros(1000)
    base = flat.untyped_storage().data_ptr()
    dense = torch.as_strided(flat, (4, 3, 2, 2), (12, 1, 6, 3), 5)  # a permuted dense view, as the flat models' OIHW views over KRSC memory
    assert item_plan.hist_records(as_cuda(dense)) == (base, 5, 48, 1)
    assert item_plan.hist_records(as_cuda(flat[7:8].reshape(()))) == (base, 7, 1, 1)
    assert item_plan.hist_records(as_cuda(torch.as_strided(flat, (4, 3, 2, 2), (0, 0, 0, 0), 9))) == (base, 9, 1, 48)
    assert item_plan.hist_records(as_cuda(torch.as_strided(flat, (64,), (0,), 11))) == (base, 11, 1, 64)
    assert item_plan.hist_records(as_cuda(torch.as_strided(flat, (6, 3, 2, 2), (1, 0, 0, 0), 20))) == (base, 20, 6, 12)
    assert item_plan.hist_records(as_cuda(torch.as_strided(flat, (6, 5), (1, 0), 3))) == (base, 3, 6, 5)
    assert item_plan.hist_records(as_cuda(torch.as_strided(flat, (1, 5), (77, 0), 3))) == (base, 3, 1, 5)  # a dimension of size 1 carries no stride
    from sota_imagenet_amd.optim import _unit_strides

    for shape in [(8, 4, 3, 3), (10, 7), (5,), ()]:
        n = int(np.prod(shape)) if shape else 1
        rec = item_plan.hist_records(as_cuda(torch.as_strided(flat, shape, _unit_strides(len(shape)), 0)))
        assert rec == ((base, 0, shape[0], n // shape[0]) if len(shape) > 1 else (base, 0, 1, n))


def test_hist_records_errors(as_cuda):
    flat = torch.zeros(1000)
    with pytest.raises(RuntimeError, match=r"\(4, 6\).*\(12, 2\)"):
        item_plan.hist_records(as_cuda(torch.as_strided(flat, (4, 6), (12, 2))))
    with pytest.raises(RuntimeError, match="strides"):
        item_plan.hist_records(as_cuda(torch.as_strided(flat, (4, 6), (0, 1))))
    with pytest.raises(RuntimeError, match="empty"):
        item_plan.hist_records(as_cuda(flat[:0]))
    with pytest.raises(NotImplementedError):
        item_plan.hist_records(flat)  # a CPU tensor
    with pytest.raises(NotImplementedError):
        item_plan.hist_records(as_cuda(flat.double()))
    with pytest.raises(NotImplementedError):
        item_plan.hist_records(0.5)


def test_dist_plan_gives_the_launches_build_plan_had_inline():
    """the grouping GradDistributionTB.build_plan spelled out before it took its launches from item_plan.dist_plan, restated on tuples: per
    storage, in order of first appearance, (lo, hi, items) and the packed table byte for byte.  W = 64; two storages interleaved in tensor order;
    first elements at 0, 1, 2, 3 mod 4; tensors of W, W + 1 and 1 element (a broadcast state); the lowest first element of storage A is no multiple
    of 4, so lo & ~3 matters"""
    W, A, B = 64, 0x7000, 0x9000
    rs = [(A, 6, W, 1), (B, 0, W + 1, 1), (A, 75, 1, 4608), (B, 69, 30, 1), (A, 80, 2 * W + 2, 1)]  # hist_records: (base, first, elements, rep)
    assert sorted(r[1] % 4 for r in rs[:4]) == [0, 1, 2, 3] and min(r[1] for r in rs if r[0] == A) % 4
    by_storage = {}  # storage base -> tensor indices, in order of first appearance
    for i, r in enumerate(rs):
        by_storage.setdefault(r[0], []).append(i)
    want = []
    for base, idx in by_storage.items():
        lo = min(rs[i][1] for i in idx) & ~3
        hi = max(rs[i][1] + rs[i][2] for i in idx)
        items, _ = item_plan.plan_items([(rs[i][1] - lo, rs[i][2]) for i in idx], W, idx)
        want.append((base, lo, hi, items))
    rows, launches, spans, n_items = item_plan.dist_plan([r[:3] for r in rs], W)
    assert rows == list(range(len(rs)))  # a row is the tensor's position in its tag
    assert [l[:4] for l in launches] == want and [b for b, *_ in want] == [A, B] and [w[1:3] for w in want] == [(4, 210), (0, 99)]
    assert want[0][3] == [(2, 64, 0), (71, 1, 2), (76, 64, 4), (140, 64, 4), (204, 2, 4)] and want[1][3] == [(0, 64, 1), (64, 1, 1), (69, 30, 3)]
    for (_, _, _, items, i0), (_, _, _, items_want) in zip(launches, want):
        assert torch.equal(item_plan.pack_records(items), item_plan.pack_records(items_want))
    assert n_items == 8 and [l[4] for l in launches] == [0, 5] and spans == [(0, 1), (5, 2), (1, 1), (7, 1), (2, 3)]


# ---- alias, configs, gates ---------------------------------------------------------------------------------------------------------------------------
def test_the_alias_resolves():
    assert C.LOGGING_CALLBACK_TARGET_ALIASES == {"src.callbacks.GradDistributionTB": "sota_imagenet_amd.callbacks.GradDistributionTB"}
    assert C.resolve_target("src.callbacks.GradDistributionTB") is callbacks.GradDistributionTB
    assert C.resolve_target("src.callbacks.OrthoInitClb") is callbacks.OrthoInitClb  # the tables before it still answer
    cb = C.call({"_target_": "src.callbacks.GradDistributionTB", "log_every": 50})
    assert (cb.log_every, cb.subsample, cb.state_keys) == (50, 10, ["exp_avg", "exp_avg_sq"])
    cb = callbacks.GradDistributionTB()
    assert (cb.log_every, cb.subsample, cb.state_keys, cb.last) == (500, 10, ["exp_avg", "exp_avg_sq"], {})
    with pytest.raises(ValueError):
        callbacks.GradDistributionTB(subsample=0)


@pytest.mark.parametrize("name, log_every", [("r50_nov_full", 50), ("nov_full_test", 5)])
def test_new_configs_compose_and_their_callbacks_construct(name, log_every):
    cfg = C.compose(None, [f"+hydra_exp={name}"])
    assert [c["_target_"] for c in cfg.run.extra_callbacks] == ["src.callbacks.OrthoInitClb", "src.callbacks.GradDistributionTB"]
    made = [C.call(c) for c in cfg.run.extra_callbacks]
    assert type(made[0]) is callbacks.OrthoInitClb and type(made[1]) is callbacks.GradDistributionTB
    assert made[1].log_every == log_every and made[1].subsample == 10 and made[1].state_keys == ["exp_avg", "exp_avg_sq"]
    assert cfg.optim._target_ == "src.optimizers.NovogradApex" and cfg.optim.wd_eps == 0.01 and cfg.optim.betas == [0.9, 0.99]


def test_r50_nov_full_is_r50_nov_plus_the_callbacks():
    full, base = C.to_plain(C.compose(None, ["+hydra_exp=r50_nov_full"])), C.to_plain(C.compose(None, ["+hydra_exp=r50_nov"]))
    for k in ("model", "optim", "criterion", "loader", "val_loader"):
        assert full[k] == base[k]
    assert full["run"]["stages"] == base["run"]["stages"] and full["run"]["ema_decay"] == base["run"]["ema_decay"] == 0.9993
    assert full["log"]["histogram"] and full["log"]["print_model"] and full["log"]["save_optim"]


def _on(model, opt, **state):
    cb = callbacks.GradDistributionTB(log_every=4, subsample=3)
    st = RunnerState(model=model, optimizer=opt)
    st.step, st.is_train = 0, True
    for k, v in state.items():
        setattr(st, k, v)
    cb.set_state(st)
    return cb


def _cpu_problem():
    m = torch.nn.Linear(3, 2)
    opt = torch.optim.Adam(m.parameters())
    m(torch.ones(1, 3)).sum().backward()
    opt.step()
    return m, opt


def test_cpu_tensors_raise_not_implemented():
    cb = _on(*_cpu_problem())
    with pytest.raises(NotImplementedError, match="no CPU path"):
        cb.on_batch_end()


def test_the_gates(monkeypatch):
    cb = _on(*_cpu_problem())
    calls = []
    monkeypatch.setattr(cb, "log", lambda: calls.append(cb.state.step))
    for step in range(10):
        cb.state.step = step
        cb.on_batch_end()
    assert calls == [0, 4, 8]  # step % log_every == 0
    cb.state.is_train, cb.state.step = False, 4
    cb.on_batch_end()  # a validation batch does not log
    assert calls == [0, 4, 8]
    cb.state.is_train, cb.state.rank = True, 1
    cb.on_batch_end()  # rank > 0 does nothing
    assert calls == [0, 4, 8] and cb.last == {} and cb.logged == 0
    cb.state.rank = 0
    monkeypatch.setenv("RANK", "3")
    cb.on_batch_end()
    assert calls == [0, 4, 8]
    monkeypatch.delenv("RANK")
    cb.on_batch_end()
    assert calls == [0, 4, 8, 4]


def test_state_errors_name_the_optimizer_and_the_key():
    m, opt = _cpu_problem()
    cb = _on(m, opt)
    cb.state_keys = ["exp_avg", "momentum_buffer"]
    with pytest.raises(KeyError, match="Adam.*momentum_buffer"):
        cb.on_batch_end()
    for v in opt.state.values():
        v["exp_avg_sq"] = 0.25  # MyAdai keeps it as a Python float
    cb.state_keys = ["exp_avg_sq"]
    with pytest.raises(TypeError, match="exp_avg_sq.*float"):
        cb.on_batch_end()
    with pytest.raises(RuntimeError, match="no state yet"):
        _on(m, torch.optim.Adam(m.parameters())).on_batch_end()


def test_raw_stats_from_the_bins():
    lim = ops.absbin_log10_limits()
    c = np.zeros(512, dtype=np.int64)
    assert callbacks.GradDistributionTB.raw_stats(lim, c) == (0.0, 0.0, 0, 0.0, 0.0)
    c[[0, 100, 101]] = [5, 2, 1]
    lo, hi, num, s1, s2 = callbacks.GradDistributionTB.raw_stats(lim, c)
    mid = [(-15 + lim[0]) / 2, (lim[99] + lim[100]) / 2, (lim[100] + lim[101]) / 2]
    assert (lo, hi, num) == (-15.0, lim[101], 8)
    assert s1 == pytest.approx(5 * mid[0] + 2 * mid[1] + mid[2]) and s2 == pytest.approx(5 * mid[0] ** 2 + 2 * mid[1] ** 2 + mid[2] ** 2)
