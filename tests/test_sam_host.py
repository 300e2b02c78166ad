"""SAMOriginal (sharpness-aware minimization) on the host: the reference's targets resolve to the native callback, the recipe and smoke configs
compose, accumulate_steps != 1 is refused, the documented rules — restated in float64 torch (tests/sam_common.py) — reproduce the trajectories that
the reference's own callback recorded in tests/golden/sam_ref_trajectories.npz, the plan marks the ndim > 1 tensors as weights and covers every
parameter element exactly once, and the four C-ABI entries refuse bad arguments before any launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from plan_common import resnet50_table as _resnet50_table
from sam_common import CASES, NORM_FLOOR, Fixture, restate_fixture
from sota_imagenet_amd import config as C
from sota_imagenet_amd import native



def test_reference_targets_resolve_to_the_native_callback():
    from sota_imagenet_amd import callbacks, fit_wrapper

    for target in ("src.callbacks.SAMOriginal", "sota_imagenet.callbacks.SAMOriginal"):
        assert C.resolve_target(target) is callbacks.SAMOriginal
        assert C.CALLBACK_TARGET_ALIASES[target] == "sota_imagenet_amd.callbacks.SAMOriginal"
        assert target not in C.TARGET_ALIASES and target not in C.LAYERWISE_TARGET_ALIASES
    clb = C.call({"_target_": "src.callbacks.SAMOriginal"})
    assert isinstance(clb, fit_wrapper.Callback) and (clb.rho, clb.eta) == (0.5, 0.01)
    assert clb.norm is None and clb.scale is None and clb.eps_flat is None
    clb = C.call({"_target_": "src.callbacks.SAMOriginal", "rho": 0.1, "eta": 0.0})
    assert (clb.rho, clb.eta) == (0.1, 0.0)
    for bad in (dict(rho=0), dict(rho=-1.0), dict(rho=float("inf")), dict(eta=-0.01), dict(eta=float("nan"))):
        with pytest.raises(ValueError):
            callbacks.SAMOriginal(**bad)


def test_recipe_and_smoke_configs_compose_with_the_callback_first():
    from sota_imagenet_amd import callbacks, fit_wrapper, optim

    ps = [{"params": [torch.nn.Parameter(torch.zeros(4))]}]
    kw = dict(weight_decay=2e-2, betas=[0.9, 0.995], lr=0)
    cfg = C.compose(None, ["+hydra_exp=r50_nov-adam_sam"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "src.optimizers.AdamLayerwise" and got == kw
    assert C.to_plain(cfg.run.extra_callbacks) == [{"_target_": "src.callbacks.SAMOriginal"},
                                                   {"_target_": "pytorch_tools.fit_wrapper.callbacks.Callback"}]
    made = [C.call(c) for c in cfg.run.extra_callbacks]
    assert type(made[0]) is callbacks.SAMOriginal and (made[0].rho, made[0].eta) == (0.5, 0.01) and type(made[1]) is fit_wrapper.Callback
    assert cfg.loader.batch_size == 192 and cfg.loader.image_size == 224 and cfg.loader.color_twist_prob == 0.3
    assert cfg.run.ema_decay == 0.9993 and cfg.criterion.smoothing == 0.1 and cfg.log.exp_name == "r50_nov-adam_sam"
    assert cfg.run.accumulate_steps == 1
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 5, [0.0001, 0.002], "linear"), (5, 90, [0.002, 0], "cos")]
    assert type(C.call(cfg.optim, ps)) is optim.AdamLayerwise
    # everything but the callback list and the name is the recipe without SAM
    plain = C.to_plain(C.compose(None, ["+hydra_exp=r50_nov-adam"]))
    with_sam = C.to_plain(cfg)
    for d in (plain, with_sam):
        d["run"].pop("extra_callbacks")
        d["log"].pop("exp_name")
    assert plain == with_sam

    cfg = C.compose(None, ["+hydra_exp=nov-adam_sam_test"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "src.optimizers.AdamLayerwise" and got == kw
    assert cfg.run.extra_callbacks[0]["_target_"] == "src.callbacks.SAMOriginal"
    assert cfg.log.exp_name == "nov-adam_sam_test" and cfg.debug is True and cfg.loader.image_size == 64 and cfg.loader.batch_size == 16
    plain, with_sam = C.to_plain(C.compose(None, ["+hydra_exp=nov-adam_test"])), C.to_plain(cfg)
    for d in (plain, with_sam):
        d["run"].pop("extra_callbacks")
        d["log"].pop("exp_name")
    assert plain == with_sam


def test_accumulate_steps_other_than_one_is_refused():
    from sota_imagenet_amd import callbacks, fit_wrapper

    clb = callbacks.SAMOriginal()
    clb.set_state(fit_wrapper.RunnerState(accumulate_steps=2))
    with pytest.raises(NotImplementedError, match="accumulate_steps"):
        clb.on_begin()
    clb.set_state(fit_wrapper.RunnerState(accumulate_steps=1))
    clb.on_begin()


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference_trajectory(case):
    """norm, eps, the parameters at the second forward and after the optimizer step, every step and tensor, to 1e-12 relative; the first step is
    skipped (one forward, no eps); the clamp case sits on the norm's floor"""
    fx = Fixture(case)
    got = restate_fixture(fx, torch.float64)
    assert fx.forwards == [1, 2, 2, 2] == [g[4] for g in got]
    assert math.isnan(fx.norm[0]) and math.isnan(got[0][0]) and not fx.eps[0].any() and not got[0][1].any()
    for k in range(fx.steps):
        norm, eps, pert, step, _ = got[k]
        if k:
            assert abs(norm - fx.norm[k]) <= 1e-12 * fx.norm[k], (case, k, norm, fx.norm[k])
            assert (norm == NORM_FLOOR) == (case == "clamp")
        for what, a, b in (("eps", eps, fx.eps[k]), ("pert", pert, fx.pert(k)), ("step", step, fx.p_step[k])):
            for i, (x, y) in enumerate(zip(fx.split(a), fx.split(b))):
                rel = ((x - y).abs().max() / y.abs().max().clamp_min(1e-300)).item()
                assert rel <= 1e-12, (case, what, k, i, rel)
        if k:
            assert all(t.abs().max() > 0 for t in fx.split(fx.eps[k]))  # every tensor is perturbed
    if case == "clamp":
        assert list(fx.norm[1:]) == [NORM_FLOOR] * 3
    assert (got[-1][3] - fx.p0.double()).abs().max().item() > (1e-9 if case == "clamp" else 1e-3)  # the steps moved the parameters


def test_plan_marks_the_weights_and_covers_every_element_once():
    """the plan over the ResNet-50 flat layout (161 tensors in one storage pair): kind = 1 exactly for the tensors with more than one dimension
    (the 53 conv weights and fc.weight), the items cover every tensor's own range once and nothing of the padding; tensors in storages of
    their own get one launch set each, their items counted from their own start"""
    from sota_imagenet_amd.callbacks import SAMOriginal

    table, total = _resnet50_table()
    W = int(native.lib().mi355_lw_item_elems())
    sizes = [int(np.prod(shape)) for _, _, shape in table]
    items, kind, pairs = SAMOriginal.plan_tables([(1 << 20, 1 << 30, off, n, len(shape)) for (_, off, shape), n in zip(table, sizes)], W)
    assert len(kind) == 161 and kind == [int(len(shape) > 1) for _, _, shape in table] and sum(kind) == 54
    assert [name for (name, _, _), k in zip(table, kind) if k and "conv" not in name and "downsample" not in name] == ["fc.weight"]
    assert not any(k for (name, _, shape), k in zip(table, kind) if name.endswith(".bias") or len(shape) == 1)
    lo = min(off for _, off, _ in table)
    assert pairs == [(lo, max(off + n for (_, off, _), n in zip(table, sizes)), 0, len(items), list(range(161)))]
    cover = np.zeros(total, dtype=np.uint8)
    for off, ln, t in items:
        assert 1 <= ln <= W and off % 4 == 0
        b, n = table[t][1], sizes[t]
        assert b <= lo + off and lo + off + ln <= b + n  # inside ONE tensor
        cover[lo + off: lo + off + ln] += 1
    real = np.zeros(total, dtype=bool)
    for (_, off, _), n in zip(table, sizes):
        real[off: off + n] = True
    assert (~real).any() and (cover[real] == 1).all() and (cover[~real] == 0).all()
    # the fixture's six tensors, each in its own parameter / gradient storage, listed group by group as the optimizer lists them
    fx = Fixture("sgd")
    order = [i for idx in fx.groups for i in idx]
    tensors = [(4096 * (i + 1), 1 << 30 | 4096 * (i + 1), 0, fx.sizes[i], len(fx.shapes[i])) for i in order]
    items, kind, pairs = SAMOriginal.plan_tables(tensors, W)
    assert kind == [1, 1, 1, 1, 0, 0] and len(pairs) == 6 and len(items) == 7  # 4797 elements: two items
    for j, (lo, hi, i0, i1, ts) in enumerate(pairs):
        assert (lo, hi, ts) == (0, fx.sizes[order[j]], [j])
        assert [(o, t) for o, _, t in items[i0:i1]] == [(c, j) for c in range(0, hi, W)] and sum(ln for _, ln, _ in items[i0:i1]) == hi
    assert [ln for _, ln, t in items if t == 3] == [4096, 701]


P = ctypes.c_void_p


def test_bad_arguments_return_status_not_crash():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    A = 4096
    E = -1  # MI355_E_ARG
    inf, nan = float("inf"), float("nan")

    def sumsq(p=A, g=A, items=A, kind=A, partial=A, n_items=1, nt=1, eta=0.01, gs=1.0):
        return L.mi355_sam_sumsq(P(p), P(g), 64, P(items), n_items, P(kind), nt, eta, gs, P(partial), None)

    assert sumsq(p=0) == E and "null" in native.last_error()
    assert sumsq(kind=0) == E and "null" in native.last_error()
    assert sumsq(partial=0) == E and "null" in native.last_error()
    assert sumsq(g=A + 4) == E and "aligned" in native.last_error()
    assert sumsq(items=A + 8) == E and "aligned" in native.last_error()
    assert sumsq(partial=A + 4) == E and "aligned" in native.last_error()
    assert sumsq(kind=A + 2) == E and "aligned" in native.last_error()
    assert sumsq(n_items=0) == E and "n_items" in native.last_error()
    assert sumsq(nt=0) == E and "n_tensors" in native.last_error()
    assert sumsq(eta=nan) == E and "eta" in native.last_error()
    assert sumsq(eta=inf) == E and "eta" in native.last_error()
    assert sumsq(eta=-0.01) == E and "eta" in native.last_error()
    assert sumsq(gs=inf) == E and "grad_scale" in native.last_error()

    def scale(partial=A, n=1, rho=0.5, out=A):
        return L.mi355_sam_scale(P(partial), n, rho, P(out), None)

    assert scale(partial=0) == E and "null" in native.last_error()
    assert scale(out=0) == E and "null" in native.last_error()
    assert scale(partial=A + 4) == E and "aligned" in native.last_error()
    assert scale(out=A + 4) == E and "aligned" in native.last_error()
    assert scale(n=0) == E and "n_partial" in native.last_error()
    assert scale(rho=0.0) == E and "rho" in native.last_error()
    assert scale(rho=-0.5) == E and "rho" in native.last_error()
    assert scale(rho=nan) == E and "rho" in native.last_error()

    def perturb(p=A, g=A, eps=A, items=A, kind=A, out=A, n_items=1, nt=1, eta=0.01, gs=1.0):
        return L.mi355_sam_perturb(P(p), P(g), P(eps), 64, P(items), n_items, P(kind), nt, P(out), eta, gs, None)

    assert perturb(eps=0) == E and "null" in native.last_error()
    assert perturb(out=0) == E and "null" in native.last_error()
    assert perturb(p=A + 8) == E and "aligned" in native.last_error()
    assert perturb(eps=A + 4) == E and "aligned" in native.last_error()
    assert perturb(out=A + 4) == E and "aligned" in native.last_error()
    assert perturb(n_items=0) == E and "n_items" in native.last_error()
    assert perturb(eta=nan) == E and "eta" in native.last_error()
    assert perturb(eta=-1.0) == E and "eta" in native.last_error()
    assert perturb(gs=nan) == E and "grad_scale" in native.last_error()

    def restore(p=A, eps=A, items=A, n_items=1, nt=1):
        return L.mi355_sam_restore(P(p), P(eps), 64, P(items), n_items, nt, None)

    assert restore(p=0) == E and "null" in native.last_error()
    assert restore(items=0) == E and "null" in native.last_error()
    assert restore(eps=A + 4) == E and "aligned" in native.last_error()
    assert restore(items=A + 8) == E and "aligned" in native.last_error()
    assert restore(n_items=0) == E and "n_items" in native.last_error()
    assert restore(nt=0) == E and "n_tensors" in native.last_error()
