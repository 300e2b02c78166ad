"""The layer-wise optimizers (NovogradApex, MyNovograd, AdamLayerwise, MyAdai) on the host: the four update rules as this project documents
them reproduce — restated in float64 torch (tests/layerwise_common.py) — the trajectories that the reference's own classes recorded in
tests/golden/layerwise_ref_trajectories.npz; the work-item planner covers every parameter element exactly once and nothing else; the
reference's targets resolve, the constructors keep the reference's domains, the flags that are not on the hot path raise, the recipe
configs compose, and the C-ABI entries refuse bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from layerwise_common import CASES, Fixture, restate_fixture
from plan_common import resnet50_params as _resnet50_params
from sota_imagenet_amd import config as C
from sota_imagenet_amd import native

CLASSES = ("NovogradApex", "MyNovograd", "AdamLayerwise", "MyAdai")


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_reproduces_the_reference_trajectory(case):
    """every recorded p64 (six steps, five tensors) to 1e-12 relative; for MyAdai also the recorded beta1 of every step and tensor"""
    fx = Fixture(case)
    got, r = restate_fixture(fx, torch.float64)
    for k in range(6):
        for i, (a, b) in enumerate(zip(fx.split(got[k]), fx.split(fx.p64[k]))):
            rel = ((a - b).abs().max() / b.abs().max()).item()
            assert rel <= 1e-12, (case, k, i, rel)
    assert (got[-1] - fx.p0.double()).abs().max().item() > 1e-3  # the steps moved the parameters
    if fx.cls == "MyAdai":
        assert np.abs(np.array(r.beta1) - fx.beta1).max() <= 1e-12
        hi = 1 - fx.hyper.get("eps", 1e-3)
        assert (fx.beta1 == 0).any() and ((fx.beta1 > 0) & (fx.beta1 < hi)).any()  # the regimes the generator asserted
        assert (fx.beta1 == hi).any() == (case == "myadai_alt")
        assert list(fx.v0) == [fx.hyper.get("ema_norm_init", 1e-3)] * 5  # the state's second moment is still the constant it was created with


def test_item_planner_covers_every_parameter_element_once_and_no_padding():
    from sota_imagenet_amd.optim import lw_plan_items

    W = int(native.lib().mi355_lw_item_elems())
    assert W >= 256 and W % 4 == 0
    params, total = _resnet50_params()
    assert len(params) == 161 and sum(n for _, n in params) == 25557032 < total
    items, spans = lw_plan_items(params, W)
    cover = np.zeros(total, dtype=np.uint8)
    for off, ln, t in items:
        assert 1 <= ln <= W and off % 4 == 0
        lo, n = params[t]
        assert lo <= off and off + ln <= lo + n  # inside ONE tensor
        cover[off:off + ln] += 1
    real = np.zeros(total, dtype=bool)
    for lo, n in params:
        real[lo:lo + n] = True
    assert (~real).any() and (cover[real] == 1).all() and (cover[~real] == 0).all()
    # the items of a tensor are consecutive, in order, and the cuts depend on numel alone: the same tensor somewhere else gives the same lengths
    for t, (first, count) in enumerate(spans):
        lo, n = params[t]
        mine = items[first:first + count]
        assert count == -(-n // W) and [x[2] for x in mine] == [t] * count
        assert [x[0] - lo for x in mine] == list(range(0, n, W))
        moved, _ = lw_plan_items([(7 * 64, 5), (lo + 4096 * 3, n)], W)
        assert [x[1] for x in moved[1:]] == [x[1] for x in mine]
    # group by group: the table follows the order it is given
    assert [x[2] for x in items] == sorted(x[2] for x in items)
    with pytest.raises(ValueError):
        lw_plan_items([(0, 0)], W)


def test_reference_targets_resolve_to_the_native_classes():
    from sota_imagenet_amd import optim

    for name in CLASSES:
        for target in (f"src.optimizers.{name}", f"sota_imagenet.optimizers.{name}"):
            assert C.resolve_target(target) is getattr(optim, name)
        assert issubclass(getattr(optim, name), optim._FlatOptimizer)
        assert C.LAYERWISE_TARGET_ALIASES[f"src.optimizers.{name}"] == f"sota_imagenet_amd.optim.{name}"


def test_constructor_domains_and_defaults_are_the_references():
    from sota_imagenet_amd import optim

    ps = [torch.nn.Parameter(torch.zeros(4))]
    assert optim.NovogradApex(ps).defaults == dict(lr=1e-3, betas=(0.95, 0), eps=1e-8, weight_decay=0)
    assert optim.AdamLayerwise(ps).defaults == dict(lr=1e-3, betas=(0.95, 0), eps=1e-6, weight_decay=0)
    assert optim.MyNovograd(ps).defaults == dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-2, ema_norm_init=1e-3)
    assert optim.MyAdai(ps).defaults == dict(lr=1e-3, betas=(0.1, 0.99), eps=1e-3, weight_decay=0)
    o = optim.MyNovograd(ps, eps=1e-5)
    assert o.eps == 1e-5 and "eps" not in o.defaults  # an attribute of the optimizer, not of the group
    a = optim.MyAdai(ps, sgd_mom=True, stable_wd=True)
    assert (a.ema_norm_init, a.sgd_mom, a.sqrt_mom, a.stable_wd, a.per_layer) == (1e-3, True, False, True, True)
    n = optim.NovogradApex(ps, wd_eps=0.01)
    assert n.wd_eps == 0.01 and n.ema_norm_init == 1e-3 and optim.AdamLayerwise(ps, stable_wd=True).stable_wd is True
    for name in CLASSES:
        cls = getattr(optim, name)
        cls(ps, lr=0)  # the recipes arrive with the base config's lr 0
        for bad in (dict(lr=-1e-3), dict(eps=-1e-8), dict(betas=(1.0, 0.9)), dict(betas=(-0.1, 0.9)), dict(betas=(0.9, 1.0)), dict(betas=(0.9, -0.1))):
            with pytest.raises(ValueError):
                cls(ps, **bad)
        cls(ps, betas=(0.0, 0.0), eps=0)
    with pytest.raises(ValueError):
        optim.MyNovograd(ps, weight_decay=-1e-3)
    optim.NovogradApex(ps, weight_decay=-1e-3)  # the other three classes do not check weight_decay, as in the reference


def test_flags_off_the_hot_path_raise_and_name_the_flag():
    from sota_imagenet_amd import optim

    ps = [torch.nn.Parameter(torch.zeros(4))]
    for cls, flag in ((optim.NovogradApex, "unitwise_norm"), (optim.MyNovograd, "unitwise_norm"), (optim.AdamLayerwise, "weight_adapt")):
        with pytest.raises(NotImplementedError, match=flag):
            cls(ps, **{flag: True})
    with pytest.raises(NotImplementedError, match="per_layer"):
        optim.MyAdai(ps, per_layer=False)


RECIPES = {
    "r50_nov": ("NovogradApex", dict(weight_decay=0.002, betas=[0.9, 0.99], lr=0, wd_eps=0.01), [0.0001, 0.05], "nov_test"),
    "r50_my-nov": ("MyNovograd", dict(weight_decay=0.002, betas=[0.9, 0.99], lr=0), [0.0001, 0.05], "my-nov_test"),
    "r50_nov-adam": ("AdamLayerwise", dict(weight_decay=2e-2, betas=[0.9, 0.995], lr=0), [0.0001, 0.002], "nov-adam_test"),
    "r50_adai_2": ("MyAdai", dict(betas=[0.1, 0.99], weight_decay=3e-5, lr=0, sgd_mom=True, stable_wd=True), [0.0001, 0.1], "adai_2_test"),
}


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_recipe_configs_compose_and_instantiate(name):
    from sota_imagenet_amd import optim

    cls_name, kw, lr, smoke = RECIPES[name]
    ps = [{"params": [torch.nn.Parameter(torch.zeros(4))]}]
    cfg = C.compose(None, [f"+hydra_exp={name}"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == f"src.optimizers.{cls_name}" and got == kw
    assert cfg.loader.batch_size == 192 and cfg.loader.image_size == 224 and cfg.loader.color_twist_prob == 0.3
    assert cfg.run.ema_decay == 0.9993 and cfg.criterion.smoothing == 0.1 and cfg.log.exp_name == name
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 5, lr, "linear"), (5, 90, [lr[1], 0], "cos")]
    assert all(cb["_target_"] == "pytorch_tools.fit_wrapper.callbacks.Callback" for cb in cfg.run.extra_callbacks)  # the left-out callbacks
    assert type(C.call(cfg.optim, ps)) is getattr(optim, cls_name)
    cfg = C.compose(None, [f"+hydra_exp={smoke}"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == f"src.optimizers.{cls_name}" and got == kw
    assert cfg.log.exp_name == smoke and cfg.debug is True and cfg.loader.image_size == 64
    assert type(C.call(cfg.optim, ps)) is getattr(optim, cls_name)


P = ctypes.c_void_p


def test_bad_arguments_return_status_not_crash():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    A = 4096
    assert L.mi355_lw_item_elems() % 4 == 0

    def sumsq(src=A, items=A, partial=A, n_items=1, nt=1, scale=1.0):
        return L.mi355_lw_sumsq(P(src), 64, P(items), n_items, nt, scale, P(partial), None)

    assert sumsq(src=0) == -1 and "null" in native.last_error()
    assert sumsq(src=A + 4) == -1 and "aligned" in native.last_error()
    assert sumsq(items=A + 8) == -1 and "aligned" in native.last_error()
    assert sumsq(partial=A + 4) == -1 and "aligned" in native.last_error()
    assert sumsq(n_items=0) == -1 and "n_items" in native.last_error()
    assert sumsq(nt=0) == -1 and "n_tensors" in native.last_error()
    assert sumsq(scale=float("nan")) == -1 and "scale" in native.last_error()

    def coef(rule=0, flags=0, partial=A, tens=A, v=A, c=A, sums=A, nt=1, b1=0.9, b2=0.99, eps=1e-8, lr=1e-3, wd=0.0, mean=1e-3):
        return L.mi355_lw_coef(rule, flags, P(partial), 1, P(tens), nt, P(v), P(c), P(sums), b1, b2, eps, lr, wd, mean, None)

    assert coef(v=0) == -1 and "null" in native.last_error()
    assert coef(c=A + 4) == -1 and "aligned" in native.last_error()
    assert coef(rule=2, v=A + 4) == -1 and "aligned" in native.last_error()
    assert coef(rule=3) == -1 and "rule" in native.last_error()
    assert coef(flags=32) == -1 and "flag" in native.last_error()
    assert coef(nt=0) == -1 and "n_tensors" in native.last_error()
    assert coef(b1=1.0) == -1 and "beta1" in native.last_error()
    assert coef(b2=-0.1) == -1 and "beta2" in native.last_error()
    assert coef(eps=-1e-3) == -1 and "eps" in native.last_error()
    assert coef(lr=float("inf")) == -1 and "lr" in native.last_error()
    assert coef(wd=float("nan")) == -1 and "weight_decay" in native.last_error()
    assert coef(rule=2, mean=0.0) == -1 and "mean" in native.last_error()

    def update(rule=0, p=A, g=A, m=A, ema=None, items=A, c=A, n_items=1, nt=1, lr=1e-3, soft=0, wd_eps=0.0, gs=1.0, decay=0.9):
        args = (64, P(items), n_items, P(c), nt, lr, soft, wd_eps, gs)
        if ema is None:
            return L.mi355_lw_update(rule, P(p), P(g), P(m), *args, None)
        return L.mi355_lw_update_ema(rule, P(p), P(g), P(m), P(ema), *args, decay, None)

    assert update(m=0) == -1 and "null" in native.last_error()
    assert update(g=A + 8) == -1 and "aligned" in native.last_error()
    assert update(ema=A + 4) == -1 and "aligned" in native.last_error()
    assert update(rule=-1) == -1 and "rule" in native.last_error()
    assert update(n_items=0) == -1 and "n_items" in native.last_error()
    assert update(lr=-1.0) == -1 and "lr" in native.last_error()
    assert update(rule=1, soft=1) == -1 and "wd_eps" in native.last_error()
    assert update(gs=float("inf")) == -1 and "grad_scale" in native.last_error()
    assert update(ema=A, decay=1.5) == -1 and "ema_decay" in native.last_error()
    assert L.mi355_lw_update_ema(0, P(A), P(A), P(A), None, 64, P(A), 1, P(A), 1, 1e-3, 0, 0.0, 1.0, 0.9, None) == -1 and "null ema" in native.last_error()
