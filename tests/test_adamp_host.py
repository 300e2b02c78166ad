"""AdamP (sota_imagenet_amd.optim.AdamP, csrc/optim_adamp.hip) without a GPU: the class's signature and checks, the host side of its plan, the
target table and the config files, the entry points' validation, and the fixture's own conditions.  The rule is the published adamp.AdamP.step
restated from memory of the public package (tests/adamp_common.py, tests/golden/make_adamp_golden.py): unpinned against the package itself."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from adamp_common import CASES, DEFAULTS, GEN, Fixture, Restated
from sota_imagenet_amd import config as C
from sota_imagenet_amd import native

W = 4096


def test_signature_defaults_and_value_checks():
    from sota_imagenet_amd import optim

    sig = inspect.signature(optim.AdamP.__init__)
    assert [(k, v.default) for k, v in list(sig.parameters.items())[2:]] == [
        ("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("weight_decay", 0), ("delta", 0.1), ("wd_ratio", 0.1), ("nesterov", False)]
    cpu = [torch.nn.Parameter(torch.zeros(3, 2))]
    for bad in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1e-2), dict(delta=-0.1),
                dict(wd_ratio=-0.5)):
        with pytest.raises(ValueError):  # the value checks come before the placement check
            optim.AdamP(cpu, **bad)
    with pytest.raises(NotImplementedError, match="AdamP has no CPU path"):
        optim.AdamP(cpu)

    class Claims(torch.Tensor):  # a tensor that says it lives on the device: an instance to look at without a GPU (it is never stepped)
        is_cuda = True

    o = optim.AdamP([torch.zeros(3, 2).as_subclass(Claims).requires_grad_()])
    with pytest.raises(NotImplementedError, match="no CPU path"):
        o.add_param_group({"params": cpu})
    assert issubclass(optim.AdamP, torch.optim.Optimizer) and o.projection_modes is None
    assert set(o.defaults) == {"lr", "betas", "eps", "weight_decay", "delta", "wd_ratio", "nesterov"}
    assert o.defaults == dict(lr=1e-3, **DEFAULTS, weight_decay=0)


def _t(off, shape, group=0, base=(1, 2)):
    n = int(np.prod(shape))
    u = n // shape[0] if len(shape) > 1 else n
    return base + (off, n, group, u, len(shape) > 1)


def test_plan_tables_on_hand_made_layouts():
    from sota_imagenet_amd.optim import AdamP

    # one pair, two groups: (2, 5000) — a unit longer than an item —, (6, 2) — a unit shorter than a float4 —, (1, 4100), and two 1-D tensors
    tensors = [_t(0, (2, 5000)), _t(10048, (6, 2)), _t(10112, (1, 4100)), _t(14272, (64,), 1), _t(14336, (4100,), 1)]
    tab = AdamP.plan_tables(tensors, W)
    assert tab["decide"] == [(0, 2, 5000, 1), (2, 6, 2, 1), (8, 1, 4100, 1), (9, 1, 64, 0), (10, 1, 4100, 0)]
    assert tab["tensors"] == [(0, 5000, 0), (10048, 2, 2), (10112, 4100, 8), (14272, 64, 9), (14336, 4100, 10)]
    # a unit longer than an item is two pieces; the (1, 4100) tensor, which plan_units takes through whole items, is two pieces of stage (a) too
    assert tab["pieces"][:4] == [(0, 4096, 0), (4096, 904, 0), (5000, 4096, 1), (9096, 904, 1)]
    assert tab["pieces"][4:] == [(10048 + 2 * j, 2, 2 + j) for j in range(6)]
    assert tab["sum_pieces"] == tab["pieces"] + [(10112, 4096, 8), (14208, 4, 8)]
    assert tab["slots"] == [(0, 2), (2, 2)] + [(4 + j, 1) for j in range(6)] + [(10, 2), (12, 1), (13, 2)]
    assert tab["groups"] == [(0, 0, 3), (1, 3, 5)]
    (lo, hi, i0, i1, pc, wh, k0, ts, by_group, sums), = tab["pairs"]
    assert (lo, hi, i0, i1, pc, wh, k0, ts) == (0, 14336 + 4100, 0, len(tab["items"]), (0, 10), (0, 5), 0, [0, 1, 2, 3, 4])
    assert by_group == [(0, 0, 6), (1, 6, 9)]
    assert sums == [(0, 0, 12, 0)]  # one launch: twelve consecutive pieces onto twelve consecutive entries; group 1 has no pieces
    # the slots of a tensor are consecutive and every piece lies inside the unit of its slot
    for (s0, cnt, u, kind), (start, _, _) in zip(tab["decide"], tab["tensors"]):
        for off, ln, slot in tab["sum_pieces"]:
            if s0 <= slot < s0 + cnt:
                assert kind == 1 and start + (slot - s0) * u <= off and off + ln <= start + (slot - s0 + 1) * u
    covered = sorted((slot, off, ln) for off, ln, slot in tab["sum_pieces"])
    assert sum(ln for _, _, ln in covered) == 10000 + 12 + 4100

    # two storage pairs; in the second a 1-D tensor between two (1, n) tensors: their entries are not consecutive, so two launches
    tensors = [_t(0, (3, 7)), _t(0, (1, 40), base=(3, 4)), _t(64, (5,), base=(3, 4)), _t(128, (1, 8), base=(3, 4))]
    tab = AdamP.plan_tables(tensors, W)
    assert [pr[:2] for pr in tab["pairs"]] == [(0, 21), (0, 136)]
    assert tab["sum_pieces"] == [(0, 7, 0), (7, 7, 1), (14, 7, 2), (0, 40, 3), (128, 8, 5)]
    assert [pr[9] for pr in tab["pairs"]] == [[(0, 0, 3, 0)], [(0, 3, 4, 3), (0, 4, 5, 5)]]
    assert tab["slots"] == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1)]
    assert tab["decide"] == [(0, 3, 7, 1), (3, 1, 40, 1), (4, 1, 5, 0), (5, 1, 8, 1)]

    # two groups that both hold matrices: one launch of stage (a) per group
    tab = AdamP.plan_tables([_t(0, (4, 4)), _t(64, (2, 3), 1)], W)
    assert tab["pairs"][0][9] == [(0, 0, 4, 0), (1, 4, 6, 4)] and tab["groups"] == [(0, 0, 1), (1, 1, 2)]


def test_targets_and_config_files():
    from sota_imagenet_amd import optim

    assert C.ADAMP_TARGET_ALIASES == {"adamp.AdamP": "sota_imagenet_amd.optim.AdamP"}
    assert C.resolve_target("adamp.AdamP") is optim.AdamP
    with pytest.raises(ImportError):  # the modified variant of recipes 12 and 13 stays unresolved, on purpose
        C.resolve_target("pytorch_tools.optim.adamp.AdamP")
    for name, kw in (("r50_adamp", dict(weight_decay=1e-2, lr=0)), ("r50_adamp_low-eps", dict(weight_decay=1e-3, lr=0, eps=1e-5))):
        cfg = C.compose(None, [f"+hydra_exp={name}"])
        got = C.to_plain(cfg.optim)
        assert got.pop("_target_") == "adamp.AdamP" and got == kw
        assert cfg.loader.batch_size == 192 and cfg.loader.image_size == 224 and cfg.loader.color_twist_prob == 0.3
        assert cfg.run.ema_decay == 0.9993 and cfg.criterion.smoothing == 0.1 and cfg.log.exp_name == name
        assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 5, [0, 0.001], "linear"), (5, 90, [0.001, 0], "cos")]
        assert all(cb["_target_"] == "pytorch_tools.fit_wrapper.callbacks.Callback" for cb in cfg.run.extra_callbacks)  # both are left out
    cfg = C.compose(None, ["+hydra_exp=adamp_test"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "adamp.AdamP" and got == dict(weight_decay=1e-2, lr=0)
    assert cfg.log.exp_name == "adamp_test" and cfg.debug is True and cfg.loader.image_size == 64 and cfg.loader.batch_size == 16
    assert cfg.run.ema_decay == 0.9 and [(s["start"], s["end"]) for s in cfg.run.stages] == [(0, 1), (1, 2)]
    with pytest.raises(NotImplementedError, match="AdamP has no CPU path"):
        C.call(cfg.optim, [{"params": [torch.nn.Parameter(torch.zeros(4))]}])


P = ctypes.c_void_p


def test_entry_points_return_status_on_bad_arguments():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    A = 4096
    inf, nan = float("inf"), float("nan")
    for name in ("mi355_adamp_unit_sums", "mi355_adamp_coef", "mi355_adamp_update", "mi355_adamp_update_ema"):
        assert getattr(L, name).restype is ctypes.c_int

    def sums(p=A, g=A, m=A, v=A, pieces=A, partial=A, n_pieces=1, ns=1, b1=0.9, b2=0.999, eps=1e-8, step=1, gs=1.0):
        return L.mi355_adamp_unit_sums(P(p), P(g), P(m), P(v), 64, P(pieces), n_pieces, ns, b1, b2, eps, step, 0, gs, P(partial), None)

    for kw, word in ((dict(p=0), "null"), (dict(v=0), "null"), (dict(partial=0), "null"), (dict(g=A + 4), "aligned"), (dict(m=A + 8), "aligned"),
                     (dict(pieces=A + 8), "aligned"), (dict(partial=A + 4), "aligned"), (dict(n_pieces=0), "n_pieces"), (dict(ns=0), "n_slots"),
                     (dict(b1=1.0), "betas"), (dict(b2=-0.1), "betas"), (dict(eps=-1.0), "eps"), (dict(eps=nan), "eps"), (dict(step=0), "step"),
                     (dict(gs=inf), "grad_scale")):
        assert sums(**kw) == -1 and word in native.last_error(), kw

    def coef(partial=A, slots=A, decide=A, cf=A, wdf=A, mode=A, n_partial=1, ns=1, nt=1, lr=1e-3, wd=1e-2, eps=1e-8, delta=0.1, ratio=0.1):
        return L.mi355_adamp_coef(P(partial), n_partial, P(slots), ns, P(decide), nt, P(cf), P(wdf), P(mode), lr, wd, eps, delta, ratio, None)

    for kw, word in ((dict(partial=0), "null"), (dict(mode=0), "null"), (dict(decide=A + 8), "aligned"), (dict(slots=A + 4), "aligned"),
                     (dict(cf=A + 4), "aligned"), (dict(wdf=A + 2), "aligned"), (dict(mode=A + 2), "aligned"), (dict(n_partial=0), "n_partial"),
                     (dict(ns=0), "n_slots"), (dict(nt=0), "n_tensors"), (dict(lr=-1.0), "lr"), (dict(lr=nan), "lr"), (dict(wd=inf), "weight_decay"),
                     (dict(eps=-1.0), "eps"), (dict(delta=-0.1), "delta"), (dict(delta=inf), "delta"), (dict(ratio=-1.0), "wd_ratio"),
                     (dict(ratio=nan), "wd_ratio")):
        assert coef(**kw) == -1 and word in native.last_error(), kw

    def update(p=A, g=A, m=A, v=A, ema=None, items=A, tens=A, cf=A, wdf=A, n_items=1, nt=1, ns=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, step=1,
               gs=1.0, decay=0.9):
        args = (64, P(items), n_items, P(tens), nt, P(cf), ns, P(wdf), lr, b1, b2, eps, step, 0, gs)
        if ema is None:
            return L.mi355_adamp_update(P(p), P(g), P(m), P(v), *args, None)
        return L.mi355_adamp_update_ema(P(p), P(g), P(m), P(v), P(ema), *args, decay, None)

    for kw, word in ((dict(m=0), "null"), (dict(cf=0), "null"), (dict(wdf=0), "null"), (dict(v=A + 8), "aligned"), (dict(items=A + 8), "aligned"),
                     (dict(tens=A + 8), "aligned"), (dict(cf=A + 4), "aligned"), (dict(wdf=A + 2), "aligned"), (dict(ema=A + 4), "aligned"),
                     (dict(ema=0), "null"), (dict(n_items=0), "n_items"), (dict(nt=0), "n_tensors"), (dict(ns=0), "n_slots"), (dict(lr=-1.0), "lr"),
                     (dict(lr=inf), "lr"), (dict(b1=1.0), "betas"), (dict(b2=1.5), "betas"), (dict(eps=nan), "eps"), (dict(step=0), "step"),
                     (dict(step=-3), "step"), (dict(gs=nan), "grad_scale"), (dict(ema=A, decay=1.5), "ema_decay")):
        assert update(**kw) == -1 and word in native.last_error(), kw


@pytest.mark.parametrize("case", CASES)
def test_fixture_conditions_hold_on_its_own_arrays(case):
    """the recorder's conditions, re-derived from the stored inputs with the restatement: margins <= 0.5 or >= 2 in both runs and the stored
    modes; the float64 run reproduces p64, the float32 run the yard and the stored state; every projected tensor lies >= 100 yards away from the
    run without projection; the native float32 arithmetic (adamp_common) takes the same decisions and stays inside the GPU tests' bound"""
    fx = Fixture(case)
    assert fx.shapes == [tuple(s) for s in GEN.SHAPES] and os.path.getsize(os.path.join(os.path.dirname(__file__), "golden",
                                                                                          "adamp_ref_trajectories.npz")) <= 1.0e6
    want = {"channel": 1, "layer": 2, "none": 0, "1d": 0}
    assert (fx.modes == np.array([[want[w] for w in GEN.WANT]] * 4)).all()
    taken = fx.margins[~np.isnan(fx.margins)]
    assert ((taken <= 0.5) | (taken >= 2.0)).all()
    assert np.isnan(fx.margins[:, :, [4, 7], :]).all() and not np.isnan(fx.margins[:, :, [0, 1, 2, 3, 5, 6], 0]).any()
    assert (fx.effect[fx.modes > 0] >= 100 * fx.yard[fx.modes > 0]).all() and (fx.effect[fx.modes == 0] == 0).all()
    p0 = fx.split(fx.p0)
    h = dict(DEFAULTS, **fx.hyper)
    r64, r32, nat = (Restated(fx.hyper, p0, fx.group_of, fx.wds, dt, native=n) for dt, n in
                     ((torch.float64, False), (torch.float32, False), (torch.float32, True)))
    off = [t.double().clone() for t in p0]
    off_st = [dict(step=0, exp_avg=torch.zeros_like(t), exp_avg_sq=torch.zeros_like(t)) for t in off]
    for k in range(4):
        grads, lrs = fx.split(fx.grads[k]), [fx.lrs[k]] * len(fx.groups)
        for r in (r64, r32, nat):
            r.step(grads, lrs)
            assert r.modes == list(fx.modes[k])
        assert torch.equal(r64.flat(), fx.p64[k])
        for i in range(len(p0)):
            off[i], _, _ = GEN.adamp_tensor_step(off[i], grads[i].double(), off_st[i], h, fx.lrs[k], fx.wds[fx.group_of[i]], project=False)
            assert (r32.p[i].double() - r64.p[i]).abs().max().item() == fx.yard[k, i]
            assert (off[i] - r64.p[i]).abs().max().item() == fx.effect[k, i]
        fx.check(k, nat.p, f"{case} native float32 restatement")
    assert torch.equal(torch.cat([s["exp_avg"].reshape(-1) for s in r32.st]), fx.state4["exp_avg"])
    assert torch.equal(torch.cat([s["exp_avg_sq"].reshape(-1) for s in r32.st]), fx.state4["exp_avg_sq"])
    assert math.isfinite(fx.p64.abs().max().item())
