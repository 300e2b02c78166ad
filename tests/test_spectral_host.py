"""The host side of the forward spectral normalisation: the float64 restatement of tests/spectral_common.py against torch's own spectral_norm, the
matrix plan, the start draws, the declared entry points and their refusals, the two switches' mutual exclusion, the callback's refusals, its alias
table and the smoke config.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import spectral_common as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def test_float64_restatement_against_torch_spectral_norm():
    """torch.nn.utils.parametrizations.spectral_norm on a float64 Conv2d(6, 10, 3), teacher-forced from its _u, _v: u, v, sigma, w_hat of one
    training forward and the weight gradient through autograd, against the rule on the filters in memory order (K, K, Cin) with v permuted"""
    from torch.nn.utils.parametrizations import spectral_norm

    torch.manual_seed(0)
    conv = spectral_norm(torch.nn.Conv2d(6, 10, 3, bias=False).double())
    p = conv.parametrizations.weight[0]
    u0, v0 = p._u.detach().numpy().copy(), p._v.detach().numpy().copy()
    W = conv.parametrizations.weight.original
    Wm = W.detach().permute(0, 2, 3, 1).reshape(10, -1).numpy()  # rows in (K, K, Cin) order
    conv.train()
    w_hat = conv.weight  # one power iteration
    gsrc = torch.randn(10, 6, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 33
    (w_hat * gsrc).sum().backward()
    u, v, sig = SN.iterate64(Wm, u0, SN.v_from_torch(v0, 3, 6), 1)
    assert _rel(u, p._u.detach().numpy()) < 1e-12
    assert _rel(SN.v_to_torch(v, 3, 6), p._v.detach().numpy()) < 1e-12
    assert abs(sig - torch.vdot(p._u, torch.mv(W.detach().flatten(1), p._v)).item()) < 1e-12 * abs(sig)
    wh = Wm / sig
    assert _rel(wh, w_hat.detach().permute(0, 2, 3, 1).reshape(10, -1).numpy()) < 1e-12
    # the backward rule with u, v constants: (g - (sum g w_hat) u v^T) / sigma
    g = gsrc.permute(0, 2, 3, 1).reshape(10, -1).numpy()
    dw = (g - (g * wh).sum() * np.outer(u, v)) / sig
    assert _rel(dw, W.grad.permute(0, 2, 3, 1).reshape(10, -1).numpy()) < 1e-12
    # the bounded form gives the same reference
    ref, bound = SN.bwd64(g.astype(np.float32), wh.astype(np.float32), u.astype(np.float32), v.astype(np.float32), np.float32(sig))
    assert _rel(ref, dw) < 1e-5 and (bound > 0).all()
    # eval: no iteration, sigma = u . W v from the stored vectors
    conv.eval()
    w_eval = conv.weight.detach().permute(0, 2, 3, 1).reshape(10, -1).numpy()
    _, _, sig0 = SN.iterate64(Wm, u, v, 0)
    assert _rel(Wm / sig0, w_eval) < 1e-12


def test_v_permutation_round_trips():
    v = np.arange(3 * 3 * 5, dtype=np.float32)
    t = SN.v_to_torch(v, 3, 5)
    assert not np.array_equal(t, v) and np.array_equal(SN.v_from_torch(t, 3, 5), v)
    assert t.reshape(5, 3, 3)[2, 1, 0] == v.reshape(3, 3, 5)[1, 0, 2]
    assert np.array_equal(SN.v_to_torch(np.arange(7.0), 1, 7), np.arange(7.0)), "a 1x1 conv's v is the same either way"


def test_plan_covers_every_conv_filter_once():
    from sota_imagenet_amd import item_plan
    from sota_imagenet_amd.models import resnet50

    m = resnet50(num_classes=10)
    mats, n_u, n_v = item_plan.spectral_mats(m._table)
    convs = [(off, shape) for _, kind, off, shape in m._table if kind == 0 and len(shape) == 4]
    assert len(mats) == len(convs) == 53
    assert n_u == sum(s[0] for _, s in convs) == 26560 == len(item_plan.ws_rows(m._table))
    assert n_v == sum(int(np.prod(s[1:])) for _, s in convs) == 52883
    assert sorted(o for o, *_ in mats) == sorted(o for o, _ in convs) and [o for o, *_ in mats] == sorted(o for o, *_ in mats)
    by_off = dict(convs)
    u0 = v0 = 0
    for off, L, R, a, b in mats:
        assert (R, L) == (by_off[off][0], int(np.prod(by_off[off][1:]))) and (a, b) == (u0, v0)
        u0, v0 = u0 + R, v0 + L
    fc = next(off for name, kind, off, shape in m._table if name == "fc.weight")
    assert all(not (o <= fc < o + L * R) and not (fc <= o < fc + 10 * 2048) for o, L, R, _, _ in mats), "the FC is no conv"
    packed = item_plan.pack_records(mats[:2], None, item_plan.SPECTRAL_FIELDS)
    assert packed.shape == (2, 4) and packed[1, 0].item() == mats[1][0] and packed[1, 2].item() == mats[1][3] and packed[1, 3].item() == mats[1][4]
    assert packed[1, 1].item() == mats[1][1] + (mats[1][2] << 32)  # { int64 off; int32 len; int32 rows; int64 u0; int64 v0 }


def test_start_draws_depend_on_the_seed_alone():
    from sota_imagenet_amd.models import ResNet50, resnet50

    table = resnet50(num_classes=10)._table
    torch.manual_seed(5)
    a = ResNet50.spectral_draws(table, 0)
    torch.manual_seed(99)
    state = torch.get_rng_state()
    b = ResNet50.spectral_draws(table, 0)
    assert torch.equal(torch.get_rng_state(), state), "the global generator is not advanced"
    c = ResNet50.spectral_draws(table, 1)
    assert len(a) == 53 and list(a) == [n[: -len(".weight")] for n, k, _, s in table if k == 0 and len(s) == 4]
    assert all(torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]) for k in a), "same seed, whatever the global generator holds"
    assert all(not torch.equal(a[k][0], c[k][0]) and not torch.equal(a[k][1], c[k][1]) for k in a), "another seed, other draws"
    assert a["conv1"][0].shape == (64,) and a["conv1"][1].shape == (3, 7, 7)
    assert all(abs(u.norm().item() - 1) < 1e-6 and abs(v.norm().item() - 1) < 1e-6 for u, v in a.values())


def test_header_constants_and_makefile():
    from sota_imagenet_amd import native, ops

    protos = native.parse_header()
    assert protos["mi355_spectral_fwd"][0] == "int" and len(protos["mi355_spectral_fwd"][1]) == 13
    assert len(protos["mi355_spectral_bwd"][1]) == 16 and protos["mi355_spectral_scratch_doubles"][0] == "size_t"
    ret, params = protos["mi355_resnet50_set_spectral_norm"]
    assert ret == "int" and [p.split()[0] for p in params] == ["mi355_ctx*", "int", "float*", "float*"]
    assert len(protos["mi355_resnet50_set_weight_transform"][1]) == 2, "a switch of its own: the weight transform keeps its prototype"
    text = open(os.path.join(ROOT, "include", "mi355rn.h")).read()
    macros = dict(re.findall(r"^#define\s+(MI355_SN_\w+)\s+(\S+)", text, re.M))
    assert set(macros) == {"MI355_SN_EPS", "MI355_SN_WARM_ITERS", "MI355_SN_SLABS"}
    assert macros["MI355_SN_EPS"] == "1e-12f" and float(macros["MI355_SN_EPS"][:-1]) == ops.SN_EPS
    assert int(macros["MI355_SN_WARM_ITERS"]) == ops.SN_WARM_ITERS == SN.WARM_ITERS == 15
    assert int(macros["MI355_SN_SLABS"]) == ops.SN_SLABS
    L = native.lib()
    assert L.mi355_spectral_scratch_doubles(26560, 52883) == 2 * 26560 + (1 + ops.SN_SLABS) * 52883
    csrc = os.path.join(ROOT, "sota_imagenet_amd", "csrc")
    assert re.search(r"^SRCS\s*:=.*\bspectral_norm\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "spectral_norm.hip")).read())  # (without the comments)
    assert "MI355_SN_EPS" in src and "MI355_SN_SLABS" in src and not re.search(r"1e-12|atomic", src), "the constants are not restated; no atomics"
    assert src.rindex('extern "C"') > src.rindex("__global__"), "the entry points stand at the bottom, with their launchers"


def test_layout_only_and_argument_refusals_of_the_entry_points():
    from sota_imagenet_amd import native

    L = native.lib()
    p = torch.zeros(64).data_ptr()  # dummy pointers, never dereferenced
    c = ctypes.c_void_p()
    native.check(L.mi355_resnet50_create(ctypes.byref(c), -1, native.F32, 2, 64, 64, 10))
    try:
        assert L.mi355_resnet50_set_spectral_norm(None, 1, p, p) == -1
        assert L.mi355_resnet50_set_spectral_norm(c, 1, None, p) == -1 and L.mi355_resnet50_set_spectral_norm(c, 1, p, None) == -1
        assert L.mi355_resnet50_set_spectral_norm(c, 0, None, None) == 0
        assert L.mi355_resnet50_set_spectral_norm(c, 1, p, p) == -3 and "layout-only" in native.last_error()  # no device, no scratch
        assert L.mi355_resnet50_set_weight_transform(c, 3) == -1, "spectral normalisation is no mode of the weight transform"
    finally:
        L.mi355_resnet50_destroy(c)
    native.check(L.mi355_resnet50_create(ctypes.byref(c), -1, native.FP8, 2, 64, 64, 10))
    try:
        assert L.mi355_resnet50_set_spectral_norm(c, 1, p, p) == -1 and "fp8" in native.last_error()
        assert L.mi355_resnet50_set_spectral_norm(c, 0, None, None) == 0
    finally:
        L.mi355_resnet50_destroy(c)
    fwd, bwd = L.mi355_spectral_fwd, L.mi355_spectral_bwd
    assert fwd(p, p, p, p, p, p, 64, 4, 4, p, 1, 16, None) == -1 and "iters" in native.last_error()
    assert fwd(p, p, p, p, p, p, 64, 4, 4, p, 1, -1, None) == -1
    assert fwd(p, p, p, p, p, p, 64, 4, 4, None, 1, 1, None) == -1 and "null" in native.last_error()
    assert fwd(p, None, None, p, p, p, 64, 4, 4, p, 1, 1, None) == -1 and fwd(p, None, p, p, p, None, 64, 4, 4, p, 1, 1, None) == -1
    assert fwd(p + 4, p, p, p, p, p, 64, 4, 4, p, 1, 1, None) == -1 and "misaligned" in native.last_error()
    assert fwd(p, p + 8, p, p, p, p, 64, 4, 4, p, 1, 1, None) == -1 and fwd(p, p, p + 2, p, p, p, 64, 4, 4, p, 1, 1, None) == -1
    for n, n_u, n_v, n_mats in ((0, 4, 4, 1), (64, 0, 4, 1), (64, 4, 0, 1), (64, 4, 4, 0), (64, 4, 4, 65536)):
        assert fwd(p, p, p, p, p, p, n, n_u, n_v, p, n_mats, 1, None) == -1 and "out of range" in native.last_error()
    q = p + 64
    assert bwd(p, q, p, p, p, p, p, 64, 4, 4, p, 1, 0, 4, 0.0, None) == -1 and "dw" in native.last_error()
    assert bwd(p, q, p, p, p, q, p, 64, 4, 4, p, 1, 0, 4, 0.0, None) == -1
    assert bwd(p, q, p, p, p, q + 64, p, 64, 4, 4, p, 1, 2, 2, 0.0, None) == -1 and "rows" in native.last_error()
    assert bwd(p, q, p, p, p, q + 64, p, 64, 4, 4, p, 1, 0, 5, 0.0, None) == -1
    assert bwd(p, q, p, p, None, q + 64, p, 64, 4, 4, p, 1, 0, 4, 0.0, None) == -1 and "null" in native.last_error()


def test_the_two_switches_exclude_each_other():
    from sota_imagenet_amd.models import resnet50

    m = resnet50(num_classes=10, weight_standardization=True)
    with pytest.raises(RuntimeError, match="exclude"):
        m.set_spectral_norm(True)
    assert m.spectral_norm is False and m.weight_transform == 1
    m.set_spectral_norm(False)  # switching off what is off is nothing
    m = resnet50(num_classes=10)
    m._sn = dict()  # as if it were on: set_weight_transform must refuse before it touches anything
    for mode in ("standardise", "centre", 1, 2):
        with pytest.raises(RuntimeError, match="exclude"):
            m.set_weight_transform(mode)
    m.set_weight_transform("off")
    assert m.weight_transform == 0
    m._sn = None


def test_model_and_callback_refusals():
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.callbacks import ForwardSpectralNorm
    from sota_imagenet_amd.fit_wrapper import RunnerState
    from sota_imagenet_amd.models import resnet50

    with pytest.raises(ValueError, match="fp8"):
        resnet50(num_classes=10, dtype="fp8").set_spectral_norm(True)
    with pytest.raises(RuntimeError, match="cuda"):
        resnet50(num_classes=10).set_spectral_norm(True)
    m = resnet50(num_classes=10)
    assert m.spectral_norm is False and m.spectral_u is None and m.spectral_v is None
    with pytest.raises(RuntimeError):
        m.spectral_state()
    with pytest.raises(RuntimeError):
        m.load_spectral_state({})
    cb = ForwardSpectralNorm()
    assert cb.seed == 0 and ForwardSpectralNorm(seed=7).seed == 7
    # not a flat model / a flat model on the CPU / the variant graph: no module walk, no CPU path
    for model in (torch.nn.Conv2d(3, 8, 3), resnet50(num_classes=10), BResNet50(num_classes=10)):
        cb.set_state(RunnerState(model=model))
        with pytest.raises(NotImplementedError):
            cb.on_begin()
        with pytest.raises(NotImplementedError):
            cb.on_end()
    assert not hasattr(BResNet50(num_classes=10), "set_spectral_norm")
    doc = ForwardSpectralNorm.__doc__
    assert all(s in doc for s in ("raw weights", "warms anew", "seed", "double"))


def test_alias_table():
    from sota_imagenet_amd import callbacks, config as C

    assert C.FORWARD_SPECTRAL_CALLBACK_TARGET_ALIASES == {
        "src.callbacks.ForwardSpectralNorm": "sota_imagenet_amd.callbacks.ForwardSpectralNorm",
        "sota_imagenet.callbacks.ForwardSpectralNorm": "sota_imagenet_amd.callbacks.ForwardSpectralNorm",
    }
    for k in C.FORWARD_SPECTRAL_CALLBACK_TARGET_ALIASES:
        assert C.resolve_target(k) is callbacks.ForwardSpectralNorm
    cb = C.call({"_target_": "src.callbacks.ForwardSpectralNorm", "seed": 3})
    assert isinstance(cb, callbacks.ForwardSpectralNorm) and cb.seed == 3
    assert C.resolve_target("src.callbacks.ForwardWeightNorm") is callbacks.ForwardWeightNorm  # (the tables in front still resolve)


def test_smoke_config_is_the_test_config_plus_the_callback():
    from sota_imagenet_amd import callbacks, config as C

    a, b = C.to_plain(C.compose(None, ["+hydra_exp=sn_test"])), C.to_plain(C.compose(None, ["+hydra_exp=test"]))
    extra = a["run"].pop("extra_callbacks")
    base_extra = b["run"].pop("extra_callbacks")
    for d in (a, b):
        d["log"].pop("exp_name")
    assert a == b, "the baseline's test config plus the callbacks, nothing else"
    added = [e for e in extra if e not in base_extra]
    assert [e["_target_"] for e in added] == ["src.callbacks.OrthoInitClb", "src.callbacks.ForwardSpectralNorm"], "behind OrthoInitClb, as recipe 29"
    assert isinstance(C.call(added[1]), callbacks.ForwardSpectralNorm)
