"""The host side of the forward weight transform: the factory routing of weight_standardization, the ForwardWeightNorm callback's refusals, its
alias table, the smoke config, the row plan and the declared entry points.  No GPU."""
import os
import re

import pytest
import torch

import weight_std_common as WS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_flag_alone_gives_the_plain_model():
    from sota_imagenet_amd.models import ResNet50, resnet50

    m = resnet50(weight_standardization=True, num_classes=10)
    assert type(m) is ResNet50 and m.weight_transform == WS.STANDARDISE
    assert resnet50(num_classes=10).weight_transform == 0 and resnet50(weight_standardization=False, num_classes=10).weight_transform == 0
    # the raw weights are what parameters() and state_dict() hold: the flag changes neither names nor values
    plain = resnet50(num_classes=10).state_dict()
    sd = m.state_dict()
    assert list(sd) == list(plain) and all(torch.equal(sd[k], plain[k]) for k in sd)
    # a variant key still routes to BResNet-50, with or without the flag
    kw = dict(stem_type="deep", antialias=True, attn_type="eca", norm_act="leaky_relu")
    assert type(resnet50(weight_standardization=True, **kw)).__name__ == "BResNet50"
    assert type(resnet50(**kw)).__name__ == "BResNet50"
    with pytest.raises(NotImplementedError):
        resnet50(weight_standardization=True, stem_type="space2depth")


def test_set_weight_transform_domain_and_fp8():
    from sota_imagenet_amd.models import resnet50

    m = resnet50(num_classes=10)
    for mode, want in (("standardise", 1), ("centre", 2), ("off", 0), (1, 1), (2, 2), (0, 0)):
        m.set_weight_transform(mode)
        assert m.weight_transform == want
    for bad in (3, -1, "std", True, None):
        with pytest.raises(ValueError):
            m.set_weight_transform(bad)
    with pytest.raises(ValueError):
        resnet50(num_classes=10, dtype="fp8", weight_standardization=True)
    f8 = resnet50(num_classes=10, dtype="fp8")
    with pytest.raises(ValueError):
        f8.set_weight_transform("centre")
    f8.set_weight_transform("off")


def test_train_config_with_the_flag_builds_the_plain_model():
    """what train.py does with configs/hydra_exp/ws_test.yaml: the flag travels into the model factory"""
    from sota_imagenet_amd import config as C

    cfg = C.compose(None, ["+hydra_exp=ws_test"])
    base = C.compose(None, ["+hydra_exp=test"])
    assert cfg.weight_standardization is True and base.weight_standardization is False
    a, b = C.to_plain(cfg), C.to_plain(base)
    for d in (a, b):
        d.pop("weight_standardization")
        d["log"].pop("exp_name")
    assert a == b, "the baseline's test config plus the flag, nothing else"
    model_cfg = C.to_plain(cfg.model)
    model_cfg["weight_standardization"] = bool(cfg.weight_standardization)
    model_cfg["dtype"] = "bf16"
    m = C.call(model_cfg)
    assert type(m).__name__ == "ResNet50" and m.weight_transform == WS.STANDARDISE


def test_callback_refusals():
    from sota_imagenet_amd.bresnet import BResNet50
    from sota_imagenet_amd.callbacks import ForwardWeightNorm
    from sota_imagenet_amd.fit_wrapper import RunnerState
    from sota_imagenet_amd.models import resnet50

    with pytest.raises(NotImplementedError, match="normalize_conv_weight"):
        ForwardWeightNorm(gamma=1.7, use_std=True)
    cb = ForwardWeightNorm()
    assert cb.use_std is False and ForwardWeightNorm(gamma=1.7).gamma == 1.7
    # not a flat model / a flat model on the CPU / the variant graph: no module walk, no CPU path
    for model in (torch.nn.Conv2d(3, 8, 3), resnet50(num_classes=10), BResNet50(num_classes=10)):
        cb.set_state(RunnerState(model=model))
        with pytest.raises(NotImplementedError):
            cb.on_begin()
        with pytest.raises(NotImplementedError):
            cb.on_end()


def test_alias_table():
    from sota_imagenet_amd import callbacks, config as C

    assert C.FORWARD_WEIGHT_CALLBACK_TARGET_ALIASES == {
        "src.callbacks.ForwardWeightNorm": "sota_imagenet_amd.callbacks.ForwardWeightNorm",
        "sota_imagenet.callbacks.ForwardWeightNorm": "sota_imagenet_amd.callbacks.ForwardWeightNorm",
    }
    for k in C.FORWARD_WEIGHT_CALLBACK_TARGET_ALIASES:
        assert C.resolve_target(k) is callbacks.ForwardWeightNorm
    cb = C.call({"_target_": "src.callbacks.ForwardWeightNorm", "use_std": False})
    assert isinstance(cb, callbacks.ForwardWeightNorm)
    assert C.resolve_target("src.callbacks.WeightNorm") is callbacks.WeightNorm  # (the tables in front still resolve)


def test_row_plan_covers_every_conv_filter_once():
    from sota_imagenet_amd import item_plan
    from sota_imagenet_amd.models import resnet50

    m = resnet50(num_classes=10)
    rows = item_plan.ws_rows(m._table)
    assert len(rows) == 26560 and sum(L for _, L in rows) == 23454912
    assert sorted({L for _, L in rows})[:3] == [64, 128, 147] and max(L for _, L in rows) == 4608
    spans = sorted(rows)
    assert all(a + la <= b for (a, la), (b, _) in zip(spans, spans[1:])), "no two rows overlap"
    by_off = {off: shape for _, kind, off, shape in m._table if kind == 0}
    fc = next(off for name, kind, off, shape in m._table if name == "fc.weight")
    assert all(not (fc <= o < fc + 10 * 2048) for o, _ in rows), "the FC is no conv"
    stem = next((off, shape) for name, kind, off, shape in m._table if name == "conv1.weight")
    assert (stem[0], 147) in rows and (stem[0] + 63 * 147, 147) in rows and by_off[stem[0]] == (64, 3, 7, 7)
    packed = item_plan.pack_records(rows[:3])
    assert packed.shape == (3, 2) and packed[1, 0].item() == rows[1][0] and packed[1, 1].item() == 147  # { int64 off; int32 len; int32 0 }


def test_header_declares_the_entry_points():
    from sota_imagenet_amd import native

    protos = native.parse_header()
    ret, params = protos["mi355_resnet50_set_weight_transform"]
    assert ret == "int" and len(params) == 2 and params[0].startswith("mi355_ctx") and params[1] == "int mode"
    assert len(protos["mi355_weight_std_rows_fwd"][1]) == 9 and len(protos["mi355_weight_std_rows_bwd"][1]) == 11
    # the creation call keeps its prototype
    assert len(protos["mi355_resnet50_create"][1]) == 7
    # the per-layer kernels BResNet-50 uses stay declared as they were
    assert len(protos["mi355_weight_std_fwd"][1]) == 8 and len(protos["mi355_weight_std_bwd"][1]) == 8
    src = open(os.path.join(ROOT, "sota_imagenet_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bweight_std\.hip\b", src, re.M)


def test_the_constants_of_host_and_header_agree():
    """the mode codes and the epsilon are stated once per side: ops for the host, include/mi355rn.h for the library and the executor"""
    from sota_imagenet_amd import ops

    text = open(os.path.join(ROOT, "include", "mi355rn.h")).read()
    macros = dict(re.findall(r"^#define\s+(MI355_WS_\w+)\s+(\S+)", text, re.M))
    assert set(macros) == {"MI355_WS_STANDARDISE", "MI355_WS_CENTRE", "MI355_WS_EPS"}
    assert int(macros["MI355_WS_STANDARDISE"]) == ops.WS_STANDARDISE == WS.STANDARDISE == 1
    assert int(macros["MI355_WS_CENTRE"]) == ops.WS_CENTRE == WS.CENTRE == 2
    assert macros["MI355_WS_EPS"].endswith("f") and float(macros["MI355_WS_EPS"][:-1]) == ops.WS_EPS == WS.EPS
    # nothing in the library's sources restates them
    csrc = os.path.join(ROOT, "sota_imagenet_amd", "csrc")
    for name in ("weight_std.hip", "resnet_exec.cpp"):
        src = open(os.path.join(csrc, name)).read()
        assert "MI355_WS_STANDARDISE" in src and not re.search(r"\bWS_EPS\s*=|mode\s*==\s*[12]\b", src), name


def test_layout_only_and_argument_refusals_of_the_entry_points():
    import ctypes

    from sota_imagenet_amd import native

    L = native.lib()
    c = ctypes.c_void_p()
    native.check(L.mi355_resnet50_create(ctypes.byref(c), -1, native.F32, 2, 64, 64, 10))
    try:
        assert L.mi355_resnet50_set_weight_transform(None, 1) == -1
        assert L.mi355_resnet50_set_weight_transform(c, 3) == -1 and L.mi355_resnet50_set_weight_transform(c, -1) == -1
        assert L.mi355_resnet50_set_weight_transform(c, 0) == 0
        assert L.mi355_resnet50_set_weight_transform(c, 1) == -3 and "layout-only" in native.last_error()  # no device, no scratch
    finally:
        L.mi355_resnet50_destroy(c)
    native.check(L.mi355_resnet50_create(ctypes.byref(c), -1, native.FP8, 2, 64, 64, 10))
    try:
        assert L.mi355_resnet50_set_weight_transform(c, 2) == -1 and "fp8" in native.last_error()
        assert L.mi355_resnet50_set_weight_transform(c, 0) == 0
    finally:
        L.mi355_resnet50_destroy(c)
    # the row launchers check their arguments before any launch (dummy pointers, never dereferenced)
    p = torch.zeros(64).data_ptr()
    assert L.mi355_weight_std_rows_fwd(p, p, p, 64, p, 1, 0, 1e-5, None) == -1 and "mode" in native.last_error()
    assert L.mi355_weight_std_rows_fwd(p, p, p, 64, None, 1, 1, 1e-5, None) == -1
    assert L.mi355_weight_std_rows_fwd(p + 4, p, p, 64, p, 1, 1, 1e-5, None) == -1 and "misaligned" in native.last_error()
    assert L.mi355_weight_std_rows_fwd(p, p, p, 64, p, 0, 1, 1e-5, None) == -1
    assert L.mi355_weight_std_rows_bwd(p, p + 16, p, p, 64, p, 0, 1, 1, 0.0, None) == -1 and "dw" in native.last_error()
    assert L.mi355_weight_std_rows_bwd(p, p + 16, p, p + 32, 64, p, 1, 1, 1, 0.0, None) == -1


def test_float64_rules_reproduce_the_parametrised_gradients():
    """the row formulas the kernels implement, against torch's own autograd through the parametrisation (float64, one small conv)"""
    import numpy as np

    torch.manual_seed(0)
    w = torch.randn(5, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    x = torch.randn(2, 3, 8, 8, dtype=torch.float64)
    for mode in (WS.STANDARDISE, WS.CENTRE):
        t = WS._Transform(mode)
        w.grad = None
        w_hat = t(w)
        w_hat.retain_grad()
        torch.nn.functional.conv2d(x, w_hat, padding=1).square().sum().backward()
        g, wh = w_hat.grad.reshape(5, -1).numpy(), w_hat.detach().reshape(5, -1).numpy()
        for r in range(5):
            row = w.detach().reshape(5, -1).numpy()[r]
            mu = row.mean()
            inv = 1.0 / np.sqrt(max((row * row).mean() - mu * mu, 0.0) + WS.EPS) if mode == WS.STANDARDISE else 1.0
            assert np.allclose((row - mu) * inv, wh[r], rtol=0, atol=1e-12)
            m1 = g[r].mean()
            m2 = (g[r] * wh[r]).mean() if mode == WS.STANDARDISE else 0.0
            ref = inv * (g[r] - m1 - wh[r] * m2)
            assert np.allclose(ref, w.grad.reshape(5, -1).numpy()[r], rtol=1e-10, atol=1e-12)
