"""Adam / AdamW on the host: the reference's optimizer targets resolve to the native classes, the C-ABI entries refuse bad
arguments with a status and a message before any launch, and the constructor refuses what is not on the hot path."""
import ctypes

import pytest
import torch

from sota_imagenet_amd import config as C
from sota_imagenet_amd import native


def test_adam_targets_resolve_to_the_native_classes():
    from sota_imagenet_amd import optim

    for target in ("torch.optim._multi_tensor.AdamW", "torch.optim.AdamW"):
        assert C.resolve_target(target) is optim.AdamW
    for target in ("torch.optim._multi_tensor.Adam", "torch.optim.Adam"):
        assert C.resolve_target(target) is optim.Adam
    # un-vendored: stays unaliased
    assert "pytorch_tools.optim.adamw.AdamW" not in C.TARGET_ALIASES


def test_adamw_configs_compose():
    cfg = C.compose(None, ["+hydra_exp=r50_adamw"])
    assert cfg.optim._target_ == "torch.optim._multi_tensor.AdamW" and cfg.optim.weight_decay == 5e-2 and cfg.optim.lr == 0
    assert cfg.loader.batch_size == 256 and cfg.loader.image_size == 224 and cfg.criterion.smoothing == 0.1
    assert cfg.loader.random_interpolation is True and cfg.loader.color_twist_prob == 0.4
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 8, [0, 0.001], "linear"), (8, 90, [0.001, 0], "cos")]
    cfg = C.compose(None, ["+hydra_exp=adamw_test"])
    assert "momentum" not in C.to_plain(cfg.optim) and cfg.log.exp_name == "adamw_test"


def _adam(L, p=4096, g=4096, m=4096, v=4096, ema=None, b1=0.9, b2=0.999, eps=1e-8, ema_decay=0.99):
    # n = 0: even a call that passed validation would touch no memory (these addresses are never dereferenced)
    P = ctypes.c_void_p
    args = [P(p), P(g), P(m), P(v)]
    tail = [0, b1, b2, eps, 1e-3, 0.03, 1e-3, 5e-2, 1, 1.0]
    if ema is None:
        return L.mi355_adam_step(*args, *tail, None)
    return L.mi355_adam_step_ema(*args, P(ema), *tail, ema_decay, None)


def test_adam_bad_arguments_return_status_not_crash():
    L = native.lib()
    assert _adam(L, p=4096 + 4) == -1 and "aligned" in native.last_error()
    assert _adam(L, ema=4096 + 8) == -1 and "aligned" in native.last_error()
    assert _adam(L, g=0) == -1 and "null" in native.last_error()
    assert _adam(L, b1=1.0) == -1 and "beta1" in native.last_error()
    assert _adam(L, b2=-0.1) == -1 and "beta2" in native.last_error()
    assert _adam(L, eps=-1e-8) == -1 and "eps" in native.last_error()
    assert _adam(L, eps=float("inf")) == -1 and "eps" in native.last_error()
    assert _adam(L, ema=4096, ema_decay=2.0) == -1 and "ema_decay" in native.last_error()
    P = ctypes.c_void_p
    rc = L.mi355_adam_step_ema(P(4096), P(4096), P(4096), P(4096), None, 0, 0.9, 0.999, 1e-8, 1e-3, 0.03, 1e-3, 5e-2, 1, 1.0, 0.9, None)
    assert rc == -1 and "null ema" in native.last_error()


def test_adam_constructor_refuses_what_is_not_on_the_hot_path():
    from sota_imagenet_amd import optim

    ps = [torch.nn.Parameter(torch.zeros(4))]
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(NotImplementedError):
            cls(ps, amsgrad=True)
        with pytest.raises(NotImplementedError):
            cls(ps, maximize=True)
        with pytest.raises(NotImplementedError):
            cls(ps, lr=torch.tensor(1e-3))
        with pytest.raises(ValueError):
            cls(ps, betas=(1.0, 0.999))
        cls(ps, foreach=True, fused=False, capturable=True, differentiable=False)  # accepted and ignored


def test_adam_defaults_and_group_keys_are_torchs():
    from sota_imagenet_amd import optim

    ps = [torch.nn.Parameter(torch.zeros(4))]
    for cls, ref in ((optim.Adam, torch.optim.Adam), (optim.AdamW, torch.optim.AdamW)):
        ours, theirs = cls(ps).param_groups[0], ref(ps).param_groups[0]
        assert set(ours) == set(theirs)
        for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "decoupled_weight_decay"):
            assert ours[k] == theirs[k], k
