"""Orthogonal initialisation (sota_imagenet_amd.callbacks.OrthoInitClb, csrc/init_ortho.hip) without a GPU: the planner on the two executors'
layout-only tables, the record packing, the target tables and the config files of recipe 53, the entry point's validation and the callback's
refusal of a CPU model."""
import ctypes

import numpy as np
import pytest
import torch

import exec_gpu_common as E
from sota_imagenet_amd import config as C
from sota_imagenet_amd import item_plan, native
from sota_imagenet_amd.fit_wrapper import RunnerState


def test_records_of_the_resnet50_table():
    m = E.resnet50()
    recs = item_plan.ortho_records(m._table)
    by_name = {name: (kind, off, shape) for name, kind, off, shape in m._table}
    assert len(recs) == 54  # 53 convolutions and the FC
    by_off = {off: name for name, (kind, off, shape) in by_name.items() if kind == 0}
    names = [by_off[r[0]] for r in recs]
    assert [r[0] for r in recs] == [off for _, kind, off, shape in m._table if kind == 0 and len(shape) in (2, 4)]  # table order
    assert recs[names.index("conv1.weight")][1:] == (64, 3, 49)
    assert recs[names.index("fc.weight")] == (by_name["fc.weight"][1], 1000, 2048, 1)
    assert recs[names.index("layer1.0.conv1.weight")][1:] == (64, 64, 1) and recs[names.index("layer4.0.conv2.weight")][1:] == (512, 512, 9)
    assert all(n.endswith(".weight") and ("conv" in n or "downsample.0" in n or n == "fc.weight") for n in names)
    assert "fc.bias" not in names and not any("bn" in n or "downsample.1" in n for n in names)
    # the records lie inside the flat array, apart from each other, and fc.weight's record ends where its padding rows begin
    spans = sorted((off, off + r * c * t) for off, r, c, t in recs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= m._nparam
    assert (1000 * 2048) % 128 == 0 and m.fc.weight.shape == (1000, 2048)


def test_records_of_the_bresnet50_table():
    m = E.bresnet50()
    recs = item_plan.ortho_records(m._table)
    shapes = {off: (name, shape) for name, kind, off, shape in m._table if kind == 0}
    assert any(len(sh) == 3 for _, sh in shapes.values())  # the ECA weights exist ...
    assert all(len(shapes[r[0]][1]) in (2, 4) for r in recs)  # ... and none is planned
    assert len(recs) == sum(len(sh) in (2, 4) for _, sh in shapes.values())
    first = recs[[shapes[r[0]][1] for r in recs].index((32, 3, 3, 3))]  # the deep stem's first convolution, 32 x 27
    assert first[1:] == (32, 3, 9) and first[1] >= first[2] * first[3]  # tall with taps = 9: the vectors are the columns in logical order


def test_hand_made_table_and_packing():
    table = [("a.weight", 0, 0, (8, 4, 3, 3)), ("a.bn.weight", 0, 320, (8,)), ("a.bn.running_mean", 1, 0, (8,)), ("e.weight", 0, 384, (1, 1, 5)),
             ("fc.weight", 0, 448, (10, 32)), ("fc.bias", 0, 1472, (10,)), ("buf.weight", 1, 64, (4, 4))]
    recs = item_plan.ortho_records(table)
    assert recs == [(0, 8, 4, 9), (448, 10, 32, 1)]
    t = item_plan.pack_records(recs, None, item_plan.ORTHO_FIELDS)
    assert t.dtype == torch.int64 and tuple(t.shape) == (2, 3)
    raw = np.frombuffer(t.numpy().tobytes(), dtype=np.dtype([("off", "<i8"), ("rows", "<i4"), ("chans", "<i4"), ("taps", "<i4"), ("pad", "<i4")]))
    assert [tuple(int(x) for x in r) for r in raw] == [(0, 8, 4, 9, 0), (448, 10, 32, 1, 0)]
    # the default packing is what it was: 16-byte records as [n, 2]
    assert tuple(item_plan.pack_records([(0, 5, 1), (64, 7, 2)]).shape) == (2, 2)


def test_targets():
    from sota_imagenet_amd import callbacks

    assert C.INIT_CALLBACK_TARGET_ALIASES == {"src.callbacks.OrthoInitClb": "sota_imagenet_amd.callbacks.OrthoInitClb",
                                              "sota_imagenet.callbacks.OrthoInitClb": "sota_imagenet_amd.callbacks.OrthoInitClb"}
    for spelling in C.INIT_CALLBACK_TARGET_ALIASES:
        assert C.resolve_target(spelling) is callbacks.OrthoInitClb
    # the four older tables are what they were
    assert C.TARGET_ALIASES == {
        "pytorch_tools.models.resnet50": "sota_imagenet_amd.models.resnet50",
        "pytorch_tools.losses.smooth.CrossEntropyLoss": "sota_imagenet_amd.losses.CrossEntropyLoss",
        "pytorch_tools.losses.CrossEntropyLoss": "sota_imagenet_amd.losses.CrossEntropyLoss",
        "torch.optim._multi_tensor.SGD": "sota_imagenet_amd.optim.SGD",
        "torch.optim.SGD": "sota_imagenet_amd.optim.SGD",
        "torch.optim._multi_tensor.AdamW": "sota_imagenet_amd.optim.AdamW",
        "torch.optim.AdamW": "sota_imagenet_amd.optim.AdamW",
        "torch.optim._multi_tensor.Adam": "sota_imagenet_amd.optim.Adam",
        "torch.optim.Adam": "sota_imagenet_amd.optim.Adam",
        "src.optimizers.MADGRAD": "sota_imagenet_amd.optim.MADGRAD",
        "sota_imagenet.optimizers.MADGRAD": "sota_imagenet_amd.optim.MADGRAD",
        "src.optimizers.AdaiS": "sota_imagenet_amd.optim.AdaiS",
        "sota_imagenet.optimizers.AdaiS": "sota_imagenet_amd.optim.AdaiS",
        "pytorch_tools.fit_wrapper.callbacks.Callback": "sota_imagenet_amd.fit_wrapper.Callback",
        "pytorch_tools.fit_wrapper.callbacks.Cutmix": "sota_imagenet_amd.callbacks.Cutmix",
        "pytorch_tools.fit_wrapper.callbacks.Mixup": "sota_imagenet_amd.callbacks.Mixup",
        "sota_imagenet.callbacks.CutmixMixup": "sota_imagenet_amd.callbacks.CutmixMixup",
    }
    assert C.LAYERWISE_TARGET_ALIASES == {f"{pre}.optimizers.{name}": f"sota_imagenet_amd.optim.{name}"
                                          for name in ("NovogradApex", "MyNovograd", "AdamLayerwise", "MyAdai") for pre in ("src", "sota_imagenet")}
    assert C.CALLBACK_TARGET_ALIASES == {f"{pre}.callbacks.{name}": f"sota_imagenet_amd.callbacks.{name}"
                                         for name in ("SAMOriginal", "SAM") for pre in ("src", "sota_imagenet")}
    assert C.ADAMP_TARGET_ALIASES == {"adamp.AdamP": "sota_imagenet_amd.optim.AdamP"}


def test_recipe_53_and_its_smoke_config():
    from sota_imagenet_amd import callbacks

    cfg = C.compose(None, ["+hydra_exp=r50_adamw_rep"])
    got = C.to_plain(cfg.optim)
    assert got.pop("_target_") == "torch.optim._multi_tensor.AdamW" and got == dict(weight_decay=2e-2, lr=0)
    assert cfg.log.exp_name == "r50_adamw_repeat_ortho-init" and cfg.init_gamma == 1.7 and cfg.criterion.smoothing == 0.1
    assert cfg.loader.batch_size == 192 and cfg.loader.image_size == 224 and cfg.loader.color_twist_prob == 0.3
    assert [(s["start"], s["end"], s["lr"], s["lr_mode"]) for s in cfg.run.stages] == [(0, 8, [0, 0.002], "linear"), (8, 90, [0.002, 0], "cos")]
    want = [{"_target_": "src.callbacks.OrthoInitClb"}, {"_target_": "pytorch_tools.fit_wrapper.callbacks.Callback"}]
    assert C.to_plain(cfg.run.extra_callbacks) == want
    test = C.compose(None, ["+hydra_exp=adamw_rep_test"])
    assert C.to_plain(test.run.extra_callbacks) == want and C.to_plain(test.optim) == C.to_plain(cfg.optim) and test.init_gamma == 1.7
    assert test.log.exp_name == "adamw_rep_test" and test.debug is True and test.loader.image_size == 64 and test.loader.batch_size == 16
    assert [(s["start"], s["end"]) for s in test.run.stages] == [(0, 1), (1, 2)]
    for c in (cfg, test):
        made = [C.call(cb) for cb in c.run.extra_callbacks]
        assert type(made[0]) is callbacks.OrthoInitClb and made[0].gain == 1 and made[0].has_been_init is False
    assert C.call({"_target_": "sota_imagenet.callbacks.OrthoInitClb", "gain": 1.7}).gain == 1.7


def test_a_cpu_model_is_refused():
    from sota_imagenet_amd.callbacks import OrthoInitClb

    for model in (E.resnet50(), torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.Linear(8, 4))):
        before = [p.detach().clone() for p in model.parameters()]
        cb = OrthoInitClb()
        cb.set_state(RunnerState(model=model))
        for call in (cb.on_begin, cb.fill, cb.orthogonalise):
            with pytest.raises(NotImplementedError, match="no CPU path"):
                call()
        assert cb.has_been_init is False
        assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))


def test_runner_records_the_start_epoch():
    from sota_imagenet_amd import fit_wrapper as fw

    seen = []

    class Spy(fw.Callback):
        def on_begin(self):
            seen.append(self.state.start_epoch)

    model = torch.nn.Linear(4, 2)
    runner = fw.Runner(model, torch.optim.SGD(model.parameters(), lr=0.1), torch.nn.CrossEntropyLoss(), callbacks=[Spy()])
    loader = [(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long))]
    runner.fit(loader, epochs=1)
    runner.fit(loader, epochs=3, start_epoch=2)
    assert seen == [0, 2]


P = ctypes.c_void_p


def test_entry_point_returns_status_on_bad_arguments():
    """every call here fails validation before any launch (the addresses are never dereferenced)"""
    L = native.lib()
    assert L.mi355_ortho_init.restype is ctypes.c_int
    A = 4096

    def call(w=A, n=64, mats=A, n_mats=1, gain=1.0, status=A):
        return L.mi355_ortho_init(P(w), n, P(mats), n_mats, gain, P(status), None)

    for bad in (dict(w=None), dict(mats=None), dict(status=None), dict(w=A + 2), dict(mats=A + 4), dict(status=A + 1), dict(n=0), dict(n_mats=0),
                dict(n_mats=(1 << 20) + 1), dict(gain=float("inf")), dict(gain=float("nan"))):
        assert call(**bad) == -1, bad
        assert "ortho_init" in native.last_error()


def test_the_wrapper_checks_its_arguments_before_the_library_is_asked():
    from sota_imagenet_amd import ops

    flat = torch.zeros(64)
    recs = [(0, 2, 4, 1)]
    with pytest.raises(ValueError):  # a CPU array
        ops.ortho_init_(flat, recs, item_plan.pack_records(recs, None, item_plan.ORTHO_FIELDS), 1.0)
