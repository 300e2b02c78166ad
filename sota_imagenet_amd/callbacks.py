"""Callbacks next to the hot path: Mixup / CutMix / CutmixMixup on device, producing the soft targets the native cross
entropy consumes, and SAMOriginal / SAM (sharpness-aware minimization), which sit on the step itself.

Re-states sota_imagenet/callbacks.py:232-247 (`CutmixMixup`: coin flip between `self.cutmix(*input)` and
`self.mixup(*input)` with Beta(alpha, alpha) samplers) and the un-vendored pt_clb.Cutmix / pt_clb.Mixup bases as
SURVEY.md Appendix C records them (mix with the PREVIOUS batch, permuted; CutMix target weight = real box area).
SAMOriginal re-states sota_imagenet/callbacks.py:279-337 over csrc/optim_sam.hip, SAM :339-420 over csrc/optim_sam_lw.hip, OrthoInitClb :250-266
over csrc/init_ortho.hip, GradDistributionTB :30-60 over csrc/optim_hist.hip, WeightDistributionTB :11-17 over csrc/optim_wdist.hip, WeightNorm :104-123 over csrc/weight_norm.hip,
ForwardWeightNorm :62-84 over csrc/weight_std.hip and the executor's weight transform, ForwardSpectralNorm :87-101 over csrc/spectral_norm.hip,
OrthoLossClb :191-203 and NormLossClb :224-229 over losses.OrthoLoss / NormLoss and csrc/ortho_loss.hip.
What these share is stated once at module level: the flat model a callback runs on and its parameters by offset (_flat_model_of, _params_by_offset:
OrthoInitClb, WeightNorm), and for the two histogram callbacks the re-plan key of a tensor (_tensor_key), the one-device check (_one_device) and the
way out to state.tb_logger (_log_histograms); their launches per storage come from item_plan.dist_plan over item_plan.storage_array.
"""

import logging
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .fit_wrapper import Callback, _unwrap, env_rank
from . import item_plan
from .item_plan import flat_views, pack_records, place, storage_pairs


class _DeviceMixer:
    """the native path (csrc/mix.hip through the C-ABI): decisions sampled ON the device from (seed, batch counter), one
    float4 kernel mixes images and soft targets with the previous batch; nothing comes back to the host."""

    def __init__(self, seed=0):
        self.seed = int(seed)
        self.counter = 0
        self.key = None

    def reseed(self, random_seed, rank):
        """one stream per (run seed, rank): the reference draws from per-process np.random / torch generators, so ranks must
        not share their coins, lambdas, boxes and permutations"""
        self.seed = (int(random_seed or 0) * 1000003 + int(rank) * 7919 + 12345) & 0x7FFFFFFF

    def params_tensor(self):
        return self.params

    def __call__(self, data, target, cutmix_alpha, mixup_alpha, prob, allow):
        from . import native

        L = native.lib()
        if data.dtype != torch.float32 or target.dtype != torch.float32:
            raise TypeError(f"Mixup / CutMix on the device take float32 images and float32 soft targets (got {data.dtype}, {target.dtype})")
        data, target = data.contiguous(), target.contiguous()
        N, C, H, W = data.shape
        key = (tuple(data.shape), tuple(target.shape), data.device)
        if key != self.key:  # first batch / stage change: the "previous" batch is the batch itself (permuted)
            self.prev = [data.clone(), torch.empty_like(data)]
            self.tprev = [target.clone(), torch.empty_like(target)]
            self.params = torch.zeros(L.mi355_mix_params_bytes(N), dtype=torch.uint8, device=data.device)
            self.cur = 0
            self.key = key
        out, tout = torch.empty_like(data), torch.empty_like(target)
        st = native.cur_stream()
        native.check(L.mi355_mix_sample(native.ptr(self.params), self.seed, self.counter, N, H, W, float(cutmix_alpha), float(mixup_alpha),
                                        float(prob), int(allow), st))
        i, o = self.cur, self.cur ^ 1
        native.check(L.mi355_mix_apply(native.ptr(data), native.ptr(out), native.ptr(self.prev[i]), native.ptr(self.prev[o]),
                                       native.ptr(target), native.ptr(tout), native.ptr(self.tprev[i]), native.ptr(self.tprev[o]),
                                       native.ptr(self.params), N, C, H, W, target.shape[1], st))
        self.cur = o
        self.counter += 1
        return out, tout


class Mixup(Callback):
    def __init__(self, alpha, num_classes=1000, prob=0.5, seed=None):
        super().__init__()
        self._seed_given = seed is not None
        seed = seed or 0
        self.alpha = float(alpha)
        self.tb = torch.distributions.Beta(alpha, alpha)
        self.num_classes = num_classes
        self.prob = prob
        self.prev_input = None
        self._dev = _DeviceMixer(seed)

    def on_begin(self):
        if not self._seed_given:  # an explicit seed= stays; otherwise (run seed, rank) -> one stream per process
            self._dev.reseed(getattr(self.state, "random_seed", 0), self.state.rank)

    def on_loader_begin(self):
        # the sampler's position is a function of (epoch, step): a resumed run continues the sequence instead of replaying it
        if self.state.is_train and self.state.epoch_size:
            self._dev.counter = int(self.state.epoch) << 32  # (epoch, step) kept apart: epoch_size changes between progressive-resize stages

    def _onehot(self, target):
        if target.dim() == 1:
            return torch.nn.functional.one_hot(target.long(), self.num_classes).float()
        return target.float()

    def on_batch_begin(self):
        if self.state.is_train:
            self.state.input = self.mixup(*self.state.input)

    @torch.no_grad()
    def mixup(self, data, target):
        target = self._onehot(target)
        if data.is_cuda:  # the hot path: HIP kernels; the torch code below serves CPU tensors (host-logic tests) only
            a = float(self.tb.concentration1)
            return self._dev(data, target, a, a, self.prob, allow=1)
        if self.prev_input is None or self.prev_input[0].shape != data.shape:
            self.prev_input = (data.clone(), target.clone())
        if np.random.rand() > self.prob:
            self.prev_input = (data.clone(), target.clone())
            return data, target
        prev_data, prev_target = self.prev_input
        self.prev_input = (data.clone(), target.clone())
        perm = torch.randperm(data.size(0), device=data.device)
        c = float(self.tb.sample())
        return c * data + (1 - c) * prev_data[perm], c * target + (1 - c) * prev_target[perm]


class Cutmix(Mixup):
    def on_batch_begin(self):
        if self.state.is_train:
            self.state.input = self.cutmix(*self.state.input)

    @torch.no_grad()
    def cutmix(self, data, target):
        target = self._onehot(target)
        if data.is_cuda:
            a = float(self.tb.concentration1)
            return self._dev(data, target, a, a, self.prob, allow=2)
        if self.prev_input is None or self.prev_input[0].shape != data.shape:
            self.prev_input = (data.clone(), target.clone())
        if np.random.rand() > self.prob:
            self.prev_input = (data.clone(), target.clone())
            return data, target
        prev_data, prev_target = self.prev_input
        self.prev_input = (data.clone(), target.clone())
        _, _, H, W = data.shape
        lam = float(self.tb.sample())
        lam = min(lam, 1 - lam)
        bh, bw = int(H * np.sqrt(lam)), int(W * np.sqrt(lam))
        cy, cx = np.random.randint(H), np.random.randint(W)
        y1, y2 = np.clip(cy - bh // 2, 0, H), np.clip(cy + bh // 2, 0, H)
        x1, x2 = np.clip(cx - bw // 2, 0, W), np.clip(cx + bw // 2, 0, W)
        perm = torch.randperm(data.size(0), device=data.device)
        data = data.clone()
        data[:, :, y1:y2, x1:x2] = prev_data[perm][:, :, y1:y2, x1:x2]
        lam_real = float((y2 - y1) * (x2 - x1)) / (H * W)
        return data, (1 - lam_real) * target + lam_real * prev_target[perm]


class CutmixMixup(Cutmix):
    """sota_imagenet/callbacks.py:232-247."""

    def __init__(self, cutmix_alpha, mixup_alpha, prob=0.5, num_classes=1000, seed=None):
        super().__init__(cutmix_alpha, num_classes, prob, seed)
        self.cutmix_tb = torch.distributions.Beta(cutmix_alpha, cutmix_alpha)
        self.mixup_tb = torch.distributions.Beta(mixup_alpha, mixup_alpha)

    def on_batch_begin(self):
        if not self.state.is_train:
            return
        data, target = self.state.input
        if data.is_cuda:  # the coin of callbacks.py:242 is drawn on the device too (mi355_mix_sample, allow = both)
            self.state.input = self._dev(data, self._onehot(target), float(self.cutmix_tb.concentration1),
                                         float(self.mixup_tb.concentration1), self.prob, allow=3)
            return
        if np.random.rand() > 0.5:
            self.tb = self.cutmix_tb
            self.state.input = self.cutmix(*self.state.input)
        else:
            self.tb = self.mixup_tb
            self.state.input = self.mixup(*self.state.input)


def _flat_model_of(state, who):
    """state.model unwrapped, if it is a flat-array model on a CUDA device: what callback `who` runs on; NotImplementedError in its name otherwise"""
    from .models import _FlatModel

    m = _unwrap(state.model)
    if not isinstance(m, _FlatModel) or not m.flat_params.is_cuda:
        raise NotImplementedError(f"{who} runs on a flat-array model (models.resnet50) on a CUDA device: there is no CPU path and no "
                                  f"module walk (got {type(m).__name__} on {getattr(getattr(m, 'flat_params', None), 'device', 'no flat array')})")
    return m


def _params_by_offset(m):
    """{offset in the flat array: (name, parameter)} of the flat model m"""
    return {off: (f"{m._name_of(leaf)}.{attr}", leaf._parameters[attr]) for leaf, attr, kind, off, _ in m._entries if kind == 0}


def _tensor_key(t):
    """what a histogram callback's plan depends on of a tensor: a change of any of these rebuilds it"""
    return t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype, t.device


def _one_device(who, what, tensors):
    """the device that all `tensors` live on; RuntimeError in the name of callback `who` if there is more than one"""
    devs = {t.device for t in tensors}
    if len(devs) != 1:
        raise RuntimeError(f"{who}: {what} must live on one device (got {sorted(map(str, devs))})")
    return devs.pop()


def _log_histograms(state, last, raw):
    """a callback's `last` to state.tb_logger at state.global_sample_step, if there is one: raw(value of a tag) -> (min, max, num, sum, sum_squares,
    bucket_limits, bucket_counts), the arguments of add_histogram_raw"""
    if state.tb_logger is not None:
        for tag, v in last.items():
            *stats, limits, counts = raw(v)
            state.tb_logger.add_histogram_raw(tag, *stats, bucket_limits=limits, bucket_counts=counts, global_step=state.global_sample_step)


class OrthoInitClb(Callback):
    """sota_imagenet/callbacks.py:250-266 (recipes 46-48, 50-53, 55): orthogonal initialisation of every conv and FC weight, once per process at the
    first on_begin (`has_been_init`: fit runs once per stage).  For a weight [O, I, kh, kw] or [O, I], rows = O and cols = I*kh*kw: a rows x cols
    matrix of N(0,1) draws becomes gain * Q, Q the factor of its QR factorisation (of the transpose when rows < cols) with the signs of diag R
    folded in — torch.nn.init.orthogonal_.  BatchNorm tensors, biases, Conv1d (ECA) weights and buffers are not touched.

    The reference walks model.modules() and calls a vendor QR per weight; here the model is a flat-array model (models._FlatModel) on a CUDA
    device, anything else raises NotImplementedError (there is no CPU path), and on_begin is
        fill()            N(0,1) draws from a torch.Generator on the model's device seeded with state.random_seed — the same numbers on every rank
                          —, tensor by tensor in table order, each drawn in its logical OIHW order and copied through the parameter view
        orthogonalise()   ONE launch over all matrices (csrc/init_ortho.hip: Gram-Schmidt, every vector projected twice) and one
                          readback of its status; a matrix the kernel refuses raises RuntimeError naming the tensor
    which are callable on their own.  `records` is the planned table [(off, rows, chans, taps)], `names` the tensors' names, `status` the last
    launch's status tensor.  Deviations, both deliberate: a fit that starts at an epoch > 0 (state.start_epoch, which Runner.fit records: a resumed
    run) skips the initialisation with a log line, where the reference would overwrite the loaded weights; the reference's silent
    `except RuntimeError` for tensors of fewer than two dimensions has no counterpart, the planner never selects them.  The parameter average
    (ModelEma) was cloned before fit, as in the reference, and is left as it is."""

    def __init__(self, gain=1):
        super().__init__()
        self.gain = gain
        self.has_been_init = False
        self.records, self.names, self.status = [], [], None

    def _plan(self, m):
        self.records = item_plan.ortho_records(m._table)
        by_off = _params_by_offset(m)
        self.names = [by_off[r[0]][0] for r in self.records]
        return [by_off[r[0]][1] for r in self.records]

    @torch.no_grad()
    def fill(self):
        """the planned tensors filled with N(0,1) draws, in table order"""
        m = _flat_model_of(self.state, "OrthoInitClb")
        dev = m.flat_params.device
        g = torch.Generator(device=dev).manual_seed(int(getattr(self.state, "random_seed", 0) or 0))
        for p in self._plan(m):
            p.copy_(torch.randn(tuple(p.shape), generator=g, device=dev, dtype=torch.float32))

    @torch.no_grad()
    def orthogonalise(self):
        """one launch over the planned matrices, one readback; RuntimeError for a matrix the kernel could not orthogonalise"""
        m = _flat_model_of(self.state, "OrthoInitClb")
        self._plan(m)
        dev = m.flat_params.device
        self.status = ops.ortho_init_(m.flat_params, self.records, pack_records(self.records, dev, item_plan.ORTHO_FIELDS), self.gain)
        bad = [(n, s) for n, s in zip(self.names, self.status.tolist()) if s != 0]
        if bad:
            what = {1: "a vector with no component outside the span of the earlier ones", 2: "a record outside the flat array"}
            raise RuntimeError("OrthoInitClb: " + "; ".join(f"{n}: {what.get(s, f'status {s}')}" for n, s in bad))

    def on_begin(self):
        if self.has_been_init:
            return
        _flat_model_of(self.state, "OrthoInitClb")
        start = int(getattr(self.state, "start_epoch", 0) or 0)
        if start > 0:
            logging.getLogger(__name__).info(f"OrthoInitClb: the fit starts at epoch {start}: the loaded weights are kept, no orthogonal initialisation")
        else:
            logging.getLogger(__name__).info("Applying orthogonal initialization")
            self.fill()
            self.orthogonalise()
        self.has_been_init = True


class WeightNorm(Callback):
    """sota_imagenet/callbacks.py:104-123 (recipes 9, 10, 14, 37-39), the reference's "backward centered weight normalization": after every
    optimizer step each conv filter and each FC row — a weight [O, ...] taken as an O x (numel / O) matrix — is centred on its mean and scaled
    to unit L2 norm, in place.  It runs at the end of every training batch (the micro-batches of accumulate_steps > 1 included), on every rank
    (each applies the same deterministic kernel to identical weights), and the first forward sees the initial weights as they are.  Listed among
    run.extra_callbacks it comes after ModelEma, as in the reference: an average fused into the optimizer's step kernel takes the weights after
    the step and before the normalisation.

    The reference walks model.modules() with several torch calls per weight; here the model is a flat-array model (models._FlatModel:
    models.resnet50, bresnet.BResNet50) on a CUDA device, anything else raises NotImplementedError (there is no CPU path), the plan
    (item_plan.wnorm_records, wnorm_items) and its packed table are built once at on_begin, and on_batch_end is ONE launch of
    ops.weight_norm_rows_ over the flat parameter array on the current stream (csrc/weight_norm.hip), nothing read back.
    `records` is the planned table [(off, rows, row_len)], `names` the tensors' names, `items` the work items, `status` the last launch's status
    tensor (all zero for a plan built from the model's own table), `launches` the launches so far.  A filter whose elements are all equal
    becomes NaN (0 / 0), as in the reference.

    Three deliberate departures from the reference:
      1. Tensors with fewer than two dimensions are not selected.  The reference takes every module with a .weight of 64 elements or more; its
         view(C, -1) of a BatchNorm weight with C >= 64 is C x 1, each row's mean is the element itself and its norm 0, so it writes NaN into
         every such BatchNorm weight (it only ever ran on norm-free nets).  The planner takes parameters with ndim >= 2 and numel >= 64: Conv2d
         and Linear weights.  The ECA Conv1d weights of BResNet-50 fall under numel < 64, exactly as in the reference.
      2. It runs only while state.is_train.  The Runner fires on_batch_end during validation too, where the reference would rewrite the weights
         being evaluated — under ModelEma the swapped-in average.
      3. The constructor takes no arguments, like the reference's class as it stands.  Recipes 9, 10 and 14 still pass gamma / use_std from an
         older signature (whose helpers lived in pytorch_tools); those keys raise TypeError here, as they would there."""

    def __init__(self):
        super().__init__()
        self.records, self.names, self.items, self.status = [], [], [], None
        self.launches = 0
        self._flat = self._items_dev = None

    def on_begin(self):
        m = _flat_model_of(self.state, "WeightNorm")
        logging.getLogger(__name__).info("Using backward Centered Weight Normalization for weights")
        self.build_plan(m)

    def build_plan(self, m):
        """the records, the work items and the packed table for the flat model m"""
        self.records = item_plan.wnorm_records(m._table)
        by_off = _params_by_offset(m)
        self.names = [by_off[r[0]][0] for r in self.records]
        self.items = item_plan.wnorm_items(self.records, ops.WNORM_ITEM_ELEMS)
        ops.wnorm_check_items(self.items)  # once: the launches below pass no host table
        self._items_dev = pack_records(self.items, m.flat_params.device)
        self._flat = m.flat_params

    @torch.no_grad()
    def on_batch_end(self):
        if not self.state.is_train:
            return
        m = _flat_model_of(self.state, "WeightNorm")
        if m.flat_params is not self._flat:  # the model moved since on_begin: the table lives where the array does
            self.build_plan(m)
        self.status = ops.weight_norm_rows_(self._flat.detach(), None, self._items_dev)
        self.launches += 1


class ForwardWeightNorm(Callback):
    """sota_imagenet/callbacks.py:62-84, the forward form of the idea WeightNorm applies after the step: on_begin registers a per-filter
    parametrisation on every non-depthwise Conv2d — with use_std=False pt.utils.misc.zero_mean_conv_weight, w_hat = w - mean over each output
    filter (restated from memory of pytorch_tools) — so that forward convolves with w_hat while the optimizer keeps the
    raw w, and on_end removes it, which leaves the parametrised weight behind as the parameter.

    Here on_begin switches the plain ResNet-50 executor's weight transform to "centre" (models.ResNet50.set_weight_transform: one launch of
    csrc/weight_std.hip at the head of every forward, one per backward segment), and on_end bakes w_hat into the flat
    parameter array — ONE launch of the same forward kernel with the parameters as source and destination (ops.weight_std_rows_fwd over
    item_plan.ws_rows) — and switches the transform off: an eval forward after on_end gives the bits of one before it (a centred filter's mean
    rounds to zero only approximately, but the executor no longer subtracts it).  A model built with weight_standardization=True keeps that
    mode: the callback refuses it (RuntimeError) instead of replacing one transform by the other.
    use_std=True needs pt.utils.misc.normalize_conv_weight(gamma=...), which is not in the reference tree: NotImplementedError.  gamma without
    use_std is ignored, as in the reference.  A model that is not the plain flat ResNet-50 on a CUDA device raises NotImplementedError."""

    def __init__(self, gamma=None, use_std=False):
        super().__init__()
        if use_std:
            raise NotImplementedError("ForwardWeightNorm(use_std=True): pt.utils.misc.normalize_conv_weight is not part of the reference tree; "
                                      "use_std=False (zero_mean_conv_weight) is what is built")
        self.gamma, self.use_std = gamma, False
        self.rows, self.invstd = [], None

    def _model(self):
        from .models import ResNet50

        m = _flat_model_of(self.state, "ForwardWeightNorm")
        if not isinstance(m, ResNet50):
            raise NotImplementedError(f"ForwardWeightNorm runs on the plain ResNet-50 executor (models.resnet50 without variant keys), got {type(m).__name__}")
        return m

    def on_begin(self):
        m = self._model()
        if m.weight_transform not in (0, ops.WS_CENTRE):
            raise RuntimeError("ForwardWeightNorm: the model already standardises its weights (weight_standardization=True)")
        logging.getLogger(__name__).info("Using forward Centered Weight Normalization for weights")
        m.set_weight_transform("centre")

    @torch.no_grad()
    def on_end(self):
        m = self._model()
        if m.weight_transform != ops.WS_CENTRE:  # (on_begin never ran, or something else switched it off: nothing to leave behind)
            return
        self.rows = item_plan.ws_rows(m._table)
        rows_dev = pack_records(self.rows, m.flat_params.device)
        self.invstd = torch.empty(len(self.rows), dtype=torch.float32, device=m.flat_params.device)
        flat = m.flat_params.detach()
        ops.weight_std_rows_fwd(flat, flat, self.invstd, rows_dev, ops.WS_CENTRE)
        m.set_weight_transform("off")


class ForwardSpectralNorm(Callback):
    """sota_imagenet/callbacks.py:87-101 (recipe 29): on_begin calls torch.nn.utils.parametrizations.spectral_norm on every nn.Conv2d — forward
    convolves with w / sigma(w), sigma from one power iteration per training forward on the buffers u, v (dim 0, eps 1e-12; 15 iterations at
    registration) — and on_end removes the parametrisations, which leaves w / sigma behind as the parameter.

    Here on_begin switches the plain ResNet-50 executor's spectral normalisation on (models.ResNet50.set_spectral_norm: csrc/spectral_norm.hip
    over all 53 convolutions at the head of every forward and behind every backward segment), and on_end bakes
    w <- w / sigma into the flat parameter array with the eval rule — no power iteration, ops.spectral_fwd with the parameters as source and
    destination — and switches it off: an eval forward after on_end gives the bits of one before it.  A second on_begin leaves a warmed state
    alone.  The model must be the plain flat ResNet-50 on a CUDA device (NotImplementedError otherwise: BResNet-50, a torch model of
    nn.Conv2d, a CPU model), not fp8 (ValueError) and without a weight transform (RuntimeError); ForwardWeightNorm.on_begin on a model that
    already has spectral normalisation raises RuntimeError likewise.

    Deviations from torch, deliberate:
      * parameters(), state_dict(), the optimizer, EMA, checkpoints and the histogram callbacks see the raw weights under torchvision names;
        torch would expose parametrizations.weight.original and the buffers _u, _v.  u and v are not saved: a resumed run warms anew
        (models.ResNet50.spectral_state / load_spectral_state carry them by hand);
      * the start vectors come from a CPU generator of their own seeded with `seed` (per conv in parameter order, u then v), not from the
        global generator: every rank draws the same state without communication and the deterministic kernels keep the ranks equal bit for
        bit, where the reference relies on DDP's per-forward buffer broadcast;
      * the sums of the power iteration are taken in double and rounded once; torch takes them in float32."""

    def __init__(self, seed=0):
        super().__init__()
        self.seed = int(seed)

    def _model(self):
        from .models import ResNet50

        m = _flat_model_of(self.state, "ForwardSpectralNorm")
        if not isinstance(m, ResNet50):
            raise NotImplementedError(f"ForwardSpectralNorm runs on the plain ResNet-50 executor (models.resnet50 without variant keys), got {type(m).__name__}")
        return m

    def on_begin(self):
        m = self._model()
        logging.getLogger(__name__).info("Adding spectral norm parametrization for weights")
        m.set_spectral_norm(True, seed=self.seed)

    @torch.no_grad()
    def on_end(self):
        m = self._model()
        if not m.spectral_norm:  # (on_begin never ran, or something else switched it off: nothing to leave behind)
            return
        sn, flat = m._sn, m.flat_params.detach()
        ops.spectral_fwd(flat, flat, sn["u"], sn["v"], sn["sigma"], sn["scratch"], sn["mats_dev"], 0)
        m.set_spectral_norm(False)


class _LossTermClb(Callback):
    """what OrthoLossClb and NormLossClb share: on_begin sets state.criterion = state.criterion + term(model) * weight, ONCE per callback
    object.  The criterion must be a losses.Loss (the `+` of the reference's pt.losses.Loss); the term needs a flat model on a CUDA device
    (NotImplementedError otherwise).  The term stays in the criterion during validation, as in the reference."""

    def __init__(self, weight):
        super().__init__()
        self.weight = weight
        self.term = None

    def _make_term(self):
        raise NotImplementedError

    def on_begin(self):
        if self.term is not None:  # a later stage: train.py calls fit once per stage
            return
        from .losses import Loss

        if not isinstance(self.state.criterion, Loss):
            raise TypeError(f"{type(self).__name__}: state.criterion must be a losses.Loss to take another term, got {type(self.state.criterion).__name__}")
        term = self._make_term()
        self.state.criterion = self.state.criterion + term * self.weight
        self.term = term


class OrthoLossClb(_LossTermClb):
    """sota_imagenet/callbacks.py:191-203 (recipes 24, 29, 30, 35, 39): on_begin appends OrthoLoss(model, **kwargs) * weight to the criterion —
    losses.OrthoLoss on csrc/ortho_loss.hip; kwargs are its eps, min_filters, min_norm, debug.  type=2, the
    convolutional form OrthoLoss2 (callbacks.py:159-188), raises NotImplementedError: no ResNet-50 recipe here uses it.

    Deviations from the reference, deliberate:
      * the term is appended once.  The reference's on_begin runs at every fit, and its train.py calls fit once per stage, so there a run of
        k stages ends with k copies of the penalty, the effective weight growing stage by stage;
      * the Gram products are always fp32 (the reference's run in half precision under autocast) and the gate F / O > min_norm is decided on the
        device (losses.OrthoLoss)."""

    def __init__(self, weight=0.01, type=1, **kwargs):
        super().__init__(weight)
        if type != 1:
            raise NotImplementedError(f"OrthoLossClb(type={type!r}): only type 1 (kernel orthogonalisation, OrthoLoss) is built; type 2 is the "
                                      "convolutional form OrthoLoss2")
        self.type, self.kwargs = type, kwargs

    def _make_term(self):
        from .losses import OrthoLoss

        return OrthoLoss(_flat_model_of(self.state, "OrthoLossClb"), **self.kwargs)


class NormLossClb(_LossTermClb):
    """sota_imagenet/callbacks.py:224-229: on_begin appends NormLoss(model) * weight to the criterion — losses.NormLoss on csrc/ortho_loss.hip.
    Appended once, not once per stage (see OrthoLossClb)."""

    def __init__(self, weight=1e-4):
        super().__init__(weight)

    def _make_term(self):
        from .losses import NormLoss

        return NormLoss(_flat_model_of(self.state, "NormLossClb"))


class GradDistributionTB(Callback):
    """sota_imagenet/callbacks.py:30-60 (recipes 46, 49-55): every log_every-th training step, a histogram of log10 |x| of a twice-subsampled
    selection of the optimizer's states (`optim/{key}_log` for every key of state_keys, taken as the reference takes them: optimizer.state.values(),
    v[key]) and of the model's parameters (`optim/model_params_log`), on rank 0 only.  The reference sorts every tensor, keeps every subsample-th
    value, sorts the concatenation and keeps every subsample-th value again; here no sort is made: the kept ranks 0, s, 2s, ... of a sorted tensor
    include exactly ceil(c / s) values below a threshold, c the tensor's elements below it, so the bin counts of the reference's selection follow
    exactly from per-tensor bin counts (csrc/optim_hist.hip).  The bins are ops.ABSBIN_*: eight per octave from 1.22e-15 to
    1.8e4, bin 0 everything the reference clamps to -15, the last bin everything above including infinities and NaN.

    The plan — what to read of every tensor (item_plan.hist_records: dense views as they are, a state stored once and shown broadcast counted
    once with its multiplicity), the tensors grouped by storage, the work items on the device — is built at the first logged step and rebuilt when
    the set of tensors or their addresses change.  A logged step is one zero_ of the histograms, one ops.absbin_hist per storage and tag, one
    ops.subsample_counts per tag and ONE copy of the [tags, 512] counts to the host, the callback's only host synchronisation.  `last` =
    {tag: (bucket_limits float64 [512]: log10 of the bins' upper edges, counts int64 [512])} holds the last logged step; with a state.tb_logger it
    goes out through add_histogram_raw at state.global_sample_step: num is exact, min and max are the outer limits of the first and last non-empty
    bins, sum and sum_squares are formed from the bins' midpoints (TensorBoard uses them for display only).

    A missing key raises KeyError naming the optimizer class and the key, a state that is no tensor TypeError (MyAdai keeps exp_avg_sq as a Python
    float; the reference would fail on .flatten() there, which is why recipe 55 lists exp_avg only), an optimizer without any state yet
    RuntimeError (the reference's torch.cat of nothing), parameters or states that are not CUDA fp32 NotImplementedError: there is no CPU path.
    One deviation, deliberate: validation batches do not log.  The reference's on_batch_end has no is_train test and would write the same unchanged
    arrays again at the same global_sample_step."""

    def __init__(self, log_every=500, subsample=10, state_keys=['exp_avg', 'exp_avg_sq']):
        super().__init__()
        if int(log_every) < 1 or int(subsample) < 1:
            raise ValueError(f"GradDistributionTB: log_every={log_every} and subsample={subsample} must be >= 1")
        self.log_every = int(log_every)
        self.subsample = int(subsample)
        self.state_keys = list(state_keys)
        self.last = {}
        self.logged = 0     # logged steps so far
        self._key = None
        self._tags = []     # per tag: (name, [(flat source array, items on the device)] per storage, rep on the device, its rows of the histograms)
        self._limits = ops.absbin_log10_limits()

    def _tensors(self):
        """[(tag, [tensor])] as the reference gathers them"""
        opt = self.state.optimizer
        states = list(opt.state.values())
        if self.state_keys and not states:
            raise RuntimeError(f"GradDistributionTB: {type(opt).__name__} has no state yet (no step was made): nothing to gather")
        out = []
        for key in self.state_keys:
            ts = []
            for v in states:
                if key not in v:
                    raise KeyError(f"GradDistributionTB: {type(opt).__name__} keeps no state '{key}' (it has {sorted(map(str, v))})")
                if not torch.is_tensor(v[key]):
                    raise TypeError(f"GradDistributionTB: state '{key}' of {type(opt).__name__} is a {type(v[key]).__name__}, not a tensor")
                ts.append(v[key])
            out.append((f"optim/{key}_log", ts))
        out.append(("optim/model_params_log", [p.data for p in _unwrap(self.state.model).parameters()]))
        return out

    def build_plan(self, tagged):
        """tagged: [(tag, [tensor])]; the tables on the device, one launch per storage and tag"""
        recs = [(tag, ts, [item_plan.hist_records(t) for t in ts]) for tag, ts in tagged]
        W = ops.lw_item_elems()
        dev = _one_device("GradDistributionTB", "all parameters and states", [t for _, ts, _ in recs for t in ts])
        rows = sum(len(ts) for _, ts, _ in recs)
        self._hist = torch.zeros(rows, ops.ABSBIN_BINS, dtype=torch.int32, device=dev)
        self._counts = torch.zeros(len(recs), ops.ABSBIN_BINS, dtype=torch.int64, device=dev)
        self._tags, row0 = [], 0
        for tag, ts, rs in recs:
            launches = []  # a row of the plan is the tensor's position in its tag
            for base, lo, hi, items, _ in item_plan.dist_plan([r[:3] for r in rs], W)[1]:
                if base % 16:
                    raise RuntimeError(f"GradDistributionTB: a storage of {tag} does not start on a 16-byte boundary")
                launches.append((item_plan.storage_array(ts[items[0][2]], lo, hi), pack_records(items, dev)))
            rep = [r[3] for r in rs]
            if max(rep) >= 1 << 31:
                raise RuntimeError(f"GradDistributionTB: a tensor of {tag} has 2^31 elements or more")
            self._tags.append((tag, launches, torch.tensor(rep, dtype=torch.int32, device=dev), (row0, row0 + len(ts))))
            row0 += len(ts)

    @torch.no_grad()
    def log(self):
        """one logged step: `last`, and the histograms to state.tb_logger if there is one"""
        tagged = self._tensors()
        key = tuple((tag, tuple(map(_tensor_key, ts))) for tag, ts in tagged)
        if key != self._key:
            self.build_plan(tagged)
            self._key = key
        self._hist.zero_()
        for k, (tag, launches, rep, (r0, r1)) in enumerate(self._tags):
            for src, items in launches:
                ops.absbin_hist(src, items, self._hist[r0:r1])
            ops.subsample_counts(self._hist[r0:r1], rep, self.subsample, self._counts[k])
        counts = self._counts.cpu().numpy()  # the one host synchronisation of a logged step
        if (counts < 0).any():
            raise RuntimeError("GradDistributionTB: the counting kernel refused its table (a multiplicity below 1)")
        self.last = {tag: (self._limits, counts[k].copy()) for k, (tag, *_) in enumerate(self._tags)}
        self.logged += 1
        _log_histograms(self.state, self.last, lambda v: (*self.raw_stats(*v), v[0].tolist(), v[1].tolist()))

    @staticmethod
    def raw_stats(limits, counts):
        """(min, max, num, sum, sum_squares) of add_histogram_raw: num exact; min / max the outer limits of the first / last non-empty bin (-15 below
        bin 0); sum and sum_squares from the bins' midpoints in log10, for display only"""
        lower = np.concatenate(([-15.0], limits[:-1]))
        num = int(counts.sum())
        nz = np.nonzero(counts)[0]
        if not len(nz):
            return 0.0, 0.0, 0, 0.0, 0.0
        mid = 0.5 * (lower + limits)
        return float(lower[nz[0]]), float(limits[nz[-1]]), num, float((mid * counts).sum()), float((mid * mid * counts).sum())

    def on_batch_end(self):
        if self.state.rank != 0 or env_rank() != 0 or not self.state.is_train or self.state.step % self.log_every != 0:
            return
        self.log()


def tb_trim(counts, edges):
    """the trimming of add_histogram (torch/utils/tensorboard/summary.py, make_histogram): counts [bins] over edges [bins + 1] -> (bucket_limits,
    bucket_counts) from the first to the last non-empty bin, with one empty bin in front so that the leftmost limit is kept — the bin to the left
    of the first non-empty one, or a zero where that is bin 0.  No counted value raises ValueError, as upstream does."""
    nz = np.flatnonzero(counts)
    if not len(nz):
        raise ValueError("The histogram is empty: no value lies inside the bins")
    start, end = int(nz[0]), int(nz[-1])
    kept = counts[start - 1: end + 1] if start > 0 else np.concatenate(([0], counts[: end + 1]))
    return edges[start: end + 2].tolist(), [int(c) for c in kept]


def tb_host_counts(values, edges):
    """np.histogram(values, bins=edges) of float64 values, stated by position: bin i is [edges[i], edges[i+1]), the last bin also takes
    values == edges[-1]; NaN, infinities and everything outside the edges are counted nowhere"""
    idx = np.searchsorted(edges, values, side="right") - 1  # the last edge <= x; NaN sorts behind every edge
    idx[values == edges[-1]] = len(edges) - 2
    ok = (idx >= 0) & (idx <= len(edges) - 2) & ~np.isnan(values)
    return np.bincount(idx[ok], minlength=len(edges) - 1)


class _WeightDistPlan:
    """what WeightDistributionTB keeps between epochs: rows / spans (item_plan.dist_plan), launches = [(flat source array, items on the device,
    (first item, end item))], gathers = [(source tensor, first, end)] into `other`, where = {entry: (first, numel)} in `other`, and the one device
    buffer `buf` with its three views hist [rows, TBBIN_ROW] int32, partial [items, TBBIN_STATS] float64 and other float64"""


class WeightDistributionTB(Callback):
    """sota_imagenet/callbacks.py:11-17, added by train.py:140 when `log.histogram` is set (recipes 4, 11-14, 45-55): at every epoch's begin, on rank 0
    only, every entry of state.model.state_dict(), in its order and under the tag "model/" + its name, as the histogram that
    SummaryWriter.add_histogram(tag, p.flatten(), global_sample_step) draws with its defaults.  The reference copies the entries to the host one
    by one and runs np.histogram over the 1549 default edges on each; here the CUDA fp32 entries (whatever item_plan.hist_records takes as a dense
    view) are counted where they lie, by one ops.tbbin_hist per storage — two launches for models.resnet50: the flat parameters and the flat
    buffers — which also gives min, max, sum and sum of squares per work item (csrc/optim_wdist.hip).  Every other entry —
    the int64 num_batches_tracked, which are views of one array — is gathered on the device, one cast to float64 per storage, and binned on the
    host by the same rule (tb_host_counts).  Counts, statistics and gathered values share one device buffer: a logged epoch is one zero_ of the
    table, the launches, and ONE copy to the host, the callback's only host synchronisation.  The plan is built at the first logged epoch and
    rebuilt when the names, addresses, shapes, strides or dtypes change.

    `last` = {tag: dict(min, max, num, sum, sum_squares, bucket_limits, bucket_counts)} holds the last logged epoch: limits and counts trimmed as
    add_histogram trims them (tb_trim), min / max / sum / sum_squares in float64 over all values, counted or not (min and max NaN where the
    tensor holds a NaN), num = numel.  With a state.tb_logger every tag goes out through add_histogram_raw at state.global_sample_step.  The sums
    are added in a fixed order (inside a workgroup, then a tensor's work items in table order on the host): two runs agree bit for bit; against
    numpy's order they differ by rounding.  An entry without a counted value — empty, or all NaN / out of range — raises ValueError as
    add_histogram does; CPU tensors raise NotImplementedError: there is no CPU path."""

    def __init__(self):
        super().__init__()
        self.last = {}
        self.logged = 0  # logged epochs so far
        self._key = None
        self._plan = None
        self._edges = ops.tbbin_edges()

    def build_plan(self, named):
        """named: [(name, tensor)] of the state_dict"""
        for name, t in named:
            if not (torch.is_tensor(t) and t.is_cuda):
                raise NotImplementedError(f"WeightDistributionTB: {name} is not a CUDA tensor (there is no CPU path)")
            if t.numel() < 1:
                raise ValueError(f"WeightDistributionTB: {name} has no element")
        dev = _one_device("WeightDistributionTB", "the state_dict", [t for _, t in named])
        records = []
        for _, t in named:
            rec = None
            if t.dtype == torch.float32:
                try:
                    base, first, n, rep = item_plan.hist_records(t)
                    if rep == 1 and base % 16 == 0 and n < 1 << 31:
                        rec = (base, first, n)
                except RuntimeError:  # neither dense nor one of the broadcast forms: the host rule takes it
                    pass
            records.append(rec)
        P = _WeightDistPlan()
        P.rows, launches, P.spans, n_items = item_plan.dist_plan(records, ops.lw_item_elems())
        # every other entry: grouped by storage and dtype where it is a dense view, else on its own
        groups, loose = {}, []
        for k, (_, t) in enumerate(named):
            if records[k] is not None:
                continue
            r = item_plan.dense_range(t)
            if r is None:
                loose.append(k)
                continue
            g = groups.setdefault((r[0], t.dtype), [r[1], r[1] + r[2], []])
            g[0], g[1] = min(g[0], r[1]), max(g[1], r[1] + r[2])
            g[2].append((k, r[1], r[2]))
        P.gathers, P.where, n_other = [], {}, 0
        for lo, hi, members in groups.values():
            P.gathers.append((item_plan.storage_array(named[members[0][0]][1], lo, hi), n_other, n_other + hi - lo))
            for k, first, n in members:
                P.where[k] = (n_other + first - lo, n)
            n_other += hi - lo
        for k in loose:
            t = named[k][1]
            P.gathers.append((t, n_other, n_other + t.numel()))
            P.where[k] = (n_other, t.numel())
            n_other += t.numel()
        h, p = len(P.rows) * ops.TBBIN_ROW // 2, n_items * ops.TBBIN_STATS  # in 8-byte words
        P.buf = torch.zeros(h + p + n_other, dtype=torch.int64, device=dev)
        P.cuts = (h, h + p)
        P.hist = P.buf[:h].view(torch.int32).view(len(P.rows), ops.TBBIN_ROW)
        P.partial = P.buf[h: h + p].view(torch.float64).view(n_items, ops.TBBIN_STATS)
        P.other = P.buf[h + p:].view(torch.float64)
        P.launches = []
        for base, lo, hi, items, i0 in launches:
            src = item_plan.storage_array(named[P.rows[items[0][2]]][1], lo, hi)
            P.launches.append((src, pack_records(items, dev), (i0, i0 + len(items))))
        return P

    @torch.no_grad()
    def log(self):
        """one logged epoch: `last`, and the histograms to state.tb_logger if there is one"""
        named = list(self.state.model.state_dict().items())
        key = tuple((name, _tensor_key(t) if torch.is_tensor(t) else None) for name, t in named)
        if key != self._key:
            self._plan = self.build_plan(named)
            self._key = key
        P = self._plan
        P.hist.zero_()
        for src, items, (i0, i1) in P.launches:
            ops.tbbin_hist(src, items, P.hist, P.partial[i0:i1])
        for t, a, b in P.gathers:
            P.other[a:b].copy_(t.reshape(-1))
        host = P.buf.cpu().numpy()  # the one host synchronisation of a logged epoch
        h, p = P.cuts
        hist = host[:h].view(np.uint32).reshape(len(P.rows), ops.TBBIN_ROW)
        partial = host[h:p].view(np.float64).reshape(-1, ops.TBBIN_STATS)
        other = host[p:].view(np.float64)
        row_of = {k: r for r, k in enumerate(P.rows)}
        edges, last = self._edges, {}
        for k, (name, t) in enumerate(named):
            if k in row_of:
                r = row_of[k]
                i0, c = P.spans[r]
                st = partial[i0: i0 + c]
                counts = hist[r, : ops.TBBIN_BINS].astype(np.int64)
                if int(counts.sum()) + int(hist[r, ops.TBBIN_NOBIN]) != t.numel():
                    raise RuntimeError(f"WeightDistributionTB: {name}: the counting kernel skipped a work item of its table")
                nan = bool(st[:, 4].any())
                # cumsum adds strictly in table order
                stats = dict(min=float("nan") if nan else float(st[:, 0].min()), max=float("nan") if nan else float(st[:, 1].max()),
                             num=t.numel(), sum=float(np.cumsum(st[:, 2])[-1]), sum_squares=float(np.cumsum(st[:, 3])[-1]))
            else:
                a, n = P.where[k]
                v = other[a: a + n]
                counts = tb_host_counts(v, edges)
                stats = dict(min=float(v.min()), max=float(v.max()), num=n, sum=float(v.sum()), sum_squares=float(v.dot(v)))
            try:
                limits, kept = tb_trim(counts, edges)
            except ValueError as e:
                raise ValueError(f"WeightDistributionTB: {name}: {e}") from None
            last["model/" + name] = dict(stats, bucket_limits=limits, bucket_counts=kept)
        self.last = last
        self.logged += 1
        _log_histograms(self.state, last, lambda d: [d[k] for k in ("min", "max", "num", "sum", "sum_squares", "bucket_limits", "bucket_counts")])

    def on_epoch_begin(self):
        if self.state.rank != 0 or env_rank() != 0:
            return
        self.log()


# one pair of parameter / gradient storage in a plan: the two storages as flat arrays over the pair's element range [lo, hi), the pair's eps array
# over the same range and (first item, end item); SAM adds the pair's part of the reduction tables: (first piece, end piece), (first whole-tensor
# item, end) and its first entry of the partial sums (its pieces, then its whole-tensor items)
_Seg = namedtuple("_Seg", "p g eps items")
_SamSeg = namedtuple("_SamSeg", _Seg._fields + ("pieces", "whole", "partial0"))


class _SecondPass(Callback):
    """what SAMOriginal and SAM share: the plan built from a parameter list under item_plan's placement rule (build_plan), one launch set per
    pair of parameter / gradient storage with an eps array of its own, the re-plan test, the second forward / backward on the same batch, and the
    way back (mi355_sam_restore)"""

    def __init__(self):
        super().__init__()
        self._key = None
        self._segs = []     # per storage pair: a _Seg / _SamSeg
        self._eps = []      # per storage pair: the eps array, indexed like the storage
        self.forwards = 0   # second forwards made so far

    @property
    def eps_flat(self):
        if not self._eps:
            return None
        return self._eps[0] if len(self._eps) == 1 else list(self._eps)

    def on_begin(self):
        if getattr(self.state, "accumulate_steps", 1) != 1:
            raise NotImplementedError(f"{type(self).__name__}: accumulate_steps != 1 is not supported (the second pass would discard the "
                                      "accumulated micro-gradients)")

    def _plan_changed(self, params):
        """True at the first perturbed step and whenever the parameters or their addresses changed since the plan was built"""
        key = tuple((id(p), p.data_ptr(), p.grad.data_ptr(), p.numel()) for p in params)
        changed, self._key = key != self._key, key
        return changed

    _table = staticmethod(pack_records)  # (records, device): the packer under the name earlier callers of the callbacks know

    def build_plan(self, params):
        """the plan for `params` (parameters that all have a gradient, in param-group order): the tables on the device and one segment per
        storage pair.  Anything item_plan.place refuses raises RuntimeError."""
        entries = place(params, type(self).__name__, aligned=True, one_device=True)
        self._eps = []
        self._segs = self._build(entries, entries[0][4].device, ops.lw_item_elems())

    def _pair_views(self, p, lo, hi):
        """the storages of p and of its gradient as flat arrays over [lo, hi) and a new eps array for the pair, indexed like the storage (eps_flat
        lines up with a model's flat array): (parameters, gradients, eps slice)"""
        eps = torch.zeros(hi, dtype=torch.float32, device=p.device)
        self._eps.append(eps)
        return (*flat_views(p, lo, hi), eps[lo:hi])

    def _second_pass(self, n_tensors):
        """zero_grad, a second forward / backward at the perturbed parameters on the same (already mixed) batch, then p -= eps"""
        self.state.optimizer.zero_grad()  # (with an attached flat model: marks its gradients clean, the second backward overwrites them)
        with torch.enable_grad():
            data, target = self.state.input
            loss_second = self.state.criterion(self.state.model(data), target)
            loss_second.backward()
        self.forwards += 1
        for seg in self._segs:
            i0, i1 = seg.items
            ops.sam_restore(seg.p, seg.eps, self._items[i0:i1], n_tensors)


class SAMOriginal(_SecondPass):
    """sota_imagenet/callbacks.py:279-337 (recipe configs/hydra_exp/49.r50_nov-adam.yaml:46-48): adaptive sharpness-aware minimization as
    the reference runs it.  After the first backward of a step, with g the gradient the optimizer would see (g * optimizer.grad_scale):
        norm  = max(sqrt(sum over all tensors of |w|^2), 2e-5),   w = g * max(|p|, eta) for tensors with ndim > 1, w = g for the others
        eps   = max(p^2, eta) * g * (rho / norm) for ndim > 1,    eps = g * (rho / norm) for the others;   p += eps
        optimizer.zero_grad(); a second criterion(model(data), target).backward() on the same (already mixed) batch;   p -= eps
    and the optimizer then steps from the unperturbed parameters on the SECOND gradient.  (p + eps) - eps is in general not p bit for bit:
    the reference's behaviour, kept.  The very first step, while the optimizer has no state yet (len(optimizer.state) == 0), is a plain step.

    The four stages are HIP kernels over the flat arrays (csrc/optim_sam.hip) on the current stream; nothing is read back in a step.  The
    plan is built at the first non-skipped step from optimizer.param_groups under the rules of the native optimizers (CUDA fp32, dense,
    parameter and gradient at the same 16-byte aligned flat offset; one launch set per pair of parameter / gradient storage; the work items
    of item_plan.py, where the plan's host side lives) and rebuilt when the parameters or their addresses change.  There is no CPU fallback:
    parameters that do not fit raise.  `norm` and `scale` are 1-element device tensors holding the last step's values, `eps_flat` the last perturbation: one
    float32 array per storage pair indexed like the storage itself (the array itself when there is one pair, zero outside the parameters).

    As in the reference the second forward runs through state.model in training mode: a data-parallel wrapper reduces the second gradient
    too, and BatchNorm running statistics and num_batches_tracked advance TWICE per SAM step.
    Deviations, both deliberate: accumulate_steps != 1 raises at on_begin (the reference's zero_grad would silently discard the accumulated
    micro-gradients); eps lives in this callback, not in optimizer.state[p]["eps_step"], so no optimizer's state_dict() changes."""

    def __init__(self, rho=0.5, eta=0.01):
        super().__init__()
        if not (rho > 0 and np.isfinite(rho)):
            raise ValueError(f"Invalid rho: {rho}")
        if not (eta >= 0 and np.isfinite(eta)):
            raise ValueError(f"Invalid eta: {eta}")
        self.rho = rho
        self.eta = eta
        self._out = None    # (rho / norm, norm) of the last step

    @property
    def scale(self):
        return None if self._out is None else self._out[0:1]

    @property
    def norm(self):
        return None if self._out is None else self._out[1:2]

    @staticmethod
    def plan_tables(tensors, W):
        """the host side of a plan.  tensors: [(param base, grad base, first elem, numel, ndim)] in param-group order; W: ops.lw_item_elems().
        Returns (items, kind, pairs): items and pairs = [(lo, hi, first item, end item, tensor indices)] from item_plan.storage_pairs — items =
        [(first element relative to its pair's range, length, tensor index)], storage pair by storage pair, [lo, hi) the element range of the
        storage a pair's tensors span; kind[tensor] = 1 for ndim > 1"""
        items, _, pairs = storage_pairs(tensors, W)
        return items, [int(t[4] > 1) for t in tensors], pairs

    def _build(self, entries, dev, W):
        items, kind, pairs = self.plan_tables([(pb, gb, off, n, p.ndim) for pb, gb, off, n, p in entries], W)
        self._items = pack_records(items, dev)
        self._kind = torch.tensor(kind, dtype=torch.int32, device=dev)
        self._partial = torch.zeros(len(items), dtype=torch.float64, device=dev)
        self._out = torch.zeros(2, dtype=torch.float32, device=dev)
        return [_Seg(*self._pair_views(entries[ts[0]][4], lo, hi), (i0, i1)) for lo, hi, i0, i1, ts in pairs]

    @torch.no_grad()
    def on_after_backward(self):
        opt = self.state.optimizer
        if len(opt.state) == 0:  # the first step: the optimizer creates its state from a plain step
            return
        params = [p for group in opt.param_groups for p in group["params"] if p.grad is not None]
        if not params:
            return
        if self._plan_changed(params):  # the first non-skipped step, or the parameters / their addresses changed
            self.build_plan(params)
        gs = float(getattr(opt, "grad_scale", 1.0))
        for seg in self._segs:
            i0, i1 = seg.items
            ops.sam_sumsq(seg.p, seg.g, self._items[i0:i1], self._kind, self._partial[i0:i1], self.eta, grad_scale=gs)
        ops.sam_scale(self._partial, self.rho, self._out)
        for seg in self._segs:
            i0, i1 = seg.items
            ops.sam_perturb(seg.p, seg.g, seg.eps, self._items[i0:i1], self._kind, self._out, self.eta, grad_scale=gs)
        self._second_pass(self._kind.numel())


class SAM(_SecondPass):
    """sota_imagenet/callbacks.py:339-420 with unitwise_norm :269-276 (the form the recipes write down, configs/hydra_exp/
    32.nf_conv-act_sam.yaml:104-106): sharpness-aware minimization with the perturbation scaled slot by slot.  A slot is a whole tensor when
    unitwise is False or the tensor has at most one dimension; otherwise every index of dim 0 (a filter of a conv, a row of the FC) is a slot of
    its own.  After the first backward of EVERY step (there is no first-step skip), with g the gradient the optimizer would see
    (g * optimizer.grad_scale), per slot:
        gn = max(||g||_2, eps),  wn = max(||p||_2, eps_2),  e = ((wn / gn) * g) * rho;   p += e
        optimizer.zero_grad(); a second criterion(model(data), target).backward() on the same (already mixed) batch;   p -= e
    and the optimizer steps from the unperturbed parameters on the SECOND gradient.  (p + e) - e is in general not p bit for bit: the
    reference's behaviour, kept.  rho = 0 is legal (the recipe file writes rho: 0): the second pass still runs.

    The stages are HIP kernels over the flat arrays (csrc/optim_sam_lw.hip) on the current stream; nothing is read back in a step.  Per pair
    of parameter / gradient storage: 4 launches layer-wise (whole-tensor sums, coefficients, perturbation, restore), 5 unit-wise (unit sums,
    whole-tensor sums of the 1-D tensors, coefficients, perturbation, restore); the coefficient launch is one per step for all pairs.  The
    plan is built at the first step under the placement rules of SAMOriginal and rebuilt when the parameters or their addresses change.  A
    unit must be one contiguous run of numel / shape[0] elements, i.e. dim 0 the outermost stride (the flat models' OIHW views over KRSC
    memory are): anything else raises RuntimeError.  There is no CPU fallback.  `coef` ([slots] float32: wn / gn) and `norms` ([slots, 2]:
    gn, wn) hold the last step's values on the device, slots numbered tensor by tensor in param-group order (slot_ranges: per tensor (first
    slot, slots)); `eps_flat` is the last perturbation as in SAMOriginal; `forwards` counts the second forwards.

    As in the reference BatchNorm running statistics and num_batches_tracked advance TWICE per step, and a data-parallel wrapper reduces the
    second gradient too.  Deviations, the two of SAMOriginal: accumulate_steps != 1 raises at on_begin; eps lives in this callback, not in
    optimizer state."""

    def __init__(self, unitwise=False, rho=0.01):
        super().__init__()
        if not (rho >= 0 and np.isfinite(rho)):
            raise ValueError(f"Invalid rho: {rho}")
        self.unitwise = bool(unitwise)
        self.rho = rho
        self.eps = 1e-5    # floor of the gradient norm (callbacks.py:367); the kernels hold it as a float32 constant
        self.eps_2 = 1e-3  # floor of the weight norm (:368)
        self._coef = self._norms = None
        self.slot_ranges = []

    @property
    def coef(self):
        return self._coef

    @property
    def norms(self):
        return self._norms

    @staticmethod
    def unit_len(shape, stride, unitwise):
        """elements per slot of a dense tensor: numel, or numel / shape[0] for a unit-wise tensor with ndim > 1 — whose dim 0 must be the
        outermost stride, so that a unit is one contiguous run"""
        return item_plan.unit_len(shape, stride, unitwise, "SAM")

    @staticmethod
    def plan_tables(tensors, W):
        """the host side of a plan.  tensors: [(param base, grad base, first elem, numel, unit_len)] in param-group order, unit_len = numel for
        a whole-tensor slot, less for a tensor taken unit by unit; W: ops.lw_item_elems().  Returns a dict:
          items    item_plan.storage_pairs' work items of ALL tensors (the perturbation and the restore walk them)
          tensors  [(start relative to its pair's range, unit_len, slot0)] per tensor; slots are numbered tensor by tensor
          pieces   [(first element relative to the pair's range, length <= W, slot)]: every unit of the unit-wise tensors, cut at multiples of
                   W from the unit's start
          whole    the work items of the whole-tensor slots, in the order of `items`
          slots    [(first, count)] per slot: its consecutive entries of the partial sums, which are laid out pair by pair, a pair's pieces
                   before its whole-tensor items
          pairs    [(lo, hi, first item, end item, (first piece, end piece), (first whole item, end), first partial entry, tensor indices)]
        (item_plan.plan_units, which the unit-wise optimizers build on as well)"""
        return item_plan.plan_units(tensors, W)

    def _build(self, entries, dev, W):
        tab = self.plan_tables([(pb, gb, off, n, self.unit_len(p.shape, p.stride(), self.unitwise)) for pb, gb, off, n, p in entries], W)
        self._items, self._tensors = pack_records(tab["items"], dev), pack_records(tab["tensors"], dev)
        self._pieces, self._whole = pack_records(tab["pieces"], dev), pack_records(tab["whole"], dev)
        n_slots = len(tab["slots"])
        self._slots = torch.tensor(tab["slots"], dtype=torch.int32, device=dev)
        self._partial = torch.zeros(2 * (len(tab["pieces"]) + len(tab["whole"])), dtype=torch.float64, device=dev)
        self._coef = torch.zeros(n_slots, dtype=torch.float32, device=dev)
        self._norms = torch.zeros(n_slots, 2, dtype=torch.float32, device=dev)
        self.slot_ranges = [(s0, e[3] // u) for (_, u, s0), e in zip(tab["tensors"], entries)]
        return [_SamSeg(*self._pair_views(entries[ts[0]][4], lo, hi), (i0, i1), pc, wh, k0) for lo, hi, i0, i1, pc, wh, k0, ts in tab["pairs"]]

    @torch.no_grad()
    def on_after_backward(self):
        opt = self.state.optimizer
        params = [p for group in opt.param_groups for p in group["params"] if p.grad is not None]
        if not params:
            return
        if self._plan_changed(params):  # the first step, or the parameters / their addresses changed
            self.build_plan(params)
        gs = float(getattr(opt, "grad_scale", 1.0))
        nt, ns = self._tensors.shape[0], self._coef.numel()
        for seg in self._segs:
            (pa, pb), (wa, wb), k0 = seg.pieces, seg.whole, seg.partial0
            k1 = k0 + pb - pa
            if pb > pa:
                ops.sam_unit_sumsq(seg.p, seg.g, self._pieces[pa:pb], self._partial[2 * k0:2 * k1], ns, grad_scale=gs)
            if wb > wa:
                ops.sam_lw_sumsq(seg.p, seg.g, self._whole[wa:wb], self._partial[2 * k1:2 * (k1 + wb - wa)], nt, grad_scale=gs)
        ops.sam_lw_coef(self._partial, self._slots, self._coef, self._norms)
        for seg in self._segs:
            i0, i1 = seg.items
            ops.sam_lw_perturb(seg.p, seg.g, seg.eps, self._items[i0:i1], self._tensors, self._coef, self.rho, grad_scale=gs)
        self._second_pass(nt)
