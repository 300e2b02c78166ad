"""`SGD`, `Adam`, `AdamW`, `MADGRAD`, `AdaiS`, `NovogradApex`, `MyNovograd`, `AdamLayerwise`, `MyAdai` and `AdamP` plugins: torch.optim-compatible optimizers whose step is fused HIP kernels over flat ranges.

Drop-in for `_target_: torch.optim._multi_tensor.SGD` (sota_imagenet/arg_parser.py:136-138; r50 recipe adds
momentum 0.9 / weight_decay 3e-5, configs/hydra_exp/1.r50_baseline.yaml:29-31; built at train.py:92 from
`opt_params = [{"params": [...]}(, {"params": [...], "weight_decay": 0})]`, train.py:83-89; the scheduler writes
`param_group["lr"]` every batch).  Semantics = torch.optim.SGD with dampening 0, nesterov off:
    g += wd * p ;  m = mu * m + g  (first step m = g) ;  p -= lr * m
Parameters that are views of a model's flat fp32 array (models.ResNet50) are updated range-wise in place;
adjacent ranges of one param group collapse into a single launch (the default recipe = 1 launch / step).
Adam / AdamW (csrc/optim.hip) share that range planner and the rest of the contract (attach_model, attach_ema, grad_scale,
zero_grad, re-planning after load_state_dict); their per-parameter state is laid out as torch lays it out.
MADGRAD and AdaiS are the reference's own optimizers (sota_imagenet/optimizers.py) on the same planner: MADGRAD is one launch per range,
AdaiS three stages (moments + partial sums, the global mean, the update) because its momentum depends on a statistic of all parameters.
NovogradApex, MyNovograd, AdamLayerwise and MyAdai (the reference's layer-wise optimizers) use one statistic PER TENSOR: they do not merge ranges
but cut every parameter's own range into work items and run three stages over that table (csrc/optim_lw.hip).  With unitwise_norm=True
NovogradApex and MyNovograd take the statistic per output unit instead (one slot per filter of a conv or row of the FC; the pieces and slots of
item_plan.plan_units).  That plan — the placement rule,
the storage pairs, the work items, the packed records — lives in item_plan.py, which the SAM callbacks build on as well.
AdamP (`adamp.AdamP`, recipes 51 and 52; restated from the published package, which is not available here: see the class) runs on the same
unit-wise tables: per-piece sums of four products, one decision per tensor on the device, and an update that takes each element's projection
coefficients from its slot (csrc/optim_adamp.hip).
"""
from collections import namedtuple
from itertools import groupby

import torch
from torch.optim import Optimizer

from . import ops
from .item_plan import TENSOR_FIELDS, dense_range, flat_views, pack_records, place, plan_units, storage_pairs, unit_len
from .item_plan import plan_items as lw_plan_items  # noqa: F401  (the name its callers know)


class _FlatOptimizer(Optimizer):
    """what the native optimizers share: the flat-range planner (merged launch ranges, barriers, 16-byte alignment), the
    fused parameter average (attach_ema), grad_scale, zero_grad that only marks the model's flat gradients clean, and
    re-planning after add_param_group / load_state_dict.  Subclasses build their plans from _merged_ranges() in
    _build_plans() and launch them in step()."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plans = None
        self._models = []
        self.grad_scale = 1.0  # e.g. 1/world_size when gradients were summed, not averaged
        self._ema = None       # (flat parameter array, its moving average, decay): attach_ema()

    def attach_model(self, model):
        """lets zero_grad() tell the model that the next backward may overwrite its flat gradients, and the range
        planner see every tensor of the model (which gaps between updated parameters are padding)."""
        self._models.append(model)
        self._plans = None

    def attach_ema(self, flat_params, flat_ema, decay):
        """the moving average of a model's flat parameter array (fit_wrapper.ModelEma, train.py:111-112) is advanced by the step kernel
        itself: ema += (1 - decay) * (p_new - ema) over every range this optimizer updates (ranges it does not update never change, so
        their average stays what it was cloned from).  detach_ema() hands the job back to the callback."""
        if not (flat_ema.is_cuda and flat_ema.dtype == torch.float32 and flat_ema.is_contiguous() and flat_ema.numel() == flat_params.numel()):
            raise ValueError("attach_ema: the average must be a contiguous CUDA fp32 tensor of the flat array's size")
        self._ema = (flat_params, flat_ema, float(decay))
        self._plans = None

    def detach_ema(self):
        self._ema = None
        self._plans = None

    def _entries(self, **rules):
        """[(param base, grad base, first elem, numel, group index, param)] of every parameter with a gradient, group by group, under
        item_plan.place's rule (rules: its options)"""
        mine = [(gi, p) for gi, group in enumerate(self.param_groups) for p in group["params"] if p.grad is not None]
        placed = place([p for _, p in mine], type(self).__name__, **rules)
        return [(pb, gb, off, n, gi, p) for (pb, gb, off, n, p), (gi, _) in zip(placed, mine)]

    def _merged_ranges(self, split_key=None, bridge_padding=True):
        """[[param base, grad base, first elem, end elem, [params], group index]]: one entry per launch.  Parameters whose
        split_key differs (Adam: their step counts) never share a range; bridge_padding=False when the update would not keep
        zeros zero (Adam with eps = 0: 0/0)."""
        name = type(self).__name__
        entries = self._entries()
        # Neighbours of one group merge into one launch only when the gap between them is PROVABLY padding (zeros stay
        # zeros under the update): every tensor of the attached models that this optimizer does not update in the same
        # group — frozen parameters, parameters of another group, parameters without a gradient — acts as a barrier.
        # Without an attached model nothing is known about a gap, so only the 64-element alignment padding is bridged.
        entries.sort(key=lambda r: (r[0], r[2]))
        mine = {id(e[5]) for e in entries}
        barriers = {}  # storage base -> sorted [(first elem, end elem)] of tensors that must not be swept up
        for mdl in self._models:
            for q in mdl.parameters():
                if id(q) in mine:
                    continue
                r = dense_range(q.data)
                if r is not None:
                    barriers.setdefault(r[0], []).append((r[1], r[1] + r[2]))
        max_gap = (64 * 2048 if self._models else 64) if bridge_padding else 1

        def gap_is_padding(pb, lo, hi):
            return 0 <= hi - lo < max_gap and not any(b < hi and e > lo for b, e in barriers.get(pb, ()))

        merged = []
        for pb, gb, off, n, gi, p in entries:
            m = merged[-1] if merged else None
            if (m and m[0] == pb and m[1] == gb and m[5] == gi and gap_is_padding(pb, m[3], off)
                    and (split_key is None or split_key(m[4][-1]) == split_key(p))):
                m[3] = off + n
                m[4].append(p)
            else:
                merged.append([pb, gb, off, off + n, [p], gi])
        for _, _, b, _, _, _ in merged:
            if b * 4 % 16:
                raise RuntimeError(f"{name}: flat range not 16-byte aligned")
        return merged

    def _state_view(self, flat, p, b, key):
        """state[p][key] := the view of the flat state array `flat` (starting at element b) that covers p; a tensor already there
        (loaded from a checkpoint, train.py:144, or kept across a re-plan) is carried over into it"""
        r = dense_range(p.data)
        view = torch.as_strided(flat, p.shape, p.stride(), r[1] - b)
        old = self.state[p].get(key)
        if old is not None:
            view.copy_(old.to(device=flat.device, dtype=torch.float32))
        self.state[p][key] = view

    def _ema_slice(self, pb, b, e):
        if self._ema is not None:
            r = dense_range(self._ema[0])
            if r is not None and r[0] == pb and r[1] <= b and e <= r[1] + r[2]:
                return self._ema[1][b - r[1]: e - r[1]]
        return None

    def _check_ema(self, slices):
        if self._ema is not None and not any(fe is not None for fe in slices):
            raise RuntimeError(f"{type(self).__name__}.attach_ema: none of the updated ranges lies in the attached flat array")

    def zero_grad(self, set_to_none=False):
        # gradients live in the model's flat array and are overwritten by the next backward: no memset needed
        if self._models:
            for m in self._models:
                m.mark_grads_clean()
        else:
            super().zero_grad(set_to_none=False)

    def add_param_group(self, group):
        super().add_param_group(group)
        self._plans = None

    def load_state_dict(self, state_dict):
        """torch's loader replaces the per-parameter state by fresh tensors: re-plan at the next step, which copies them into
        the flat state arrays the kernel reads (resume path, train.py:140-146)."""
        super().load_state_dict(state_dict)
        self._plans = None


class SGD(_FlatOptimizer):
    def __init__(self, params, lr=0.0, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, **ignored):
        if dampening != 0.0 or nesterov:
            raise NotImplementedError("dampening / nesterov are not on the hot path")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay)
        super().__init__(params, defaults)

    # one plan per param group: list of (p_flat_slice, g_flat_slice, m_flat_slice, ema_flat_slice or None)
    def _build_plans(self):
        plans = [[] for _ in self.param_groups]
        for pb, gb, b, e, ps, gi in self._merged_ranges():
            fp, fg = flat_views(ps[0], b, e)
            fm = torch.zeros(e - b, dtype=torch.float32, device=fp.device)
            for p in ps:  # expose momentum buffers per parameter (state_dict compatibility)
                self._state_view(fm, p, b, "momentum_buffer")
            plans[gi].append((fp, fg, fm, self._ema_slice(pb, b, e)))
        self._check_ema([fe for segs in plans for *_, fe in segs])
        self._plans = plans

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plans is None:
            self._build_plans()
        for group, segs in zip(self.param_groups, self._plans):
            for fp, fg, fm, fe in segs:
                ops.sgd_step(fp, fg, fm, float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]), float(self.grad_scale),
                             ema=fe, ema_decay=self._ema[2] if fe is not None else 0.0)
        return loss


class Adam(_FlatOptimizer):
    """torch.optim.Adam (decoupled_weight_decay=False: L2 term g += wd*p) whose step is one mi355_adam_step launch per flat range
    (csrc/optim.hip).  Per-parameter state as torch lays it out — state[p] = {step: 0-dim fp32 CPU tensor, exp_avg, exp_avg_sq} —
    so checkpoints move both ways between this class and torch's; exp_avg / exp_avg_sq are views of the flat m / v arrays and the
    step tensors are views of one CPU array that a single add_(1) advances.  A launch range holds parameters of one group with equal
    step counts only (after loading a state whose counts differ, the ranges split there).
    amsgrad, maximize and a tensor lr are not on the hot path; foreach / fused / capturable / differentiable are accepted and ignored."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if amsgrad or maximize:
            raise NotImplementedError("amsgrad / maximize are not on the hot path")
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError("a tensor lr is not on the hot path")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i, b in enumerate(betas):
            if not 0.0 <= float(b) < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # the group keys of torch's Adam (with its defaults for the ignored switches): state dicts load into torch as they are
        defaults = dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps, weight_decay=weight_decay, amsgrad=False,
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=bool(decoupled_weight_decay))
        super().__init__(params, defaults)
        self._steps = None  # CPU fp32 array behind every state[p]['step'] of the planned parameters

    def __setstate__(self, state):
        # (load_state_dict ends here) groups of older or capturable / fused torch checkpoints: the switches this class ignores
        # take torch's defaults again, which describe the layout it keeps (CPU step counts)
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("amsgrad", False)
            group.setdefault("maximize", False)
            group.setdefault("decoupled_weight_decay", False)
            group.update(foreach=None, capturable=False, differentiable=False, fused=None)

    def _step_count(self, p):
        t = self.state[p].get("step")
        return 0 if t is None else int(float(t))

    # one plan per param group: list of [p, g, m, v, ema or None, step count of the range]
    def _build_plans(self):
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError("amsgrad / maximize are not on the hot path")
        plans = [[] for _ in self.param_groups]
        planned = []
        bridge = all(float(g["eps"]) > 0.0 for g in self.param_groups)
        for pb, gb, b, e, ps, gi in self._merged_ranges(split_key=self._step_count, bridge_padding=bridge):
            fp, fg = flat_views(ps[0], b, e)
            fm = torch.zeros(e - b, dtype=torch.float32, device=fp.device)
            fv = torch.zeros(e - b, dtype=torch.float32, device=fp.device)
            t = self._step_count(ps[0])
            for p in ps:
                self._state_view(fm, p, b, "exp_avg")
                self._state_view(fv, p, b, "exp_avg_sq")
                planned.append((p, t))
            plans[gi].append([fp, fg, fm, fv, self._ema_slice(pb, b, e), t])
        self._check_ema([seg[4] for segs in plans for seg in segs])
        self._steps = torch.tensor([float(t) for _, t in planned], dtype=torch.float32)
        for i, (p, _) in enumerate(planned):
            self.state[p]["step"] = self._steps[i]
        self._plans = plans

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plans is None:
            self._build_plans()
        for group, segs in zip(self.param_groups, self._plans):
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                raise NotImplementedError("a tensor lr is not on the hot path")
            decoupled = bool(group.get("decoupled_weight_decay", False))
            for seg in segs:
                fp, fg, fm, fv, fe, t = seg
                ops.adam_step(fp, fg, fm, fv, t, float(lr), group["betas"], float(group["eps"]), float(group["weight_decay"]),
                              decoupled=decoupled, grad_scale=float(self.grad_scale), ema=fe,
                              ema_decay=self._ema[2] if fe is not None else 0.0)
                seg[5] = t + 1
        self._steps.add_(1.0)
        return loss


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay, p *= 1 - lr*wd before the update (weight_decay default 1e-2)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True)

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True


class MADGRAD(_FlatOptimizer):
    """the reference's src.optimizers.MADGRAD (sota_imagenet/optimizers.py:650-770; recipe configs/hydra_exp/54.r50_madgrad.yaml) whose step
    is one mi355_madgrad_step launch per flat range (csrc/optim.hip).  Signature, defaults and state are the reference's — state[p] =
    {grad_sum_sq, s, x0} (views of flat arrays; x0 = the parameter before its first step) and the global counter state["k"], a 1-element
    long CPU tensor — so a state_dict() moves both ways.  The rule, weight decay included (p *= 1 - weight_decay, decoupled and NOT
    scaled by lr), is reproduced as the reference has it.
    One deviation: lr == 0 is accepted.  The recipe reaches the constructor with `lr: 0` merged in from the base config and the
    scheduler writes the real value before the first step, while the reference class raises on lr <= 0 (so the recipe cannot have run
    with the merged default as written)."""

    def __init__(self, params, lr=1e-2, momentum=0.9, weight_decay=0, eps=1e-6):
        if momentum < 0 or momentum >= 1:
            raise ValueError(f"Momentum {momentum} must be in the range [0,1)")
        if lr < 0:
            raise ValueError(f"Learning rate {lr} must be non-negative")
        if weight_decay < 0:
            raise ValueError(f"Weight decay {weight_decay} must be non-negative")
        if eps < 0:
            raise ValueError("Eps must be non-negative")
        defaults = dict(lr=lr, eps=eps, momentum=momentum, weight_decay=weight_decay)
        super().__init__(params, defaults)

    # one plan per param group: list of (p, g, grad_sum_sq, s, x0, ema or None)
    def _build_plans(self):
        plans = [[] for _ in self.param_groups]
        # padding inside a range computes 0 / (cbrt(0) + eps): zeros stay zeros only for eps > 0
        bridge = all(float(g["eps"]) > 0.0 for g in self.param_groups)
        for pb, gb, b, e, ps, gi in self._merged_ranges(bridge_padding=bridge):
            fp, fg = flat_views(ps[0], b, e)
            fq, fs, fx = (torch.zeros(e - b, dtype=torch.float32, device=fp.device) for _ in range(3))
            for p in ps:
                fresh = "grad_sum_sq" not in self.state[p]
                self._state_view(fq, p, b, "grad_sum_sq")
                self._state_view(fs, p, b, "s")
                self._state_view(fx, p, b, "x0")
                if fresh:
                    self.state[p]["x0"].copy_(p.data)
            plans[gi].append((fp, fg, fq, fs, fx, self._ema_slice(pb, b, e)))
        self._check_ema([seg[5] for segs in plans for seg in segs])
        k = self.state["k"] if "k" in self.state else torch.tensor([0], dtype=torch.long)
        self.state["k"] = k.detach().to(device="cpu", dtype=torch.long).reshape(1)  # (a checkpoint may have been mapped to the GPU)
        self._plans = plans

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plans is None:
            self._build_plans()
        k = int(self.state["k"].item())
        for group, segs in zip(self.param_groups, self._plans):
            for fp, fg, fq, fs, fx, fe in segs:
                ops.madgrad_step(fp, fg, fq, fs, fx, k, float(group["lr"]), float(group["momentum"]), float(group["weight_decay"]),
                                 float(group["eps"]), grad_scale=float(self.grad_scale), ema=fe,
                                 ema_decay=self._ema[2] if fe is not None else 0.0)
        self.state["k"] += 1
        return loss


class AdaiS(_FlatOptimizer):
    """the reference's src.optimizers.AdaiS (sota_imagenet/optimizers.py:522-641; recipe configs/hydra_exp/50.r50_adais.yaml): Adai with
    stable / decoupled weight decay.  Every element's momentum beta1 depends on the mean of the bias-corrected second moment over ALL
    parameters of ALL groups, so a step is three device stages on the current stream (csrc/optim.hip) with nothing read back:
    mi355_adais_moments per flat range, one mi355_adais_mean, mi355_adais_step per flat range.  Signature, defaults, validation and
    state are the reference's — state[p] = {step: int, exp_avg, exp_avg_sq (from ema_norm_init), beta1_prod (from 1)}, the tensors
    being views of flat arrays — so a state_dict() moves both ways.  Padding inside a range holds exp_avg_sq = 0 and is not counted in
    param_size: it never enters the mean.  A launch range holds parameters of one group with equal step counts only."""

    def __init__(self, params, lr=0, betas=(0.1, 0.99), eps=1e-3, weight_decay=0, ema_norm_init=1e-3):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0]:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.ema_norm_init = ema_norm_init
        self._planned = []   # the parameters whose state["step"] a step advances
        self._ws = None      # float64 partial sums of every range, back to back
        self._mean = None    # exp_avg_sq_hat_mean of the last step: one float32 on the device

    @property
    def exp_avg_sq_hat_mean(self):
        """the statistic of the last step (a 1-element CUDA tensor the step kernels read; None before the first step)"""
        return self._mean

    def _step_count(self, p):
        return int(self.state[p].get("step", 0))

    # one plan per param group: list of [p, g, exp_avg, exp_avg_sq, beta1_prod, ema or None, step count of the range, workspace slice]
    def _build_plans(self):
        plans = [[] for _ in self.param_groups]
        planned, total, dev = [], 0, None
        for pb, gb, b, e, ps, gi in self._merged_ranges(split_key=self._step_count):
            fp, fg = flat_views(ps[0], b, e)
            if dev is not None and fp.device != dev:
                raise RuntimeError("AdaiS: all parameters must live on one device (the mean is taken there)")
            dev = fp.device
            # zeros first, the initial values through the per-parameter views: padding keeps exp_avg_sq = 0 and stays out of the mean
            fm, fv, fb = (torch.zeros(e - b, dtype=torch.float32, device=dev) for _ in range(3))
            for p in ps:
                fresh = "exp_avg_sq" not in self.state[p]
                self._state_view(fm, p, b, "exp_avg")
                self._state_view(fv, p, b, "exp_avg_sq")
                self._state_view(fb, p, b, "beta1_prod")
                if fresh:
                    self.state[p]["step"] = 0
                    self.state[p]["exp_avg_sq"].fill_(self.ema_norm_init)
                    self.state[p]["beta1_prod"].fill_(1.0)
                planned.append(p)
            cnt = ops.adais_workspace_elems(e - b)
            plans[gi].append([fp, fg, fm, fv, fb, self._ema_slice(pb, b, e), self._step_count(ps[0]), (total, total + cnt)])
            total += cnt
        self._check_ema([seg[5] for segs in plans for seg in segs])
        self._planned = planned
        self._param_size = sum(p.numel() for p in planned)
        if planned:
            self._ws = torch.zeros(total, dtype=torch.float64, device=dev)
            self._mean = torch.zeros(1, dtype=torch.float32, device=dev)
            for segs in plans:
                for seg in segs:
                    seg[7] = self._ws[seg[7][0]: seg[7][1]]
        self._plans = plans

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plans is None:
            self._build_plans()
        if not self._planned:
            return loss
        gs = float(self.grad_scale)
        for group, segs in zip(self.param_groups, self._plans):
            for seg in segs:
                ops.adais_moments(seg[1], seg[3], seg[6] + 1, float(group["betas"][1]), seg[7], grad_scale=gs)
        ops.adais_mean(self._ws, self._param_size, self._mean)
        for group, segs in zip(self.param_groups, self._plans):
            for seg in segs:
                fp, fg, fm, fv, fb, fe, t, _ = seg
                ops.adais_step(fp, fg, fm, fv, fb, self._mean, t + 1, float(group["lr"]), group["betas"], float(group["eps"]),
                               float(group["weight_decay"]), grad_scale=gs, ema=fe, ema_decay=self._ema[2] if fe is not None else 0.0)
                seg[6] = t + 1
        for p in self._planned:
            self.state[p]["step"] += 1
        return loss


def _runs(indices, keys):
    """[(key, first index, last index)] of the runs of equal keys[index] among consecutive indices"""
    return [(k, run[0], run[-1]) for k, run in ((k, list(run)) for k, run in groupby(indices, keys.__getitem__))]


# one pair of parameter / gradient storage in a layer-wise plan: the two storages as flat arrays over the pair's element range [lo, hi), the first
# moment of that range, the moving average's slice of it or None, (first item, end item), [(group index, first item, end item)] of the groups present
_LwSeg = namedtuple("_LwSeg", "p g m ema items by_group")


def _unit_strides(ndim):
    """strides of the view that shows one value per slot in a tensor's own shape: 1 on dim 0 of a unit-wise tensor, 0 everywhere else"""
    return ((1,) + (0,) * (ndim - 1)) if ndim > 1 else (0,) * ndim


# the same for a unit-wise plan: + (first piece, end piece), (first whole item, end) and the pair's first entry of the partial sums
_LwUnitSeg = namedtuple("_LwUnitSeg", "p g m ema items by_group pieces whole partial0")


class _Layerwise(_FlatOptimizer):
    """what NovogradApex, MyNovograd, AdamLayerwise and MyAdai share: the work-item plan (plan_tables, the pure host part on item_plan.py;
    _build_plans adds what needs the device: one _LwSeg per storage pair) and the three stages of csrc/optim_lw.hip —
    (a) one lw_sumsq launch per (parameter storage, gradient storage) pair, (b) one lw_coef launch per param group, (c) one lw_update
    launch per param group (and storage pair) — 3 launches per step for a flat model in one group, 1 + 2 + 2 with filter_from_wd.
    The first moment is a view of a flat array as in the other native optimizers.  The second moment, which the reference keeps as a
    full-size tensor holding ONE value, is one float32 slot per tensor on the device: state[p][key] is a stride-0 view of it with the
    parameter's shape, state_dict() returns dense copies (the reference loads them), load_state_dict() accepts the reference's dense tensors
    (checked once for min == max) and keeps element 0.

    unitwise_norm=True (NovogradApex and MyNovograd; the reference's optimizers.py:16-22) takes the statistic per SLOT — a whole tensor with
    ndim <= 1, one index of dim 0 otherwise — and it is the NORM of the slot, not the sum of squares, for the 1-D tensors too.  The plan is
    plan_unit_tables; a step is unit sums and 1-D sums per storage pair, one lw_unit_coef and one lw_unit_update per param group: 4 launches on
    a flat model in one group, 1 + 1 + 2 + 2 with filter_from_wd.  The second moment is one float32 per slot on the device; state[p][key] is a
    strided view of it with the parameter's shape (stride 1 on dim 0 and 0 elsewhere, all zeros for the 1-D tensors); load_state_dict()
    accepts the reference's dense tensors, keeps the first element of every unit and allows inside a unit the relative spread the
    reference's own float32 run shows: 2^-23 / (1 - beta2), one rounding per step damped by beta2.  There is no CPU path: with
    unitwise_norm=True the constructor and add_param_group raise NotImplementedError for any parameter that is not a CUDA tensor."""

    _rule = ops.LW_NORMGRAD
    _m_key, _v_key = "exp_avg", "exp_avg_sq"
    _param_stat = False  # MyNovograd: the statistic is taken of the parameter, not of the gradient

    def _v_init(self, group):
        return self.ema_norm_init

    def _coef_args(self, group):
        """(flags, beta1, beta2, eps) of stage (b) for one group"""
        raise NotImplementedError

    def _wd_eps(self):
        return None

    @staticmethod
    def plan_tables(tensors, W):
        """the host side of a plan.  tensors: [(param base, grad base, first elem, numel, group index)] in param-group order; W:
        ops.lw_item_elems().  Returns a dict:
          items    item_plan.storage_pairs' work items: storage pair by storage pair, inside it group by group; tensor index = index into `tensors`
          tensors  [(first item, item count, numel)] per tensor: the records of lw_coef
          pairs    [(lo, hi, first item, end item, [(group index, first item, end item)] of the groups present in the pair, tensor indices)]
          groups   [(group index, first tensor, end tensor)] of the groups present: the tensors of a group are consecutive"""
        items, spans, pairs = storage_pairs(tensors, W)
        group_of = [t[4] for t in tensors]
        return dict(items=items, tensors=[(first, count, float(t[3])) for (first, count), t in zip(spans, tensors)],
                    pairs=[(lo, hi, i0, i1, [(gi, spans[a][0], sum(spans[b])) for gi, a, b in _runs(ts, group_of)], ts) for lo, hi, i0, i1, ts in pairs],
                    groups=[(gi, a, b + 1) for gi, a, b in _runs(range(len(tensors)), group_of)])

    @staticmethod
    def plan_unit_tables(tensors, W):
        """the host side of a unit-wise plan.  tensors: [(param base, grad base, first elem, numel, group index, unit_len)] in param-group
        order.  Returns item_plan.plan_units' dict (items, tensors, pieces, whole, slots, pairs) with two additions: every entry of `pairs`
        ends with [(group index, first item, end item)] of the groups present in the pair, and
          groups   [(group index, first slot, end slot)] of the groups present: slots are numbered tensor by tensor in param-group order, so the
                   slots of a group are consecutive"""
        tab = plan_units([t[:4] + (t[5],) for t in tensors], W)
        lw = _Layerwise.plan_tables([t[:5] for t in tensors], W)
        assert lw["items"] == tab["items"]
        ends = [s0 + t[3] // t[5] for (_, _, s0), t in zip(tab["tensors"], tensors)]
        tab["pairs"] = [pr + (lp[4],) for pr, lp in zip(tab["pairs"], lw["pairs"])]
        tab["groups"] = [(gi, tab["tensors"][a][2], ends[b - 1]) for gi, a, b in lw["groups"]]
        return tab

    def _check_unit_placement(self, group):
        """unitwise_norm=True: placement is checked when the parameters arrive (there is no CPU path to fall back to)"""
        for p in group["params"]:
            if not p.is_cuda:
                raise NotImplementedError(f"unitwise_norm=True has no CPU path: {type(self).__name__} needs CUDA parameters, got a "
                                          f"{p.device.type} tensor of shape {tuple(p.shape)}")

    def add_param_group(self, group):
        super().add_param_group(group)
        if getattr(self, "unitwise_norm", False):
            self._check_unit_placement(self.param_groups[-1])

    def _build_unit_plans(self, entries):
        dev, name = entries[0][5].device, type(self).__name__
        tab = self.plan_unit_tables([e[:5] + (unit_len(e[5].shape, e[5].stride(), True, name),) for e in entries], ops.lw_item_elems())
        self._items, self._tensors = pack_records(tab["items"], dev), pack_records(tab["tensors"], dev)
        self._pieces = pack_records(tab["pieces"], dev) if tab["pieces"] else None
        self._whole = pack_records(tab["whole"], dev) if tab["whole"] else None
        ns = len(tab["slots"])
        self._slots = torch.tensor(tab["slots"], dtype=torch.int32, device=dev)
        self._partial = torch.zeros(len(tab["pieces"]) + len(tab["whole"]), dtype=torch.float64, device=dev)
        self._sums = torch.zeros(ns, dtype=torch.float64, device=dev)  # S per slot of the last step
        self._den = torch.zeros(ns, dtype=torch.float32, device=dev)
        self.slot_ranges = [(s0, e[3] // u) for (_, u, s0), e in zip(tab["tensors"], entries)]  # per planned tensor: (first slot, slots)
        self._v = self._make_unit_v(entries, dev, ns)
        self._coefs = tab["groups"]
        for lo, hi, i0, i1, pc, wh, k0, ts, by_group in tab["pairs"]:
            fp, fg, fm = self._pair_state(entries, ts, lo, hi, dev)
            self._segs.append(_LwUnitSeg(fp, fg, fm, self._ema_slice(entries[ts[0]][0], lo, hi), (i0, i1), by_group, pc, wh, k0))

    def _pair_state(self, entries, ts, lo, hi, dev):
        """the flat arrays of one storage pair over [lo, hi): parameters, gradients and a new first moment that state[p] views"""
        ps = [entries[t][5] for t in ts]
        fp, fg = flat_views(ps[0], lo, hi)
        fm = torch.zeros(hi - lo, dtype=torch.float32, device=dev)
        for p in ps:
            fresh = self._m_key not in self.state[p]
            self._state_view(fm, p, lo, self._m_key)
            if fresh:
                self.state[p].setdefault("step", 0)
        return fp, fg, fm

    def _make_unit_v(self, entries, dev, n_slots):
        """one float32 per slot; state[p][v key] becomes a view of the tensor's slots with the parameter's shape: stride 1 on dim 0 (a unit-wise
        tensor) and 0 elsewhere.  A tensor already there gives the first element of every unit."""
        v = torch.empty(n_slots, dtype=torch.float32, device=dev)
        for (s0, cnt), (_, _, _, _, gi, p) in zip(self.slot_ranges, entries):
            old = self.state[p].get(self._v_key)
            if old is None:
                v[s0:s0 + cnt] = self._v_init(self.param_groups[gi])
            else:
                v[s0:s0 + cnt] = old.reshape(cnt, -1)[:, 0].to(device=dev, dtype=torch.float32)
            self.state[p][self._v_key] = torch.as_strided(v, p.shape, _unit_strides(p.dim()), s0)
        return v

    def _unit_step(self, gs):
        src_scale = 1.0 if self._param_stat else gs
        nt, ns = self._tensors.shape[0], self._den.numel()
        for seg in self._segs:
            (pa, pb), (wa, wb), k0 = seg.pieces, seg.whole, seg.partial0
            k1 = k0 + pb - pa
            src = seg.p if self._param_stat else seg.g
            if pb > pa:
                ops.lw_unit_sumsq(src, self._pieces[pa:pb], self._partial[k0:k1], ns, scale=src_scale)
            if wb > wa:
                ops.lw_sumsq(src, self._whole[wa:wb], self._partial[k1:k1 + wb - wa], nt, scale=src_scale)
        for gi, s0, s1 in self._coefs:
            _, _, b2, eps = self._coef_args(self.param_groups[gi])
            ops.lw_unit_coef(self._partial, self._slots[s0:s1], self._v[s0:s1], self._den[s0:s1], self._sums[s0:s1], b2, eps)
        for seg in self._segs:
            for gi, i0, i1 in seg.by_group:
                group = self.param_groups[gi]
                ops.lw_unit_update(self._rule, seg.p, seg.g, seg.m, self._items[i0:i1], self._tensors, self._den, self._coef_args(group)[1],
                                   float(group["lr"]), float(group["weight_decay"]), wd_eps=self._wd_eps(), grad_scale=gs, ema=seg.ema,
                                   ema_decay=self._ema[2] if seg.ema is not None else 0.0)

    def _build_plans(self):
        entries = self._entries(aligned=True, one_device=True)
        self._planned = [e[5] for e in entries]
        self._segs, self._coefs = [], []
        if not entries:
            self._plans = []
            return
        if getattr(self, "unitwise_norm", False):
            self._build_unit_plans(entries)
            self._check_ema([seg.ema for seg in self._segs])
            self._plans = self._segs
            return
        dev, nt = entries[0][5].device, len(entries)
        tab = self.plan_tables([e[:5] for e in entries], ops.lw_item_elems())
        self._items = pack_records(tab["items"], dev)
        self._tensors = pack_records(tab["tensors"], dev, TENSOR_FIELDS)
        self._partial = torch.zeros(len(tab["items"]), dtype=torch.float64, device=dev)
        self._sums = torch.zeros(nt, dtype=torch.float64, device=dev)   # S per tensor of the last step (tensor order = group by group)
        self._coef = torch.zeros(nt, 4, dtype=torch.float32, device=dev)
        self._v = self._make_v(entries, dev)
        self._coefs = tab["groups"]
        for lo, hi, i0, i1, by_group, ts in tab["pairs"]:
            fp, fg, fm = self._pair_state(entries, ts, lo, hi, dev)
            self._segs.append(_LwSeg(fp, fg, fm, self._ema_slice(entries[ts[0]][0], lo, hi), (i0, i1), by_group))
        self._check_ema([seg.ema for seg in self._segs])
        self._plans = self._segs

    def _make_v(self, entries, dev):
        """one float32 slot per tensor; state[p][v key] becomes a stride-0 view of its slot"""
        v = torch.empty(len(entries), dtype=torch.float32, device=dev)
        for t, (_, _, _, _, gi, p) in enumerate(entries):
            old = self.state[p].get(self._v_key)
            if old is None:
                v[t] = self._v_init(self.param_groups[gi])
            else:
                v[t] = old[(0,) * old.dim()].to(device=dev, dtype=torch.float32)
            self.state[p][self._v_key] = torch.as_strided(v, p.shape, (0,) * p.dim(), t)
        return v

    def _adai_mean(self):
        return 1.0

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        mean = self._adai_mean()  # (before the plan creates state: the reference's first step sees none)
        if self._plans is None:
            self._build_plans()
        if not self._planned:
            return loss
        gs = float(self.grad_scale)
        if getattr(self, "unitwise_norm", False):
            self._unit_step(gs)
            for p in self._planned:
                self.state[p]["step"] += 1
            return loss
        nt = self._sums.numel()
        for seg in self._segs:
            i0, i1 = seg.items
            ops.lw_sumsq(seg.p if self._param_stat else seg.g, self._items[i0:i1], self._partial[i0:i1], nt, scale=1.0 if self._param_stat else gs)
        for gi, t0, t1 in self._coefs:
            group = self.param_groups[gi]
            flags, b1, b2, eps = self._coef_args(group)
            ops.lw_coef(self._rule, flags, self._partial, self._tensors[t0:t1], self._v[t0:t1], self._coef[t0:t1], self._sums[t0:t1], b1, b2, eps,
                        float(group["lr"]), float(group["weight_decay"]), mean=mean)
        for seg in self._segs:
            for gi, i0, i1 in seg.by_group:
                ops.lw_update(self._rule, seg.p, seg.g, seg.m, self._items[i0:i1], self._coef, float(self.param_groups[gi]["lr"]),
                              wd_eps=self._wd_eps(), grad_scale=gs, ema=seg.ema, ema_decay=self._ema[2] if seg.ema is not None else 0.0)
        for p in self._planned:
            self.state[p]["step"] += 1
        return loss

    def state_dict(self):
        """the second moment as the reference keeps it: a dense tensor of the parameter's shape"""
        sd = super().state_dict()
        sd["state"] = {k: {key: (v.contiguous() if torch.is_tensor(v) and key == self._v_key else v) for key, v in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        loaded = [(p, st[self._v_key]) for p, st in self.state.items() if torch.is_tensor(st.get(self._v_key))]
        if loaded and getattr(self, "unitwise_norm", False):
            self._load_unit_v(loaded)
        elif loaded:
            # the reference's tensors hold one value each: checked here, once, then element 0 is kept
            spread = torch.stack([(t.max() - t.min()).float() for _, t in loaded])
            if bool((spread != 0).any()):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {self._v_key} must hold one value per tensor (min == max)")
            for p, t in loaded:
                self.state[p][self._v_key] = t.reshape(-1)[0].clone().expand(t.shape)

    def _load_unit_v(self, loaded):
        """the reference's dense second moments: one value per unit up to the jitter its own float32 run shows (_foreach_add_ rounds its vector
        body and its scalar tail differently) — a relative spread of 2^-23 / (1 - beta2) inside a unit, beyond which ValueError.  The first
        element of every unit is kept; a layer-wise state (one value per tensor) loads as it is."""
        beta2 = {id(p): float(self._coef_args(g)[2]) for g in self.param_groups for p in g["params"]}
        rows = [(t.reshape(t.shape[0] if t.dim() > 1 else 1, -1), 2.0 ** -23 / (1.0 - beta2[id(p)])) for p, t in loaded]
        bad = torch.stack([((r.max(1).values - r.min(1).values).double() > tol * r.abs().max(1).values.double()).any() for r, tol in rows])
        if bool(bad.any()):
            raise ValueError(f"{type(self).__name__}.load_state_dict: {self._v_key} must hold one value per unit (a relative spread inside a unit "
                             "of at most 2^-23 / (1 - beta2))")
        for (p, t), (r, _) in zip(loaded, rows):
            first = r[:, 0].clone()
            self.state[p][self._v_key] = torch.as_strided(first, t.shape, _unit_strides(t.dim()))


def _lw_checks(lr, eps, betas):
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: {}".format(lr))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {}".format(eps))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))


class NovogradApex(_Layerwise):
    """the reference's src.optimizers.NovogradApex (sota_imagenet/optimizers.py:189-290; recipe configs/hydra_exp/46.r50_nov.yaml): the first
    moment of the gradient divided by sqrt of the running SUM of squares of the tensor's gradient; decoupled weight decay, or with wd_eps a
    decay of |p| - wd_eps only (p -= lr*wd*max(|p| - wd_eps, 0)*sign(p)).  Signature, defaults, checks and state (step: int, exp_avg,
    exp_avg_sq) are the reference's.  unitwise_norm=True takes the NORM of the gradient per output unit instead (see _Layerwise): native on CUDA
    parameters only — there is no CPU path, the constructor raises NotImplementedError for anything else."""

    def __init__(self, params, lr=1e-3, betas=(0.95, 0), eps=1e-8, weight_decay=0, ema_norm_init=1e-3, unitwise_norm=False, wd_eps=None):
        _lw_checks(lr, eps, betas)
        self.unitwise_norm = unitwise_norm  # (before the groups arrive: add_param_group checks their placement)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.ema_norm_init = ema_norm_init
        self.wd_eps = wd_eps

    def _coef_args(self, group):
        return (ops.LW_SOFT_WD if self.wd_eps is not None else 0), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])

    def _wd_eps(self):
        return None if self.wd_eps is None else float(self.wd_eps)


class AdamLayerwise(_Layerwise):
    """the reference's src.optimizers.AdamLayerwise (sota_imagenet/optimizers.py:293-397; recipe configs/hydra_exp/49.r50_nov-adam.yaml):
    NovogradApex with the MEAN of squares of the tensor's gradient, and stable_wd (p *= 1 - lr*wd/den).  weight_adapt is not on the hot path."""

    def __init__(self, params, lr=1e-3, betas=(0.95, 0), eps=1e-6, weight_decay=0, ema_norm_init=1e-3, weight_adapt=False, stable_wd=False):
        _lw_checks(lr, eps, betas)
        if weight_adapt:
            raise NotImplementedError("weight_adapt=True is not on the hot path")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.ema_norm_init = ema_norm_init
        self.weight_adapt = weight_adapt
        self.stable_wd = stable_wd

    def _coef_args(self, group):
        return ops.LW_MEAN | (ops.LW_STABLE_WD if self.stable_wd else 0), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])


class MyNovograd(_Layerwise):
    """the reference's src.optimizers.MyNovograd (sota_imagenet/optimizers.py:35-161; recipe configs/hydra_exp/47.r50_my-nov.yaml): the update
    is the first moment of the gradient divided by sqrt of a running sum of squares — which the class takes of the PARAMETER, not of the gradient
    (its grad_norms are built from params_with_grad, :138).  Reproduced as it is.  State keys are ema_grad and ema_norm; eps is an attribute of
    the optimizer and ema_norm_init a group key, as there.  unitwise_norm=True (recipe configs/hydra_exp/48.r50_my-nov-unit.yaml) takes the NORM of
    the parameter per output unit instead (see _Layerwise): native on CUDA parameters only — there is no CPU path, the constructor raises
    NotImplementedError for anything else."""

    _rule = ops.LW_NOVOGRAD
    _m_key, _v_key = "ema_grad", "ema_norm"
    _param_stat = True

    def __init__(self, params, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, ema_norm_init=1e-3, unitwise_norm=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self.unitwise_norm = unitwise_norm  # (before the groups arrive: add_param_group checks their placement)
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay, ema_norm_init=ema_norm_init))
        self.eps = eps

    def _v_init(self, group):
        return group["ema_norm_init"]

    def _coef_args(self, group):
        return 0, float(group["betas"][0]), float(group["betas"][1]), float(self.eps)


class MyAdai(_Layerwise):
    """the reference's src.optimizers.MyAdai (sota_imagenet/optimizers.py:400-519; recipe configs/hydra_exp/55.r50_adai_2.yaml) with
    per_layer=True: every tensor's momentum beta1 = clip(1 - vt/mean * beta0, 0, 1 - eps) from vt = v0*beta2 + (1 - beta2)*mean(g^2).
    The class never writes vt back into its state (it rebinds a local, :489): state[p]["exp_avg_sq"] stays the Python float it was created
    with, the "mean over layers" is the mean of those constants (ema_norm_init itself on the very first step, :456-459) and a step has no memory
    of the one before.  Reproduced as it is; floats that a loaded state carries are kept and used.  per_layer=False is not on the hot path."""

    _rule = ops.LW_ADAI

    def __init__(self, params, lr=1e-3, betas=(0.1, 0.99), eps=1e-3, weight_decay=0, ema_norm_init=1e-3, sgd_mom=False, sqrt_mom=False,
                 stable_wd=False, per_layer=True):
        _lw_checks(lr, eps, betas)
        if not per_layer:
            raise NotImplementedError("per_layer=False is not on the hot path")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.ema_norm_init = ema_norm_init
        self.sgd_mom = sgd_mom
        self.sqrt_mom = sqrt_mom
        self.stable_wd = stable_wd
        self.per_layer = per_layer

    def _make_v(self, entries, dev):
        for _, _, _, _, _, p in entries:
            self.state[p].setdefault("exp_avg_sq", self.ema_norm_init)
        return torch.tensor([float(self.state[e[5]]["exp_avg_sq"]) for e in entries], dtype=torch.float64, device=dev)

    def _adai_mean(self):
        if len(self.state) == 0:
            return float(self.ema_norm_init)
        return float(sum(v["exp_avg_sq"] for v in self.state.values()) / len(self.state))

    def _coef_args(self, group):
        flags = (ops.LW_MEAN | (ops.LW_SGD_MOM if self.sgd_mom else 0) | (ops.LW_SQRT_MOM if self.sqrt_mom else 0)
                 | (ops.LW_STABLE_WD if self.stable_wd else 0))
        return flags, float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])

    def state_dict(self):
        return _FlatOptimizer.state_dict(self)

    def load_state_dict(self, state_dict):
        _FlatOptimizer.load_state_dict(self, state_dict)


# one pair of parameter / gradient storage in an AdamP plan: the two storages as flat arrays over the pair's element range, both moments of that
# range, the moving average's slice or None, [(group index, first item, end item)] of the groups present and the launches of stage (a):
# [(group index, first piece, end piece, first entry of the partial sums)]
_AdamPSeg = namedtuple("_AdamPSeg", "p g m v ema by_group sums")


class AdamP(_FlatOptimizer):
    """`adamp.AdamP` (the reference's recipes configs/hydra_exp/51.r50_adamp.yaml and 52.r50_adamp_low-eps.yaml): Adam whose update loses its
    component along the weight, and whose weight decay is scaled by wd_ratio, for every tensor with more than one dimension whose gradient is
    nearly orthogonal to it — per output unit first, then per whole tensor; cosine under delta / sqrt(row length).

    Provenance: the `adamp` package is neither in the reference tree nor available where this was written.  The rule is the published
    adamp.AdamP.step (package 0.3.0) written down from memory of the public package (include/mi355rn.h states it); parity is against the torch
    restatement of tests/adamp_common.py and is unpinned against the package itself.  pytorch_tools.optim.adamp.AdamP (recipes 12, 13) is a
    modified variant whose code is not available: it does not resolve.

    Signature, group keys and state are the package's — state[p] = {step: int, exp_avg, exp_avg_sq}, the tensors being views of flat arrays, one
    per storage pair — so a state_dict() is meant to move both ways.  A step is three stages of csrc/optim_adamp.hip on the current stream with
    nothing read back (the package asks the host `cosine_sim.max() < ...` per tensor): adamp_unit_sums per storage pair and param group over the
    pieces of the group's ndim > 1 tensors, adamp_coef per param group, adamp_update per storage pair and param group: 3 launches on a flat model
    in one group, at most 5 with filter_from_wd (its no-decay group holds 1-D tensors only: no pieces).  All planned tensors of one group share
    `step`; a loaded state that differs inside a group raises ValueError.  There is no CPU path: parameters that are not CUDA tensors raise
    NotImplementedError at construction and in add_param_group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, delta=0.1, wd_ratio=0.1, nesterov=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        for i, b in enumerate(betas):
            if not 0.0 <= float(b) < 1.0:
                raise ValueError(f"Invalid beta parameter at index {i}: {b}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 <= delta:
            raise ValueError(f"Invalid delta value: {delta}")
        if not 0.0 <= wd_ratio:
            raise ValueError(f"Invalid wd_ratio value: {wd_ratio}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, delta=delta, wd_ratio=wd_ratio, nesterov=nesterov))
        self._planned, self._segs, self._modes = [], [], None
        self.slot_ranges = []

    def add_param_group(self, group):
        super().add_param_group(group)
        for p in self.param_groups[-1]["params"]:
            if not p.is_cuda:
                raise NotImplementedError(f"AdamP has no CPU path: it needs CUDA parameters, got a {p.device.type} tensor of shape "
                                          f"{tuple(p.shape)}")

    @property
    def projection_modes(self):
        """what the last step decided, one int32 per planned tensor in param-group order, on the device: 0 no projection, 1 per output unit,
        2 per whole tensor (None before the first step)"""
        return self._modes

    @staticmethod
    def plan_tables(tensors, W):
        """the host side of a plan.  tensors: [(param base, grad base, first elem, numel, group index, unit_len, kind)] in param-group order,
        kind 1 for ndim > 1; W: ops.lw_item_elems().  Returns item_plan.plan_units' dict (items, tensors, pieces, whole, slots, pairs) and
          decide      [(slot0, slot count, unit_len, kind)] per tensor: the records of stage (b)
          sum_pieces  the table of stage (a): a pair's `pieces`, then — plan_units takes a tensor whose unit is the whole tensor, dim 0 of 1,
                      through whole-tensor items — the whole items of its kind-1 tensors as pieces { off, len, slot }
          groups      [(group index, first tensor, end tensor)] of the groups present
        and every entry of `pairs` ends with [(group index, first item, end item)] of the groups present in the pair and the launches of stage
        (a), [(group index, first, end in sum_pieces, first entry of the partial sums)]: consecutive records whose entries are consecutive"""
        tab = plan_units([t[:4] + (t[5],) for t in tensors], W)
        lw = _Layerwise.plan_tables([t[:5] for t in tensors], W)
        assert lw["items"] == tab["items"]
        slot0 = [r[2] for r in tab["tensors"]]
        tab["decide"] = [(s0, t[3] // t[5], t[5], int(t[6])) for s0, t in zip(slot0, tensors)]
        tab["groups"] = lw["groups"]
        tensor_of_slot = [i for i, t in enumerate(tensors) for _ in range(t[3] // t[5])]
        sum_pieces, pairs = [], []
        for (lo, hi, i0, i1, (pa, pb), (wa, wb), k0, ts), lp in zip(tab["pairs"], lw["pairs"]):
            # (record, its entry of the partial sums, group): the unit pieces, then the whole items of the kind-1 tensors
            recs = [(pc, k0 + j, tensors[tensor_of_slot[pc[2]]][4]) for j, pc in enumerate(tab["pieces"][pa:pb])]
            recs += [((o, ln, slot0[t]), k0 + pb - pa + j, tensors[t][4]) for j, (o, ln, t) in enumerate(tab["whole"][wa:wb]) if tensors[t][6]]
            sums = []
            for pc, k, gi in recs:
                if sums and sums[-1][0] == gi and sums[-1][3] + sums[-1][2] - sums[-1][1] == k:
                    sums[-1][2] += 1
                else:
                    sums.append([gi, len(sum_pieces), len(sum_pieces) + 1, k])
                sum_pieces.append(pc)
            pairs.append((lo, hi, i0, i1, (pa, pb), (wa, wb), k0, ts, lp[4], [tuple(x) for x in sums]))
        tab["sum_pieces"], tab["pairs"] = sum_pieces, pairs
        return tab

    def _step_count(self, p):
        return int(self.state[p].get("step", 0))

    def _group_steps(self, params_of):
        """{group index: the step count its tensors share}; ValueError where they differ inside a group"""
        out = {}
        for gi, ps in params_of.items():
            counts = {self._step_count(p) for p in ps}
            if len(counts) > 1:
                raise ValueError(f"AdamP: the tensors of param group {gi} carry different step counts {sorted(counts)}: one launch takes one "
                                 "bias correction")
            out[gi] = counts.pop() if counts else 0
        return out

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._group_steps({gi: [p for p in g["params"] if "step" in self.state.get(p, {})] for gi, g in enumerate(self.param_groups)})

    def _build_plans(self):
        entries = self._entries(aligned=True, one_device=True)
        self._planned = [e[5] for e in entries]
        self._segs, self._groups = [], []
        if not entries:
            self._plans = []
            return
        dev, name = entries[0][5].device, type(self).__name__
        by_group = {}
        for e in entries:
            by_group.setdefault(e[4], []).append(e[5])
        self._gstep = self._group_steps(by_group)
        tab = self.plan_tables([e[:5] + (unit_len(e[5].shape, e[5].stride(), True, name), e[5].dim() > 1) for e in entries], ops.lw_item_elems())
        self._items, self._tensors = pack_records(tab["items"], dev), pack_records(tab["tensors"], dev)
        self._sum_pieces = pack_records(tab["sum_pieces"], dev) if tab["sum_pieces"] else None
        ns, nt = len(tab["slots"]), len(entries)
        self._slots = torch.tensor(tab["slots"], dtype=torch.int32, device=dev)
        self._decide = torch.tensor(tab["decide"], dtype=torch.int32, device=dev)
        self._partial = torch.zeros(len(tab["pieces"]) + len(tab["whole"]), 4, dtype=torch.float64, device=dev)
        self._coef = torch.zeros(ns, 2, dtype=torch.float32, device=dev)
        self._wdf = torch.ones(nt, dtype=torch.float32, device=dev)
        self._modes = torch.zeros(nt, dtype=torch.int32, device=dev)
        self.slot_ranges = [(s0, cnt) for s0, cnt, _, _ in tab["decide"]]  # per planned tensor: (first slot, slots)
        self._groups = tab["groups"]
        for lo, hi, i0, i1, _, _, _, ts, items_by_group, sums in tab["pairs"]:
            ps = [entries[t][5] for t in ts]
            fp, fg = flat_views(ps[0], lo, hi)
            fm, fv = (torch.zeros(hi - lo, dtype=torch.float32, device=dev) for _ in range(2))
            for p in ps:
                self._state_view(fm, p, lo, "exp_avg")
                self._state_view(fv, p, lo, "exp_avg_sq")
                self.state[p]["step"] = self._step_count(p)
            self._segs.append(_AdamPSeg(fp, fg, fm, fv, self._ema_slice(entries[ts[0]][0], lo, hi), items_by_group, sums))
        self._check_ema([seg.ema for seg in self._segs])
        self._plans = self._segs

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._plans is None:
            self._build_plans()
        if not self._planned:
            return loss
        gs, ns = float(self.grad_scale), self._coef.shape[0]

        def adam(gi):
            group = self.param_groups[gi]
            return dict(step=self._gstep[gi] + 1, betas=group["betas"], eps=float(group["eps"]), nesterov=bool(group["nesterov"]), grad_scale=gs)

        for seg in self._segs:
            for gi, a, b, k in seg.sums:
                ops.adamp_unit_sums(seg.p, seg.g, seg.m, seg.v, self._sum_pieces[a:b], self._partial[k:k + b - a], ns, **adam(gi))
        for gi, t0, t1 in self._groups:
            group = self.param_groups[gi]
            ops.adamp_coef(self._partial, self._slots, self._decide[t0:t1], self._coef, self._wdf[t0:t1], self._modes[t0:t1], float(group["lr"]),
                           float(group["weight_decay"]), float(group["eps"]), float(group["delta"]), float(group["wd_ratio"]))
        for seg in self._segs:
            for gi, i0, i1 in seg.by_group:
                ops.adamp_update(seg.p, seg.g, seg.m, seg.v, self._items[i0:i1], self._tensors, self._coef, self._wdf,
                                 lr=float(self.param_groups[gi]["lr"]), ema=seg.ema, ema_decay=self._ema[2] if seg.ema is not None else 0.0,
                                 **adam(gi))
        for gi in self._gstep:
            self._gstep[gi] += 1
        for p in self._planned:
            self.state[p]["step"] += 1
        return loss
