"""`SGD`, `Adam`, `AdamW`, `MADGRAD` and `AdaiS` plugins: torch.optim-compatible optimizers whose step is fused HIP kernels over flat ranges.

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
"""
import torch
from torch.optim import Optimizer

from . import ops


def _dense_range(t):
    """(storage base ptr, first elem, numel) if `t` covers a dense memory range (any permutation of strides)."""
    n = t.numel()
    sizes_strides = sorted(zip(t.stride(), t.size()))
    expect = 1
    for st, sz in sizes_strides:
        if sz == 1:
            continue
        if st != expect:
            return None
        expect *= sz
    base = t.untyped_storage().data_ptr()
    return base, (t.data_ptr() - base) // t.element_size(), n


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

    def _merged_ranges(self, split_key=None, bridge_padding=True):
        """[[param base, grad base, first elem, end elem, [params], group index]]: one entry per launch.  Parameters whose
        split_key differs (Adam: their step counts) never share a range; bridge_padding=False when the update would not keep
        zeros zero (Adam with eps = 0: 0/0)."""
        name = type(self).__name__
        entries = []  # (param base, grad base, first elem, numel, group index, param)
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not (p.is_cuda and p.dtype == torch.float32):
                    raise RuntimeError(f"{name}: parameters must be CUDA fp32 tensors (no CPU fallback on the hot path)")
                rp, rg = _dense_range(p.data), _dense_range(p.grad)
                if rp is None or rg is None or rp[1:] != rg[1:]:
                    raise RuntimeError(f"{name}: parameter and gradient must be dense and share their flat offset")
                entries.append((rp[0], rg[0], rp[1], rp[2], gi, p))
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
                r = _dense_range(q.data)
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

    @staticmethod
    def _flat_views(ps, b, e):
        """the (parameter, gradient) slices [b, e) of the flat arrays the parameters ps live in"""
        dev = ps[0].device
        fp = torch.empty(0, dtype=torch.float32, device=dev).set_(ps[0].data.untyped_storage(), b, (e - b,))
        fg = torch.empty(0, dtype=torch.float32, device=dev).set_(ps[0].grad.untyped_storage(), b, (e - b,))
        return fp, fg

    def _state_view(self, flat, p, b, key):
        """state[p][key] := the view of the flat state array `flat` (starting at element b) that covers p; a tensor already there
        (loaded from a checkpoint, train.py:144, or kept across a re-plan) is carried over into it"""
        r = _dense_range(p.data)
        view = torch.as_strided(flat, p.shape, p.stride(), r[1] - b)
        old = self.state[p].get(key)
        if old is not None:
            view.copy_(old.to(device=flat.device, dtype=torch.float32))
        self.state[p][key] = view

    def _ema_slice(self, pb, b, e):
        if self._ema is not None:
            r = _dense_range(self._ema[0])
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
            fp, fg = self._flat_views(ps, b, e)
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
            fp, fg = self._flat_views(ps, b, e)
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
            fp, fg = self._flat_views(ps, b, e)
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
            fp, fg = self._flat_views(ps, b, e)
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
