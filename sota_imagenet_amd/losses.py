"""`CrossEntropyLoss` plugin: label-smoothed softmax cross entropy on float targets, one native HIP kernel.

Drop-in for `_target_: pytorch_tools.losses.smooth.CrossEntropyLoss` (sota_imagenet/arg_parser.py:140-142;
`smoothing: 0.1` in configs/hydra_exp/1.r50_baseline.yaml:34-35; built at train.py:81; call form
`criterion(output, target)` sota_imagenet/callbacks.py:316).  Targets are the loader's one-hot float rows
(dali_dataloader.py:123) or the soft rows CutMix/Mixup produce (callbacks.py:244-247); 1-D class indices are
accepted too.  Forward and the gradient wrt the logits come out of the same kernel launch.

`Loss` is the small base the reference's callbacks lean on (pt.losses.Loss: `state.criterion += OrthoLoss(model) * weight`,
sota_imagenet/callbacks.py:200, :229): `+` builds a sum of terms, `*` a weighted term, and every term is called with the same
`(y_pred, y_true)`.  `OrthoLoss` and `NormLoss` are the two parameter-only terms (callbacks.py:126-156, :206-221) on the kernels of
csrc/ortho_loss.hip; DESIGN.md section 22.
"""
import torch
import torch.nn as nn

from . import item_plan, ops


class Loss(nn.Module):
    """a criterion term: a + b -> SumOfLosses, a * w and w * a -> WeightedLoss (the two operators of pt.losses.Loss the reference uses)"""

    def __add__(self, other):
        if not isinstance(other, Loss):
            raise ValueError("Loss should be inherited from `Loss` class")
        return SumOfLosses(self, other)

    def __mul__(self, value):
        if not isinstance(value, (int, float)):
            raise ValueError("Loss should be multiplied by int or float")
        return WeightedLoss(self, value)

    def __rmul__(self, other):
        return self.__mul__(other)


class WeightedLoss(Loss):
    def __init__(self, loss, weight=1.0):
        super().__init__()
        self.loss = loss
        self.weight = float(weight)

    def forward(self, *inputs):
        return self.loss(*inputs) * self.weight


class SumOfLosses(Loss):
    def __init__(self, l1, l2):
        super().__init__()
        self.l1 = l1
        self.l2 = l2

    def forward(self, *inputs):
        return self.l1(*inputs) + self.l2(*inputs)


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, smoothing):
        loss, dlogits = ops.ce_loss(logits, target, smoothing, 1.0, need_grad=True)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None


class CrossEntropyLoss(Loss):
    def __init__(self, mode="multiclass", smoothing=0.0, reduction="mean", from_logits=True, temperature=1.0, **unsupported):
        super().__init__()
        if mode != "multiclass" or reduction != "mean" or not from_logits or temperature != 1.0:
            raise NotImplementedError("only mode='multiclass', reduction='mean', from_logits=True, temperature=1 is on the hot path")
        for k, v in unsupported.items():
            if v not in (None, False, 0, 0.0):
                raise NotImplementedError(f"CrossEntropyLoss({k}={v!r}) unsupported")
        self.smoothing = float(smoothing)

    def forward(self, y_pred, y_true):
        if not y_pred.is_cuda:
            raise RuntimeError("CrossEntropyLoss: the MI355X hot path has no CPU fallback")
        y_pred = y_pred.float().contiguous()
        if y_true.dim() == 1:
            y_true = torch.nn.functional.one_hot(y_true.long(), y_pred.shape[1])
        y_true = y_true.to(torch.float32).contiguous()
        if torch.is_grad_enabled() and y_pred.requires_grad:
            return _CEFn.apply(y_pred, y_true, self.smoothing)
        loss, _ = ops.ce_loss(y_pred, y_true, self.smoothing, 1.0, need_grad=False)
        return loss


class _PenaltyFn(torch.autograd.Function):
    """the autograd node of a parameter-only term.  It takes the logits as an input and returns no gradient for them: autograd then runs this
    node before the executor's node, whatever order the terms were summed in.  backward clears the flat gradients if they are clean, adds the
    term's gradient and marks them dirty, so that the executor's backward — which OVERWRITES clean gradients — accumulates on top.
    The gradient pass reads what the term's LAST forward left in its scratch (G, the coefficients): a node whose forward is no longer the last
    one — two forwards of one term before a backward — raises RuntimeError instead of using another forward's statistics."""

    @staticmethod
    def forward(ctx, y_pred, hook, term):
        ctx.term = term
        out = term._launch_forward().clone()
        term._forwards += 1
        ctx.stamp = term._forwards
        return out

    @staticmethod
    def backward(ctx, g):
        term = ctx.term
        if ctx.stamp != term._forwards:
            raise RuntimeError(f"{type(term).__name__}: backward of forward {ctx.stamp}, but the scratch holds forward {term._forwards}: one "
                               "backward per forward, before the next forward of the same term")
        m = term.model
        m._attach_grads()
        if not m._grads_dirty:
            m.flat_grads.zero_()
        term._launch_backward(g.detach().to(torch.float32).reshape(1).contiguous())
        m._grads_dirty = True
        return None, None, None


class _FlatPenalty(Loss):
    """what OrthoLoss and NormLoss share: a flat model (models._FlatModel) on a CUDA device — anything else raises NotImplementedError —, the
    plan built lazily from the model's table and rebuilt when flat_params.data_ptr() changes (a device move), and forward(*args): a 0-dim fp32
    device tensor, with gradients enabled behind an autograd node whose backward launches the gradient pass into model.flat_grads.  The term
    always reads model.flat_params — the raw weights, whatever forward transform is switched on — and nothing is read back to the host."""

    def __init__(self, model):
        super().__init__()
        from .models import _FlatModel

        m = model.module if hasattr(model, "module") else model
        if not isinstance(m, _FlatModel):
            raise NotImplementedError(f"{type(self).__name__} runs on the flat parameter array of a native model (models._FlatModel), got "
                                      f"{type(m).__name__}")
        if not m.flat_params.is_cuda:
            raise NotImplementedError(f"{type(self).__name__}: the model must be on a CUDA device (there is no CPU path)")
        self.__dict__["model"] = m  # not a submodule: moving or saving the criterion must not touch the model
        self._plan_ptr = None
        self._hook = None
        self._forwards = 0  # forwards so far: stamps the autograd node, whose backward reads this forward's scratch

    def _plan(self):
        m = self.model
        if not m.flat_params.is_cuda:
            raise NotImplementedError(f"{type(self).__name__}: the model must be on a CUDA device (there is no CPU path)")
        if self._plan_ptr != m.flat_params.data_ptr():
            self._build(m)
            self._hook = torch.zeros(1, device=m.flat_params.device, requires_grad=True)  # an edge for autograd when the logits carry none
            self._plan_ptr = m.flat_params.data_ptr()

    def forward(self, *args):
        self._plan()
        if not torch.is_grad_enabled():
            self._forwards += 1  # the scratch no longer holds an earlier node's statistics
            return self._launch_forward().clone()
        y_pred = args[0] if args and torch.is_tensor(args[0]) else self._hook
        return _PenaltyFn.apply(y_pred, self._hook, self)


class OrthoLoss(_FlatPenalty):
    """sota_imagenet/callbacks.py:126-156, type 1: for every conv weight viewed as W [O, K] with O <= K and O >= min_filters, G = W W^T - I and
    F = |G|_F; where F / O > min_norm the loss takes F, and the gradient (2 / F) G W.  Three launches forward, one backward, over all
    matrices (ops.ortho_loss_fwd / ortho_loss_bwd; item_plan.ortho_loss_mats, ortho_loss_cut).  eps is unused, as in the reference's type 1.
    debug=True prints one line per matrix, as the reference does, from ONE copy of the statistics to the host.

    Deviations from the reference, deliberate:
      * its Runner evaluates the criterion under autocast when fp16 is on, so its Gram product runs in half precision; here the products are
        always fp32 (the exact fp32 MFMA) on the fp32 master weights, the sums of squares double;
      * the gate F / O > min_norm is decided on the device from the fp32 F, without a host synchronisation per matrix."""

    def __init__(self, model, eps=1e-2, min_filters=384, min_norm=1, debug=False):
        super().__init__(model)
        self.eps, self.min_filters, self.min_norm, self.debug = eps, int(min_filters), float(min_norm), bool(debug)
        self.mats, self.names = [], []

    def _build(self, m):
        dev = m.flat_params.device
        self.mats, n_gram = item_plan.ortho_loss_mats(m._table, self.min_filters)
        if not self.mats:
            raise NotImplementedError(f"OrthoLoss(min_filters={self.min_filters}): the rule selects no convolution of {type(m).__name__}")
        by_off = {off: name for name, kind, off, shape in m._table if kind == 0}
        self.names = [by_off[r[0]] for r in self.mats]
        cut = item_plan.ortho_loss_cut(self.mats, ops.OL_TILE, ops.OL_KSLAB)
        fields = dict(mats=item_plan.ORTHO_LOSS_FIELDS, tiles=item_plan.OL_TILE_FIELDS, items=item_plan.OL_ITEM_FIELDS, gitems=item_plan.OL_TILE_FIELDS)
        self._tables = {k: item_plan.pack_records(cut[k], dev, fields[k]) for k in fields}
        self._scratch = ops.ortho_loss_scratch(n_gram, len(cut["mats"]), len(cut["tiles"]), len(cut["items"]), dev)

    def _launch_forward(self):
        loss = ops.ortho_loss_fwd(self.model.flat_params.detach(), self._tables, self._scratch, self.min_norm)
        if self.debug:
            stats = self._scratch["stats"].cpu()  # ONE copy
            for name, (_, L, R, _), row in zip(self.names, self.mats, stats.tolist()):
                print(f"{name:40s}: ({R}, {L}) {row[0]:.3f}")
        return loss

    def _launch_backward(self, s):
        m = self.model
        ops.ortho_loss_bwd(m.flat_params.detach(), m.flat_grads, self._tables, self._scratch, s, accumulate=True)


class NormLoss(_FlatPenalty):
    """sota_imagenet/callbacks.py:206-221: for every parameter named *.weight with 64 elements or more, viewed as [shape[0], -1], the mean over
    its rows of (1 - |row|_2)^2 — BatchNorm weights (rows of one element) and the FC weight included, biases not.  Two launches forward, one
    backward (ops.norm_loss_fwd / norm_loss_bwd; item_plan.norm_loss_rows, norm_loss_items).  The reference prints a line per module at every
    call; this does not."""

    def _build(self, m):
        dev = m.flat_params.device
        self.records = item_plan.norm_loss_rows(m._table)
        if not self.records:
            raise NotImplementedError(f"NormLoss: {type(m).__name__} has no .weight of 64 elements or more")
        items, tensors = item_plan.norm_loss_items(self.records, ops.NL_ITEM_ELEMS)
        self._items_dev, self._tensors_dev = item_plan.pack_records(items, dev), item_plan.pack_records(tensors, dev)
        self._scratch = ops.norm_loss_scratch(len(items), len(tensors), dev)

    def _launch_forward(self):
        return ops.norm_loss_fwd(self.model.flat_params.detach(), self._items_dev, self._tensors_dev, self._scratch)

    def _launch_backward(self, s):
        m = self.model
        ops.norm_loss_bwd(m.flat_params.detach(), m.flat_grads, self._items_dev, self._tensors_dev, s, accumulate=True)
