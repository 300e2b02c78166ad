"""The host side of the work-item plan, written once: what the layer-wise optimizers (optim._Layerwise) and the sharpness-aware callbacks
(callbacks.SAMOriginal, callbacks.SAM) run on.  Which parameters fit the flat kernels (place), the parameters grouped by pair of parameter /
gradient storage with every tensor cut into work items of at most W elements (plan_items, storage_pairs), the 16-byte records the kernels read
(pack_records) and a storage as flat arrays (flat_views).  Everything up to pack_records is pure Python on plain tuples, so a planner is pinned
without a GPU (tests/test_item_plan_host.py); the device side of the records is csrc/optim_items.h.  The merged-range planner of SGD / Adam /
MADGRAD / AdaiS (optim._merged_ranges) takes place and flat_views only."""
import numpy as np
import torch

ITEM_FIELDS = ("<i8", "<i4", "<i4")    # work items, SAM's pieces { first element, length, tensor or slot } and tensor records { start, unit_len, slot0 }
TENSOR_FIELDS = ("<i4", "<i4", "<f8")  # the tensor records of lw_coef { first item, item count, numel }


def dense_range(t):
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


def place(params, name, aligned=False, one_device=False):
    """the placement rule.  params: parameters that all have a gradient; returns [(param base, grad base, first elem, numel, param)] in their
    order and raises RuntimeError (in the name of class `name`) for anything that is not CUDA fp32, not dense, or whose parameter and gradient
    sit at different flat offsets; aligned: every tensor starts on a 16-byte boundary of both storages; one_device: all on one device"""
    out = []
    for p in params:
        if not (p.is_cuda and p.dtype == torch.float32 and p.grad.is_cuda and p.grad.dtype == torch.float32):
            raise RuntimeError(f"{name}: parameters and gradients must be CUDA fp32 tensors (no CPU fallback on the hot path)")
        rp, rg = dense_range(p.data), dense_range(p.grad)
        if rp is None or rg is None or rp[1:] != rg[1:]:
            raise RuntimeError(f"{name}: parameter and gradient must be dense and share their flat offset")
        if aligned and ((rp[1] * 4) % 16 or p.data_ptr() % 16 or p.grad.data_ptr() % 16):
            raise RuntimeError(f"{name}: flat range not 16-byte aligned")
        out.append((rp[0], rg[0], rp[1], rp[2], p))
    if one_device and any(e[4].device != out[0][4].device for e in out):
        raise RuntimeError(f"{name}: all parameters must live on one device")
    return out


def plan_items(tensors, W, index=None):
    """the work-item table.  tensors: [(first element, numel)] in table order; returns (items, spans): items = [(first element, length, tensor
    index)], every tensor's own range cut at multiples of W from its start (the cuts depend on numel alone), the items of one tensor
    consecutive; spans = [(first item, item count)] per tensor, in table order.  The tensor index of an item is the tensor's position in
    `tensors`, or index[position] where the caller numbers its tensors otherwise.  Nothing outside a tensor's range — alignment gaps, the FC
    padding — is ever covered."""
    items, spans = [], []
    for t, (off, n) in zip(index or range(len(tensors)), tensors):
        if n < 1:
            raise ValueError(f"tensor {t}: numel={n} must be >= 1")
        spans.append((len(items), (n + W - 1) // W))
        items.extend((off + c, min(W, n - c), t) for c in range(0, n, W))
    return items, spans


def storage_pairs(tensors, W):
    """tensors: [(param base, grad base, first elem, numel, ...)] in param-group order; one launch set per pair of parameter / gradient
    storage.  Returns (items, spans, pairs): pairs = [(lo, hi, first item, end item, tensor indices)] in order of first appearance, [lo, hi)
    the element range of the storage its tensors span; items = plan_items' table pair by pair, inside a pair in the order given, the offsets
    relative to the pair's lo, the tensor index the index into `tensors`; spans[tensor] = (first item, item count)"""
    pairs = {}  # (param base, grad base) -> [lo, hi, tensor indices]
    for t, (pb, gb, off, n, *_) in enumerate(tensors):
        r = pairs.setdefault((pb, gb), [off, off + n, []])
        r[0], r[1] = min(r[0], off), max(r[1], off + n)
        r[2].append(t)
    order = [t for r in pairs.values() for t in r[2]]  # table order
    lo_of = {t: r[0] for r in pairs.values() for t in r[2]}
    items, in_order = plan_items([(tensors[t][2] - lo_of[t], tensors[t][3]) for t in order], W, order)
    spans = [span for _, span in sorted(zip(order, in_order))]  # by tensor index
    return items, spans, [(lo, hi, spans[ts[0]][0], sum(spans[ts[-1]]), ts) for lo, hi, ts in pairs.values()]


def pack_records(records, device=None, fields=ITEM_FIELDS):
    """16-byte records (tuples of three `fields`) as the [n, 2] int64 tensor the ops wrappers take, on `device` (the CPU if None)"""
    rec = np.array(records, dtype=[(f"f{i}", f) for i, f in enumerate(fields)])
    t = torch.from_numpy(rec.view(np.int64).reshape(-1, 2))
    return t if device is None else t.to(device)


def flat_views(p, lo, hi):
    """the storages of the parameter p and of its gradient as flat fp32 arrays over the elements [lo, hi)"""
    return tuple(torch.empty(0, dtype=torch.float32, device=p.device).set_(t.untyped_storage(), lo, (hi - lo,)) for t in (p.data, p.grad))
