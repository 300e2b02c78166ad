"""The host side of the work-item plan, written once: what the layer-wise optimizers (optim._Layerwise) and the sharpness-aware callbacks
(callbacks.SAMOriginal, callbacks.SAM) run on.  Which parameters fit the flat kernels (place), the parameters grouped by pair of parameter /
gradient storage with every tensor cut into work items of at most W elements (plan_items, storage_pairs), the 16-byte records the kernels read
(pack_records) and a storage as a flat array (storage_array; flat_views for a parameter and its gradient); for the statistics taken per output unit (callbacks.SAM, the unit-wise optimizers of
optim.py) the unit rule (unit_len) and the tables of pieces, slots and tensor records (plan_units); for the callbacks that run on a flat model's own
table the matrices of OrthoInitClb (ortho_records), the rows of WeightNorm with their work items (wnorm_records, wnorm_items) and the matrices,
tiles and rows of the two loss penalties (ortho_loss_mats, ortho_loss_cut; norm_loss_rows, norm_loss_items); for the two
histogram callbacks what to read of a tensor (hist_records) and the launches, one per storage (dist_plan).  Everything up to pack_records is pure Python on plain tuples, so a planner is pinned
without a GPU (tests/test_item_plan_host.py); the device side of the records is csrc/optim_items.h.  The merged-range planner of SGD / Adam /
MADGRAD / AdaiS (optim._merged_ranges) takes place and flat_views only."""
import numpy as np
import torch

ITEM_FIELDS = ("<i8", "<i4", "<i4")    # work items, SAM's pieces { first element, length, tensor or slot } and tensor records { start, unit_len, slot0 }
TENSOR_FIELDS = ("<i4", "<i4", "<f8")  # the tensor records of lw_coef { first item, item count, numel }
ORTHO_FIELDS = ("<i8", "<i4", "<i4", "<i4", "<i4")  # the matrices of ortho_init_ { first element, rows, chans, taps, pad }: 24 bytes
SPECTRAL_FIELDS = ("<i8", "<i4", "<i4", "<i8", "<i8")  # the matrices of ops.spectral_fwd { first element, row_len, rows, u0, v0 }: 32 bytes
ORTHO_LOSS_FIELDS = SPECTRAL_FIELDS  # the matrices of ops.ortho_loss_fwd { first element, row_len, rows, g0, t0 }: 32 bytes
OL_TILE_FIELDS = ("<i4", "<i4", "<i4", "<i4")  # its tiles { mat, ti | tj << 16, item0, n_slabs } and gradient items { mat, ti, tc, 0 }: 16 bytes
OL_ITEM_FIELDS = ("<i4", "<i4")  # its Gram items { tile, slab }: 8 bytes


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


def unit_len(shape, stride, unitwise, name):
    """elements per slot of a dense tensor: numel, or numel / shape[0] for a unit-wise tensor with ndim > 1 — whose dim 0 must be the
    outermost stride, so that a unit is one contiguous run; anything else raises RuntimeError in the name of class `name`"""
    n = int(np.prod(shape)) if len(shape) else 1
    if not unitwise or len(shape) <= 1:
        return n
    u = n // shape[0]
    if shape[0] > 1 and stride[0] != u:
        raise RuntimeError(f"{name}: unitwise needs dim 0 as the outermost stride (shape {tuple(shape)}, strides {tuple(stride)}): a unit must be "
                           "one contiguous run of numel / shape[0] elements")
    return u


def plan_units(tensors, W):
    """the tables of a plan with one statistic per slot.  tensors: [(param base, grad base, first elem, numel, unit_len)] in param-group order,
    unit_len = numel for a whole-tensor slot, less for a tensor taken unit by unit; W: ops.lw_item_elems().  Returns a dict:
      items    storage_pairs' work items of ALL tensors
      tensors  [(start relative to its pair's range, unit_len, slot0)] per tensor; slots are numbered tensor by tensor
      pieces   [(first element relative to the pair's range, length <= W, slot)]: every unit of the unit-wise tensors, cut at multiples of
               W from the unit's start
      whole    the work items of the whole-tensor slots, in the order of `items`
      slots    [(first, count)] per slot: its consecutive entries of the partial sums, which are laid out pair by pair, a pair's pieces
               before its whole-tensor items
      pairs    [(lo, hi, first item, end item, (first piece, end piece), (first whole item, end), first partial entry, tensor indices)]"""
    items, _, pairs0 = storage_pairs(tensors, W)
    slot0, n_slots = [], 0
    for _, _, _, n, u in tensors:
        if u < 1 or n % u or n >= 1 << 31:
            raise ValueError(f"numel={n}, unit_len={u}: a tensor is a whole number of units and shorter than 2^31 elements")
        slot0.append(n_slots)
        n_slots += n // u
    trec, pieces, whole, slots, pairs = [None] * len(tensors), [], [], [None] * n_slots, []
    k = 0  # entries of the partial sums so far
    for lo, hi, i0, i1, ts in pairs0:
        pa, wa, k0 = len(pieces), len(whole), k
        for t in ts:
            _, _, off, n, u = tensors[t]
            trec[t] = (off - lo, u, slot0[t])
            if u == n:
                continue
            per = (u + W - 1) // W
            for j in range(n // u):
                slots[slot0[t] + j] = (k, per)
                pieces.extend((off - lo + j * u + c, min(W, u - c), slot0[t] + j) for c in range(0, u, W))
                k += per
        for o, ln, t in items[i0:i1]:
            if tensors[t][4] != tensors[t][3]:
                continue
            first, count = slots[slot0[t]] or (k, 0)
            slots[slot0[t]] = (first, count + 1)
            whole.append((o, ln, t))
            k += 1
        pairs.append((lo, hi, i0, i1, (pa, len(pieces)), (wa, len(whole)), k0, ts))
    return dict(items=items, tensors=trec, pieces=pieces, whole=whole, slots=slots, pairs=pairs)


def ortho_records(table):
    """the matrices the OrthoInitClb callback orthogonalises.  table: a flat model's [(name, kind, offset, shape)]; returns [(off, rows, chans,
    taps)] for every parameter (kind 0) with 4 or 2 dimensions, in table order: a conv weight [O, I, kh, kw] (KRSC memory) gives (off, O, I, kh*kw),
    an FC weight [O, I] gives (off, O, I, 1) — without the padding rows behind it.  BatchNorm tensors, biases, 3-D (Conv1d) weights and buffers
    are not selected (sota_imagenet/callbacks.py:260-261 walks nn.Conv2d / nn.Linear)"""
    out = []
    for _, kind, off, shape in table:
        if kind == 0 and len(shape) == 4:
            out.append((off, shape[0], shape[1], shape[2] * shape[3]))
        elif kind == 0 and len(shape) == 2:
            out.append((off, shape[0], shape[1], 1))
    return out


def wnorm_records(table):
    """the rows the WeightNorm callback normalises.  table: a flat model's [(name, kind, offset, shape)]; returns [(off, rows, row_len)] for every
    parameter (kind 0) with two or more dimensions and 64 elements or more, in table order: rows = shape[0], row_len = numel / rows — a conv
    weight [O, I, kh, kw] is KRSC in memory, a row is still one contiguous run of I*kh*kw elements; an FC weight [O, I] gives (off, O, I), without
    the padding rows behind it.  BatchNorm tensors and biases (one dimension: the reference's view(C, -1) of them has rows of ONE element, whose
    norm after centring is 0), buffers and the ECA Conv1d weights (numel < 64, sota_imagenet/callbacks.py:118) are not selected."""
    out = []
    for _, kind, off, shape in table:
        n = int(np.prod(shape)) if len(shape) else 1
        if kind == 0 and len(shape) >= 2 and n >= 64:
            out.append((off, shape[0], n // shape[0]))
    return out


def ws_rows(table):
    """the rows of the forward weight transform (ops.weight_std_rows_fwd): [(first element, row_len)], one per output filter of every conv
    weight — a parameter (kind 0) with four dimensions — of a flat model's [(name, kind, offset, shape)], in table order.  An FC weight is not
    a conv: the transform leaves it alone.  A conv weight [O, I, kh, kw] is KRSC in memory, a filter is one contiguous run of I*kh*kw elements."""
    rows = []
    for _, kind, off, shape in table:
        if kind == 0 and len(shape) == 4:
            L = int(np.prod(shape[1:]))
            rows.extend((off + r * L, L) for r in range(shape[0]))
    return rows


def spectral_mats(table):
    """the matrices of the forward spectral normalisation (ops.spectral_fwd / spectral_bwd): ([(first element, row_len, rows, u0, v0)], n_u, n_v),
    one record per conv weight — a parameter (kind 0) with four dimensions — of a flat model's [(name, kind, offset, shape)], in the order of
    their offsets in the flat array, which is the order the executor lays out its own table in: u0 is the running sum of the rows (one
    element of u per filter), v0 the running sum of the row lengths (one element of v per filter element, in memory order (K,K,Cin)); n_u and
    n_v are the sizes of u and v.  An FC weight is not a conv.  Pack with pack_records(records, device, SPECTRAL_FIELDS)."""
    mats, u0, v0 = [], 0, 0
    for _, kind, off, shape in sorted(table, key=lambda t: t[2]):
        if kind == 0 and len(shape) == 4:
            L = int(np.prod(shape[1:]))
            mats.append((off, L, shape[0], u0, v0))
            u0, v0 = u0 + shape[0], v0 + L
    return mats, u0, v0


def ortho_loss_mats(table, min_filters):
    """the matrices of the orthogonality penalty (losses.OrthoLoss; sota_imagenet/callbacks.py:138-146): ([(first element, row_len, rows, g0)],
    n_gram) for every conv weight — a parameter (kind 0) with four dimensions — of a flat model's [(name, kind, offset, shape)] whose rows = O
    and row_len = I*kh*kw have rows <= row_len and rows >= min_filters, in the order of their offsets; g0 is the running sum of rows^2 (the
    place of its Gram matrix), n_gram the total.  A filter is one contiguous run of row_len elements (KRSC memory), and W W^T does not depend on
    the order of the columns."""
    mats, g0 = [], 0
    for _, kind, off, shape in sorted(table, key=lambda t: t[2]):
        if kind == 0 and len(shape) == 4:
            O, L = shape[0], int(np.prod(shape[1:]))
            if O <= L and O >= min_filters:
                mats.append((off, L, O, g0))
                g0 += O * O
    return mats, g0


def ortho_loss_cut(mats, tile, kslab):
    """the work items of ops.ortho_loss_fwd / ortho_loss_bwd, a function of the records [(off, row_len, rows, g0)] and the two sizes alone.
    Returns a dict of tables in the kernels' field order:
      mats    [(off, row_len, rows, g0, t0)]: t0 the matrix's first tile (ORTHO_LOSS_FIELDS)
      tiles   [(mat, ti | tj << 16, item0, n_slabs)]: per matrix the tiles of `tile` rows x `tile` rows on or below the diagonal, ti ascending and
              tj <= ti ascending inside — tile (ti, tj) of a matrix sits at t0 + ti (ti + 1) / 2 + tj —, each with its n_slabs = ceil(row_len /
              kslab) consecutive items (OL_TILE_FIELDS)
      items   [(tile, slab)]: the Gram pass, item tiles[t].item0 + j = (t, j) (OL_ITEM_FIELDS)
      gitems  [(mat, ti, tc, 0)]: the gradient pass, every row tile with every tile of `tile` columns of row_len (OL_TILE_FIELDS)
    A record with rows > row_len has no Gram matrix to ask for and raises ValueError: it must never reach a kernel."""
    out = dict(mats=[], tiles=[], items=[], gitems=[])
    for m, (off, L, R, g0) in enumerate(mats):
        if R < 1 or L < 1 or R > L:
            raise ValueError(f"matrix at offset {off}: rows={R}, row_len={L} — 1 <= rows <= row_len is needed")
        nt, n_slabs = -(-R // tile), -(-L // kslab)
        if nt >= 1 << 15:
            raise ValueError(f"matrix at offset {off}: {nt} row tiles do not fit the tile record")
        out["mats"].append((off, L, R, g0, len(out["tiles"])))
        for ti in range(nt):
            for tj in range(ti + 1):
                t = len(out["tiles"])
                out["tiles"].append((m, ti | tj << 16, len(out["items"]), n_slabs))
                out["items"].extend((t, j) for j in range(n_slabs))
            out["gitems"].extend((m, ti, tc, 0) for tc in range(-(-L // tile)))
    return out


def norm_loss_rows(table):
    """the rows of the norm penalty (losses.NormLoss; sota_imagenet/callbacks.py:213-217 walks every module with a .weight of 64 elements or
    more): [(off, rows, row_len)] for every parameter (kind 0) of a flat model's [(name, kind, offset, shape)] whose name ends in ".weight" and
    that has 64 elements or more, in table order; rows = shape[0], row_len = numel / rows.  Unlike wnorm_records the BatchNorm weights are in
    (rows of ONE element: n_r = |gamma_r|) and so is the FC weight, without its padding rows; biases and buffers are not."""
    out = []
    for name, kind, off, shape in table:
        n = int(np.prod(shape)) if len(shape) else 1
        if kind == 0 and name.endswith(".weight") and n >= 64:
            out.append((off, shape[0], n // shape[0]))
    return out


def norm_loss_items(records, W):
    """the tables of ops.norm_loss_fwd / norm_loss_bwd from norm_loss_rows' records: (items, tensors) — items = wnorm_items(records, W), runs of
    whole rows of one tensor; tensors = [(first item, item count, rows)] per record (ITEM_FIELDS)"""
    items, tensors = [], []
    for rec in records:
        mine = wnorm_items([rec], W)
        tensors.append((len(items), len(mine), rec[1]))
        items.extend(mine)
    return items, tensors


def wnorm_items(records, W):
    """the work items of ops.weight_norm_rows_.  records: [(off, rows, row_len)]; returns [(first element, row_len, n_rows)]: every record's rows
    cut, from its first row, into runs of max(1, W // row_len) rows — whole rows only, a row longer than W is an item of its own; the cuts depend
    on (rows, row_len, W) alone, the items of one record are consecutive and cover exactly its rows"""
    items = []
    for off, rows, row_len in records:
        if rows < 1 or row_len < 1:
            raise ValueError(f"record at offset {off}: rows={rows}, row_len={row_len} must be >= 1")
        per = max(1, W // row_len)
        items.extend((off + r * row_len, row_len, min(per, rows - r)) for r in range(0, rows, per))
    return items


def hist_records(t):
    """what the histogram of callbacks.GradDistributionTB counts of the CUDA fp32 tensor view `t`: (storage base ptr, first element, source
    elements, rep) — the elements to read and how many shown elements each stands for.  A dense view (dense_range) is read as it is, rep 1; a view
    with stride 0 on every dimension (exp_avg_sq of the layer-wise optimizers) is ONE element shown numel times; the unit form of
    optim._unit_strides (stride 1 on dim 0, 0 on the others) is shape[0] elements shown numel / shape[0] times each.  Dimensions of size 1 carry
    no stride.  Anything else raises RuntimeError naming the shape and strides."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
        raise NotImplementedError(f"hist_records: a CUDA fp32 tensor is needed (there is no CPU path), got {getattr(t, 'dtype', type(t).__name__)} "
                                  f"on {getattr(t, 'device', 'the host')}")
    n = t.numel()
    if n < 1:
        raise RuntimeError(f"hist_records: an empty tensor (shape {tuple(t.shape)}) has nothing to count")
    base = t.untyped_storage().data_ptr()
    first = (t.data_ptr() - base) // t.element_size()
    r = dense_range(t)
    if r is not None:
        return base, first, n, 1
    strides = [st if sz > 1 else 0 for st, sz in zip(t.stride(), t.size())]
    if not any(strides):
        return base, first, 1, n
    if strides[0] == 1 and not any(strides[1:]):
        return base, first, t.shape[0], n // t.shape[0]
    raise RuntimeError(f"hist_records: shape {tuple(t.shape)} with strides {tuple(t.stride())} is neither dense, nor one value shown broadcast, "
                       "nor one value per index of dim 0")


def dist_plan(records, W):
    """the launches of the two histogram callbacks.  records: (storage base ptr, first element, elements to read) for a tensor the counting kernel
    reads, None for one it does not — callbacks.WeightDistributionTB: per entry of a state_dict, in its order; callbacks.GradDistributionTB: per
    tensor of one tag (hist_records' source elements), none of them None.  The tensors are numbered in that order (their rows of the histogram table)
    and grouped by storage, one launch per storage in order of first appearance.  Returns (rows, launches, spans, n_items): rows[r] = the entry of
    row r; launches = [(base, lo, hi, items, first item)], [lo, hi) the element range of the storage that the launch's flat array covers (lo a
    multiple of 4 elements), items = plan_items' table with offsets relative to lo and the row as tensor index, first item = the launch's place
    in an array of per-item results shared by all launches (n_items entries); spans[r] = (first item, item count) of row r there."""
    rows = [k for k, r in enumerate(records) if r is not None]
    by_storage = {}
    for r, k in enumerate(rows):
        by_storage.setdefault(records[k][0], []).append(r)
    launches, spans, n_items = [], [None] * len(rows), 0
    for base, rs in by_storage.items():
        recs = [records[rows[r]] for r in rs]
        lo = min(first for _, first, _ in recs) & ~3
        hi = max(first + n for _, first, n in recs)
        items, sp = plan_items([(first - lo, n) for _, first, n in recs], W, rs)
        for r, (i0, c) in zip(rs, sp):
            spans[r] = (n_items + i0, c)
        launches.append((base, lo, hi, items, n_items))
        n_items += len(items)
    return rows, launches, spans, n_items


def pack_records(records, device=None, fields=ITEM_FIELDS):
    """records (tuples of `fields`, 16 bytes for the default three) as the [n, bytes / 8] int64 tensor the ops wrappers take, on `device` (the
    CPU if None); a record shorter than `fields` is padded with zeros"""
    records = [tuple(r) + (0,) * (len(fields) - len(r)) for r in records]
    rec = np.array(records, dtype=[(f"f{i}", f) for i, f in enumerate(fields)])
    t = torch.from_numpy(rec.view(np.int64).reshape(-1, rec.dtype.itemsize // 8))
    return t if device is None else t.to(device)


def storage_array(t, lo, hi):
    """the storage of the tensor t, in t's dtype and on its device, as a flat array over the elements [lo, hi)"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), lo, (hi - lo,))


def flat_views(p, lo, hi):
    """the storages of the parameter p and of its gradient (fp32 under the placement rule) as flat arrays over the elements [lo, hi)"""
    return storage_array(p.data, lo, hi), storage_array(p.grad, lo, hi)
