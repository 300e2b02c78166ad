"""What the bit tests of the row kernels (csrc/weight_norm.hip, csrc/weight_std.hip) share with tests/golden/make_row_kernels_golden.py, which
describes the table and the arrays of tests/golden/row_kernels_bits.npz: the table, the inputs and the calls whose outputs the file holds."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "row_kernels_bits.npz")
SENTINEL = 0x7FC0DEAD
# (residue of the first element mod 4, rows, row_len)
SHAPES = [(1, 1, 1), (2, 1, 2), (1, 1, 3), (0, 1, 4), (3, 1, 5), (2, 1, 7), (1, 1, 63), (0, 1, 64), (3, 1, 65), (2, 1, 147), (3, 1, 257), (0, 1, 576),
          (2, 1, 1023), (1, 1, 1024), (3, 1, 1025), (0, 1, 1152), (1, 6, 147), (2, 3, 36)]
CONST_RECORD, CONST_ROW, CONST = len(SHAPES) - 1, 1, 0.25
MEANS = [0.0, 0.05, -3.0, 1e3, 0.01, -0.2, 1.0]
SDS = [1.0, 0.02, 1e-3, 1.0, 0.05, 0.3, 2.0]
BWD_SLICE = (2, 23)
MODES, BETAS = (1, 2), (0.0, 0.5)


def layout():
    recs, off = [], 8
    for res, rows, L in SHAPES:
        off += (res - off) % 4
        recs.append((off, rows, L))
        off += rows * L + 8
    return recs, off


def rows_of(recs):
    return [(int(o + r * L), int(L)) for o, rows, L in recs for r in range(rows)]


def sentinels(n):
    return np.full(n, SENTINEL, dtype=np.int32).view(np.float32).copy()


def inputs():
    recs, n = layout()
    rng = np.random.default_rng(8037)
    w, g, old = sentinels(n), sentinels(n), sentinels(n)
    for k, (o, L) in enumerate(rows_of(recs)):
        w[o: o + L] = (MEANS[k % 7] + SDS[k % 7] * rng.standard_normal(L)).astype(np.float32)
        g[o: o + L] = ((0.3 if k % 2 else -0.01) + 10.0 ** (-(k % 4)) * rng.standard_normal(L)).astype(np.float32)
        old[o: o + L] = (1.0 + rng.standard_normal(L)).astype(np.float32)
    o, rows, L = recs[CONST_RECORD]
    w[o + CONST_ROW * L: o + (CONST_ROW + 1) * L] = CONST
    return recs, w, g, old


def run_weight_norm(recs, w, dev="cuda"):
    """the weight_norm call of the fixture on the arrays given: {name: numpy array}"""
    from sota_imagenet_amd import item_plan, ops

    items = [(int(o), int(L), int(rows)) for o, rows, L in recs]
    flat = torch.from_numpy(w).to(dev)
    status = ops.weight_norm_rows_(flat, items, item_plan.pack_records(items, dev))
    return {"wnorm/out": flat.cpu().numpy(), "wnorm/status": status.cpu().numpy()}


def run_weight_std(recs, w, g, old, dev="cuda"):
    """the weight_std calls of the fixture, the in-place forward included: {name: numpy array}"""
    from sota_imagenet_amd import item_plan, ops

    out = {}
    rows = rows_of(recs)
    tab = item_plan.pack_records(rows, dev)
    for mode in MODES:
        src = torch.from_numpy(w).to(dev)
        w_hat = torch.from_numpy(sentinels(w.size)).to(dev)
        invstd = torch.full((len(rows),), float("nan"), device=dev)
        ops.weight_std_rows_fwd(src, w_hat, invstd, tab, mode)
        baked = torch.from_numpy(w).to(dev)
        inv2 = torch.full((len(rows),), float("nan"), device=dev)
        ops.weight_std_rows_fwd(baked, baked, inv2, tab, mode)
        out[f"fwd/{mode}/w_hat"], out[f"fwd/{mode}/invstd"] = w_hat.cpu().numpy(), invstd.cpu().numpy()
        out[f"fwd/{mode}/in_place"], out[f"fwd/{mode}/in_place_invstd"] = baked.cpu().numpy(), inv2.cpu().numpy()
        for beta in BETAS:
            dw = torch.from_numpy(old).to(dev) if beta else torch.full((w.size,), float("nan"), device=dev)
            ops.weight_std_rows_bwd(torch.from_numpy(g).to(dev), w_hat, invstd, dw, tab, mode, beta=beta, row_begin=BWD_SLICE[0], row_end=BWD_SLICE[1])
            out[f"bwd/{mode}/{beta}/dw"] = dw.cpu().numpy()
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def row_mask(n, rows):
    m = np.zeros(n, dtype=bool)
    for o, L in rows:
        m[o: o + L] = True
    return m
