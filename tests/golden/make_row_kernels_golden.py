#!/usr/bin/env python3
"""Records tests/golden/row_kernels_bits.npz: what the row kernels of csrc/weight_norm.hip and csrc/weight_std.hip give, bit for bit, on rows at
which their walk can go wrong.  Run by hand on an MI355X, with the library of the commit whose bits are to be kept, through the library's own
entry points (ops.weight_norm_rows_, ops.weight_std_rows_fwd, ops.weight_std_rows_bwd) and nothing else:

    python tests/golden/make_row_kernels_golden.py [output file]

The file was recorded at 8c37e32, the last commit whose kernels spell every pass out twice (a scalar and an f32x4 form); a later change of these
kernels that does not reproduce it has changed their arithmetic or the order of a sum.  It is never made again from the code it tests.

The table, [(first element, rows, row_len)]: one row each of 1, 2, 3, 4, 5, 7, 63, 64, 65, 147, 257, 576, 1023, 1024, 1025 and 1152 elements — rows
that end inside the scalar head (1 element, three in front of a 16-byte boundary), heads alone (2 and 3 elements), no f32x4 body, every tail
of 0..3 elements, one lane short of a wave's 64 vectors and one past, the stem's 147, both sides of mi355_wnorm_wave_row_max() (1025 and
1152 take weight_norm's whole-workgroup path) —, six consecutive rows of 147 (every alignment of a first element; as a weight_norm item, n_rows
is no multiple of 4) and three rows of 36 whose middle one is constant.  The first elements cover all four residues mod 4; in front, behind and
in every gap of 8..11 elements lies SENTINEL, a NaN: a gap that is read poisons what reads it, a gap that is written loses its bits.
weight_norm takes every record as one item (first, row_len, rows), sixteen of them with n_rows == 1; weight_std takes every row as a record of
its own (25 rows: seven workgroups, the last with three idle waves).

Arrays of the file (float32 arrays as they are; SENTINEL in the gaps unless said otherwise):
    records        int64 [n, 3]   the table;   bwd_slice  int64 [2]   [row_begin, row_end) of the backward calls, both inside a group of four
    w, g, dw_old   the inputs: the weights, the gradient wrt w_hat, what dw held before a backward with beta != 0
    wnorm/out, wnorm/status       weight_norm_rows_ on a copy of w.  The row of one element and the constant row are NaN (0 / 0)
    fwd/<mode>/w_hat, fwd/<mode>/invstd     weight_std_rows_fwd, mode in {1, 2}, into an array filled with SENTINEL.  The in-place call (w_hat is a
                   copy of w) gave the same array, gaps included, which is asserted here: one array stands for both
    bwd/<mode>/<beta>/dw          weight_std_rows_bwd over bwd_slice from g and the forward's w_hat and invstd of that mode; beta 0.5 on dw_old,
                   beta 0 on an array filled with the plain NaN 0x7FC00000, which is never read: the rows come out finite"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import row_bits_common as R  # noqa: E402
from row_bits_common import BETAS, BWD_SLICE, MODES, SENTINEL, inputs, rows_of, run_weight_norm, run_weight_std, same_bits  # noqa: E402


def main():
    recs, w, g, old = inputs()
    n = w.size
    heads = {min((4 - o % 4) % 4, L) for o, L in rows_of(recs)}
    tails = {(L - min((4 - o % 4) % 4, L)) % 4 for o, L in rows_of(recs)}
    assert {o % 4 for o, _, _ in recs} == {0, 1, 2, 3} and heads == {0, 1, 2, 3} and tails == {0, 1, 2, 3}
    assert BWD_SLICE[0] % 4 and (BWD_SLICE[1] - BWD_SLICE[0]) % 4 and BWD_SLICE[1] < len(rows_of(recs))
    out = {**run_weight_norm(recs, w), **run_weight_std(recs, w, g, old)}
    again = {**run_weight_norm(recs, w), **run_weight_std(recs, w, g, old)}
    assert all(same_bits(out[k], again[k]) for k in out), "two runs agree bit for bit"
    mask = R.row_mask(n, rows_of(recs))
    assert (out["wnorm/status"] == 0).all() and (out["wnorm/out"].view(np.int32)[~mask] == SENTINEL).all()
    for mode in MODES:
        assert same_bits(out.pop(f"fwd/{mode}/in_place"), out[f"fwd/{mode}/w_hat"]), "in place: the same array, gaps included"
        assert same_bits(out.pop(f"fwd/{mode}/in_place_invstd"), out[f"fwd/{mode}/invstd"])
        assert np.isfinite(out[f"fwd/{mode}/w_hat"][mask]).all() and np.isfinite(out[f"fwd/{mode}/invstd"]).all()
        sl = R.row_mask(n, rows_of(recs)[BWD_SLICE[0]: BWD_SLICE[1]])
        for beta in BETAS:
            dw = out[f"bwd/{mode}/{beta}/dw"]
            assert np.isfinite(dw[sl]).all(), "beta 0: the NaN in dw is never read"
            assert same_bits(dw[~sl], old[~sl] if beta else np.full((~sl).sum(), np.nan, dtype=np.float32))
    arrays = dict(records=np.array(recs, dtype=np.int64), bwd_slice=np.array(BWD_SLICE, dtype=np.int64), w=w, g=g, dw_old=old, **out)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "row_kernels_bits.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 300_000, size
    print(f"wrote {path}: {size} bytes, {n} elements per array, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
