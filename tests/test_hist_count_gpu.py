"""The workgroup histogram of csrc/hist_count.h on the MI355X, through both kernels that call it (ops.absbin_hist, ops.tbbin_hist): where the
wave-uniform shortcut of count_four can go wrong.  One tensor of 1024 equal elements at an aligned offset is 4 waves of 64 lanes, each lane holding
one f32x4; one other value is planted in lane 0 (whose first bin the wave compares against), in its last component, in the last lane of a wave and
in the first lane of the next; 1024 - 8 elements leave the last wave with 62 active lanes, which must add 4 * 62; and the same array one element
behind a 16-byte boundary has a scalar head and tail around a uniform body.  Counts are compared exactly with the numpy restatements of
grad_dist_common and weight_dist_common; the rows of other tensors stay zero and the fill between the records is never counted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import grad_dist_common as G  # noqa: E402
import weight_dist_common as WD  # noqa: E402
from flat_layout import _layout, _ops  # noqa: E402

pytestmark = pytest.mark.gpu
VALUE, OTHER, FILL = 0.5, -3.0, 7.0e3  # three different bins under either rule

# case -> (elements, first element in the flat array, where the other value is planted)
CASES = {
    "lane0_first_component": (1024, 8, 0),
    "lane0_last_component": (1024, 8, 3),
    "last_lane_of_wave0": (1024, 8, 255),
    "lane0_of_wave1": (1024, 8, 256),
    "last_wave_62_lanes": (1024 - 8, 8, None),
    "head_and_tail_around_a_uniform_body": (1024 - 8, 9, None),
}


def _absbin(dev, src, items):
    ops, _ = _ops()
    hist = torch.zeros(3, ops.ABSBIN_BINS, dtype=torch.int32, device=dev)
    ops.absbin_hist(src, items, hist)
    return hist.cpu().numpy().astype(np.int64), G.hist


def _tbbin(dev, src, items):
    ops, _ = _ops()
    hist = torch.zeros(3, ops.TBBIN_ROW, dtype=torch.int32, device=dev)
    ops.tbbin_hist(src, items, hist, torch.zeros(items.shape[0], ops.TBBIN_STATS, dtype=torch.float64, device=dev))
    return hist.cpu().numpy().astype(np.int64), WD.counts_of


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("kernel", [_absbin, _tbbin])
def test_count_four_around_the_wave_uniform_shortcut(dev, kernel, case):
    ops, item_plan = _ops()
    n, off, planted = CASES[case]
    a = np.full(n, VALUE, dtype=np.float32)
    if planted is not None:
        a[planted] = OTHER
    flat, recs = _layout([a], [off], FILL, 9)
    items, _ = item_plan.plan_items(recs, ops.lw_item_elems(), [1])  # one work item, counted into row 1 of three
    assert len(items) == 1 and (flat != FILL).sum() == n
    got, count = kernel(dev, torch.from_numpy(flat).to(dev), item_plan.pack_records(items, dev))
    want = count(a)
    print(case, kernel.__name__, {int(k): int(got[1, k]) for k in np.flatnonzero(got[1])}, {int(k): int(want[k]) for k in np.flatnonzero(want)})
    assert want.sum() == n and (want > 0).sum() == (1 if planted is None else 2) and count(np.float32([FILL]))[want > 0].sum() == 0
    assert np.array_equal(got[1, :len(want)], want)
    assert (got[1, len(want):] == 0).all() and (got[0] == 0).all() and (got[2] == 0).all()
