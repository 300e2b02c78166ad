"""What tests/test_weight_dist_host.py and tests/test_weight_dist_gpu.py share: the rule of SummaryWriter.add_histogram with its defaults
(torch/utils/tensorboard/writer.py: the default bins; summary.py: histogram, make_histogram) restated in numpy — the edges by the recurrence,
np.histogram over them, the trimming to the support, the statistics in float64 — which is what the reference's WeightDistributionTB
(sota_imagenet/callbacks.py:11-17) hands every state_dict entry to.  Written on np.histogram, where the callback's host code counts by position."""
import numpy as np

N_POS, N_EDGES, N_BINS = 774, 1549, 1548
E_LAST = 9.920775621859783e+19
# the issue's example: of these 13 values np.histogram counts 8
EXAMPLE = [np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0, 1e-13, -1e-13, E_LAST, -E_LAST, 3.0, -3.0]


def edges():
    """float64 [1549]: v = 1e-12; v *= 1.1 while v < 1e20, in double; the negatives reversed, 0, the positives"""
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    return np.array([-e for e in pos[::-1]] + [0.0] + pos, dtype=np.float64)


EDGES = edges()


def counts_of(values):
    """int64 [1548]: np.histogram of the values widened to float64, over the edges"""
    c, _ = np.histogram(np.asarray(values).astype(np.float64).ravel(), bins=EDGES)
    return c.astype(np.int64)


def trim(counts, limits=None):
    """make_histogram's trimming: (bucket_limits, bucket_counts) as lists.  start / end: the first and last non-empty bins; the counts from
    start - 1 (a zero in front if start is 0) to end, the limits from start to end + 1"""
    limits = EDGES if limits is None else limits
    counts = np.asarray(counts)
    nz = np.nonzero(counts > 0)[0]
    if nz.size == 0:
        raise ValueError("The histogram is empty")
    start, end = int(nz.min()), int(nz.max())
    kept = counts[start - 1: end + 1] if start > 0 else np.concatenate([[0], counts[:end + 1]])
    return limits[start: end + 2].tolist(), kept.tolist()


def histogram(values):
    """dict(min, max, num, sum, sum_squares, bucket_limits, bucket_counts) of one tensor, as add_histogram computes it"""
    v = np.asarray(values).astype(np.float64).ravel()
    if v.size == 0:
        raise ValueError("The input has no element.")
    limits, kept = trim(counts_of(v))
    with np.errstate(invalid="ignore"):  # inf - inf is NaN
        return dict(min=float(v.min()), max=float(v.max()), num=int(v.size), sum=float(v.sum()), sum_squares=float(v.dot(v)),
                    bucket_limits=limits, bucket_counts=kept)


def same(a, b):
    """two floats equal, NaN equal to NaN"""
    return a == b or (a != a and b != b)


class Capture:
    """a tb_logger that keeps what add_histogram_raw is given"""

    def __init__(self):
        self.calls = []

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None):
        self.calls.append(dict(tag=tag, min=min, max=max, num=num, sum=sum, sum_squares=sum_squares, bucket_limits=bucket_limits,
                               bucket_counts=bucket_counts, step=global_step))
