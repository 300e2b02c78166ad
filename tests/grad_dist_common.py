"""What tests/test_grad_dist_host.py and tests/test_grad_dist_gpu.py share: the selection of the reference's GradDistributionTB callback
(sota_imagenet/callbacks.py:30-60) restated in numpy in the x domain, by both routes — the sorts the reference makes, and the counting formula the
kernels of csrc/optim_hist.hip implement — over bins that are formed here from powers of two, not from the bit pattern the kernels use; and the
fixture recorded from the reference's own callback (tests/golden/grad_dist_ref.npz, written by tests/golden/make_grad_dist_golden.py)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "grad_dist_ref.npz")
NB = 512
Q0 = 77 * 8 + 2  # bin b >= 1 starts at 2^(q // 8 - 127) * (1 + (q % 8) / 8), q = Q0 + b: eight bins per octave from 2^-50 * 1.375
TAGS = ("optim/exp_avg_log", "optim/exp_avg_sq_log", "optim/model_params_log")
SUBSAMPLES = (1, 3, 10)


def edges():
    """float32 [511]: the lower edges of bins 1..511"""
    q = Q0 + np.arange(1, NB)
    return (2.0 ** (q // 8 - 127) * (1.0 + (q % 8) / 8.0)).astype(np.float32)


def bin_of(x):
    """bin of |x| per element: the number of edges at or below it; NaN sorts above every edge, like infinity"""
    return np.searchsorted(edges(), np.abs(np.asarray(x, dtype=np.float32)).ravel(), side="right")


def bin_of_log(v):
    """bin of a recorded log10 value (the reference's clamp -15 lies in bin 0)"""
    return np.searchsorted(np.log10(edges().astype(np.float64)), np.asarray(v, dtype=np.float64).ravel(), side="right")


def hist(x):
    return np.bincount(bin_of(x), minlength=NB).astype(np.int64)


def hist_fast(x):
    """hist() for arrays of tens of millions of elements, by the bit rule (exponent and top three mantissa bits); tests/test_grad_dist_host.py holds
    it to bin_of at every edge and one ulp either side"""
    key = np.ascontiguousarray(x, dtype=np.float32).ravel().view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.bincount(np.clip((key >> 20).astype(np.int64) - Q0, 0, NB - 1), minlength=NB).astype(np.int64)


def sort_route(tensors, s):
    """int64 [512]: per tensor sort(|x|)[::s], concatenate, sort, [::s], bin — what the reference hands to the histogram, before its log10"""
    kept = np.concatenate([np.sort(np.abs(np.asarray(t, dtype=np.float32)).ravel())[::s] for t in tensors])
    return hist(np.sort(kept)[::s])


def formula(hists, s, rep=None):
    """int64 [512] from per-tensor bin counts [n, 512]: c_t(k) = rep_t * (elements of t in bins below k), C(k) = sum_t ceil(c_t(k) / s),
    counts[k] = ceil(C(k+1) / s) - ceil(C(k) / s)"""
    h = np.asarray(hists, dtype=np.int64).reshape(-1, NB)
    rep = np.ones(len(h), dtype=np.int64) if rep is None else np.asarray(rep, dtype=np.int64)
    c = np.concatenate([np.zeros((len(h), 1), dtype=np.int64), np.cumsum(h, axis=1)], axis=1) * rep[:, None]
    C = (-(-c // s)).sum(axis=0)
    return np.diff(-(-C // s))


def formula_of(tensors, s):
    return formula([hist(t) for t in tensors], s)


def kept_total(numels, s):
    """how many values the reference's selection holds: ceil(sum_t ceil(n_t / s) / s)"""
    return -(-sum(-(-int(n) // s) for n in numels) // s)


class Fixture:
    """inputs[tag]: the list of float32 arrays the reference's callback gathered for the tag; recorded[(tag, s)]: the float32 array it handed to
    tb_logger.add_histogram (log10, clamped below at -15); step: the global step it passed"""

    def __init__(self):
        z = np.load(GOLDEN)
        meta = json.loads(bytes(z["meta"]).decode())
        self.step = meta["global_sample_step"]
        self.inputs = {tag: [z[f"in/{tag}/{i}"].reshape(shape) for i, shape in enumerate(meta["shapes"][tag])] for tag in TAGS}
        self.recorded = {(tag, s): z[f"out/{s}/{tag}"] for tag in TAGS for s in SUBSAMPLES}
