"""What the GPU tests of the two counting kernels (test_grad_dist_gpu.py, test_weight_dist_gpu.py, test_hist_count_gpu.py) share: drawn arrays laid
into one flat array with a fill value between them.  Each caller brings its own fill and exponent range."""
import numpy as np


def _ops():
    from sota_imagenet_amd import item_plan, ops

    return ops, item_plan


def _draw(rng, n, lo_exp, hi_exp):
    """|x| = 10^u, u uniform over [lo_exp, hi_exp], signs mixed, some exact zeros"""
    x = (10.0 ** rng.uniform(lo_exp, hi_exp, n)).astype(np.float32) * rng.choice(np.float32([-1, 1]), n)
    x[rng.uniform(size=n) < 0.05] = 0.0
    return x


def _layout(arrays, offsets, fill, tail):
    """the arrays laid into one flat array at `offsets` (None: each at the next multiple of 4 behind a gap of 4), `fill` everywhere else;
    returns (flat numpy, [(offset, numel)])"""
    recs, end = [], 0
    for i, a in enumerate(arrays):
        off = offsets[i] if offsets else (end + 4 + 3) // 4 * 4
        assert off >= end
        recs.append((off, a.size))
        end = off + a.size
    flat = np.full(end + tail, fill, dtype=np.float32)
    for (off, n), a in zip(recs, arrays):
        flat[off:off + n] = a.ravel()
    return flat, recs
