"""What the WeightNorm tests and the fixture's maker share: the rule of sota_imagenet/callbacks.py:120-122 restated in float64, and the two bounds.

With u = 2^-24 and, in float64 from the fp32 input row X of length L, the mean M, the centred norm N and the result Y = (X - M) / N:

  native bound     |y - Y| <= 8u|Y| + 4u|M| / N
      the kernel's mean is one rounding of an essentially exact (double) mean: an error of at most u|M| in m, which moves every c_i by as much,
      i.e. y by u|M| / N; c, nrm and the quotient are one rounding each: about 4u|Y| + 2u|M| / N in total, doubled.
  reference bound  |y - Y| <= 8u|Y| + (4u|M| + G u mean|X|) / N,   G = 2 + ceil(log2 L)
      the reference's own float32 torch result does not meet the native bound: its mean is accumulated in float32 (pairwise, depth about
      log2 L), an error of up to G u mean|X| in m.
Neither comes from what the code under test gives."""
import math

import numpy as np

U = 2.0 ** -24
GRID = [(0.0, 1.0), (0.05, 0.02), (-3.0, 1e-3), (1e3, 1.0)]  # (mean, sd) of the test rows


def rule64(x):
    """x: float32 [rows, L] -> (M [rows, 1], N [rows, 1], Y [rows, L]) in float64; a constant row has N == 0 and Y all NaN"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    M = x.mean(axis=-1, keepdims=True)
    C = x - M
    N = np.sqrt((C * C).sum(axis=-1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        Y = C / N
    return M, N, Y


def native_bound(M, N, Y):
    with np.errstate(invalid="ignore", divide="ignore"):
        return 8 * U * np.abs(Y) + 4 * U * np.abs(M) / N


def reference_bound(x, M, N, Y):
    x = np.asarray(x, dtype=np.float64)
    G = 2 + math.ceil(math.log2(x.shape[-1])) if x.shape[-1] > 1 else 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return 8 * U * np.abs(Y) + (4 * U * np.abs(M) + G * U * np.abs(x).mean(axis=-1, keepdims=True)) / N


def reapply_bound(b0, y1):
    """how far a second application may move the result y1 of a first one whose input had the native bound b0 [rows, L].  y1 = Y + e with
    |e_i| <= b0_i, mean Y = 0, ||Y|| = 1, so y1's own mean M1 and centred norm N1 obey |M1| <= mean(b0) and |N1 - 1| <= ||b0||_2 =: s, and its
    exact image Y' = (y1 - M1) / N1 lies within (|y1_i| s + mean(b0)) / (1 - s) of y1_i; the kernel's second result lies within the native
    bound of y1, taken as an input, of Y'.  The sum of the two.  (The native bound of the ORIGINAL row alone is not a bound here: an element
    with |Y_i| near 0 has a bound near 4u|M| / N, and the mean of the other elements' roundings, which the second application removes, is
    larger than that for a long row of small mean; the prescribed arithmetic run on the CPU moves such elements by 5 times as much.)"""
    y1 = np.asarray(y1, dtype=np.float64)
    s = np.sqrt((b0 * b0).sum(axis=-1, keepdims=True))
    M1, N1, Y1 = rule64(y1)
    return native_bound(M1, N1, Y1) + (np.abs(y1) * s + b0.mean(axis=-1, keepdims=True)) / (1 - s)


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements (rows with N == 0 are the caller's to treat); 0 for an empty array"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - want) / bound).max())
