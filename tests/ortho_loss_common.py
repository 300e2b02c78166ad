"""What the tests of the weight penalties (csrc/ortho_loss.hip, losses.OrthoLoss / NormLoss) share: both rules restated in float64 stage by
stage, the bounds, and the test matrices.

Every stage is restated from what the kernels STORED for the stage before (G from w; F, gate and coefficient from the stored G; dw from the stored
G and coefficient), so roundings do not compound.  With U = 2^-24 (half a float32 ulp, relative) and D = 2^-52:

  G      a Gram entry is a float32 dot product of length K taken in some order (products rounded once, K - 1 additions in any tree: at most
         K U / (1 - K U) <= (K + 2) U relative to sum |terms| for K <= 2^13) and one subtraction:
             |G_ij - ref| <= (K + 2) U sum_k |w_ik w_jk| + U |ref|
  F      from the stored G: the squares are exact in double, the sum of n = O^2 of them in some order carries n D sum, sqrt and the rounding to
         float32 one each:     |F - ref| <= (U + (n + 4) D) ref
  ratio  one float32 division of the stored F by O:   |ratio - F / O| <= U |F / O|
  gate   the data keep every F / O at least a relative 1e-3 away from min_norm (asserted on the CPU), far more than the errors above: the gate
         must EQUAL the float64 one.  (A matrix whose G is exactly zero has F = 0 and is closed at any min_norm >= 0.)
  coef   from the stored F:  2 / F rounded once:  |coef - ref| <= U |ref|;  exactly 0 where the gate is closed or F == 0
  total  the gated stored F summed in double, rounded to float32:  |total - ref| <= U |ref| + M D sum |F|      (M matrices)
  dw     from the stored G and coefficient, s the scalar the kernel reads.  acc = sum_j G_rj w_jc is a float32 dot product of length O:
         (O + 2) U A with A = sum_j |G_rj w_jc|; s * coef is rounded, its product with acc is rounded (2 U |s coef| A, second order
         dropped into the + 5), the sum with the old value is rounded (U of the result; 2 U |ref| covers it with the second order):
             |dw - ref| <= |s coef| (O + 5) U A + 2 U |ref|
  NormLoss   n_r = sqrt(sum x^2) in double: (L + 2) D relative.  A term (1 - n_r)^2 then carries d_r = 2 |1 - n_r| n_r (L + 2) D + (n_r (L + 2) D)^2
         + 2 D (1 - n_r)^2 (the subtraction and the square);
         the mean over R rows in some order (R + 2) D of it; the sum over T tensors T D; one rounding to float32:
             |total - ref| <= U |ref| + sum_tensors (mean_r d_r + (R + 2) D mean) + T D |ref|
         the gradient's factor f = s (2 / R)(n_r - 1) / n_r: the absolute error of n_r - 1 is n_r (L + 2) D, so f carries |s| (2 / R)(L + 8) D
         with the few double operations behind it, then one rounding to float32; f * w and the sum with the old value are rounded:
             |dw - ref| <= (2 U |f| + |s| (2 / R)(L + 8) D) |w| + 2 U |ref|
None of these comes from what the code under test gives."""
import numpy as np

from weight_std_common import worst  # noqa: F401  (max |got - ref| / bound)

U = 2.0 ** -24
D = 2.0 ** -52
TILE, KSLAB = 64, 512  # what the tests expect of ops.OL_TILE / OL_KSLAB (held together in test_ortho_loss_host.py)
MIN_NORM = 0.01  # the near-orthonormal matrix lies below it, every random one above
CLEAR = 1e-3

# (rows, row_len) by name; conv shapes are (rows, row_len, 1, 1) except the stem's (64, 3, 7, 7)
STEM, SHORT, ONE, RAGGED, LARGEST, ORTHO, ZERO, NEAR = range(8)
SHAPES = [(64, 147), (5, 64), (1, 33), (130, 1152), (512, 4608), (64, 64), (8, 64), (64, 128)]
SCALES = [0.1, 1.0, 3.0, 0.02, 0.01, None, None, None]
TALL = (256, 64)  # rows > row_len: the planner must drop it


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def make_case(seed=0, shapes=None):
    """(flat float32 array, table [(name, kind, offset, shape)]): the matrices of SHAPES as conv weights of a flat model's table — the first at an
    element offset = 1 mod 4 —, the tall one among them, NaN in front, in every gap and behind"""
    rng = np.random.default_rng(seed)
    shapes = SHAPES if shapes is None else shapes
    table, off = [], 5  # 5 % 4 == 1
    for k, (R, L) in enumerate(list(shapes) + [TALL]):
        shape = (64, 3, 7, 7) if (R, L) == (64, 147) else (R, L, 1, 1)
        table.append((f"m{k}.weight", 0, off, shape))
        off += R * L
        off += 3 + (-off) % 4 + (2 if k % 2 else 0)
    n = off + 7
    flat = np.full(n, np.nan, dtype=np.float32)
    for k, (R, L) in enumerate(shapes):
        o = table[k][2]
        if shapes is SHAPES and k == ORTHO:  # exactly orthonormal rows: +-1 at a place of its own per row
            W = np.zeros((R, L), dtype=np.float32)
            W[np.arange(R), rng.permutation(L)[:R]] = rng.choice([-1.0, 1.0], R)
        elif shapes is SHAPES and k == ZERO:
            W = np.zeros((R, L), dtype=np.float32)
        elif shapes is SHAPES and k == NEAR:
            q, _ = np.linalg.qr(rng.standard_normal((L, R)))
            W = (q.T + 1e-3 * rng.standard_normal((R, L))).astype(np.float32)
        else:
            W = ((SCALES[k] if shapes is SHAPES else 0.05) * rng.standard_normal((R, L))).astype(np.float32)
        flat[o: o + R * L] = W.reshape(-1)
    o = table[-1][2]
    flat[o: o + TALL[0] * TALL[1]] = (0.1 * rng.standard_normal(TALL[0] * TALL[1])).astype(np.float32)
    return flat, table


def integer_case(seed=3):
    """weights in {-2 .. 2}: every product and every sum of a Gram entry (at most 4 * 1152 in magnitude) is exact in float32 in any order"""
    rng = np.random.default_rng(seed)
    shapes = [(64, 147), (130, 1152), (70, 600)]
    flat, table = make_case(seed, shapes)
    for (R, L), (_, _, o, _) in zip(shapes, table):
        flat[o: o + R * L] = rng.integers(-2, 3, R * L).astype(np.float32)
    return flat, table[: len(shapes)]


def mat_mask(n, mats):
    m = np.zeros(n, dtype=bool)
    for o, L, R, *_ in mats:
        m[o: o + R * L] = True
    return m


def mat_of(flat, rec):
    o, L, R = rec[:3]
    return np.asarray(flat[o: o + R * L]).reshape(R, L)


# ---- OrthoLoss, stage by stage ----------------------------------------------------------------------------------------------------------------
def gram64(W):
    """(G = W W^T - I in float64 from the float32 W, its bound)"""
    W = _f64(W)
    ref = W @ W.T - np.eye(W.shape[0])
    return ref, (W.shape[1] + 2) * U * (np.abs(W) @ np.abs(W).T) + U * np.abs(ref)


def frob64(G):
    """from the stored float32 G: (F, its bound)"""
    G = _f64(G)
    F = float(np.sqrt((G * G).sum()))
    return F, (U + (G.size + 4) * D) * F


def gate64(F, rows, min_norm):
    return F / rows > min_norm


def clearance(F, rows, min_norm):
    """relative distance of F / O from min_norm (inf for the exactly-zero G, which is closed at any min_norm >= 0)"""
    if F == 0.0:
        return np.inf
    return abs(F / rows - min_norm) / max(F / rows, min_norm)


def coef64(F_stored, gate):
    """from the stored float32 F: (coefficient, bound)"""
    F = float(np.float32(F_stored))
    ref = 2.0 / F if gate and F > 0 else 0.0
    return ref, U * abs(ref)


def total64(F_stored, gates):
    F = _f64(F_stored) * np.asarray(gates, dtype=np.float64)
    ref = float(F.sum())
    return ref, U * abs(ref) + len(F) * D * float(np.abs(F).sum())


def grad64(W, G_stored, coef_stored, s, old=None):
    """one matrix: dw = old + s coef G W from the stored float32 G and coefficient: (reference, bound)"""
    W, G, c, s = _f64(W), _f64(G_stored), float(np.float32(coef_stored)), float(np.float32(s))
    ref = s * c * (G @ W)
    A = np.abs(G) @ np.abs(W)
    if old is not None:
        ref = _f64(old) + ref
    return ref, abs(s * c) * (W.shape[0] + 5) * U * A + 2 * U * np.abs(ref)


def ortho_loss64(mats_w, min_norm):
    """the whole rule in float64 from [W]: (loss, [dloss / dW], [F], [gate])"""
    loss, grads, Fs, gates = 0.0, [], [], []
    for W in mats_w:
        W = np.asarray(W, dtype=np.float64)
        G = W @ W.T - np.eye(W.shape[0])
        F = float(np.sqrt((G * G).sum()))
        gate = gate64(F, W.shape[0], min_norm)
        loss += F if gate else 0.0
        grads.append((2.0 / F) * (G @ W) if gate and F > 0 else np.zeros_like(W))
        Fs.append(F), gates.append(gate)
    return loss, grads, Fs, gates


def ortho_loss32(mats_w, min_norm, s=1.0, slab=KSLAB, plant=None):
    """the rule in plain float32 numpy, slab by slab as the kernels cut it: [(G, F, gate, coef, dw)] and the total.  plant: one of the errors the
    host test plants — "transpose" (an off-diagonal tile of G stored transposed), "slab" (the last slab dropped), "identity" (not subtracted),
    "two" (the factor 2 missing), "gate" (ignored: always open), "s" (not applied)"""
    f = np.float32
    out, total = [], 0.0
    for W in mats_w:
        W = np.asarray(W, dtype=f)
        R, L = W.shape
        cuts = list(range(0, L, slab))
        if plant == "slab" and len(cuts) > 1:
            cuts = cuts[:-1]
        G = np.zeros((R, R), dtype=f)
        for k0 in cuts:
            G = (G + W[:, k0: k0 + slab] @ W[:, k0: k0 + slab].T).astype(f)
        if plant != "identity":
            G = (G - np.eye(R, dtype=f)).astype(f)
        if plant == "transpose" and R >= 2 * TILE:  # tile (1, 0), stored as its own transpose
            G = G.copy()
            G[TILE: 2 * TILE, :TILE] = G[TILE: 2 * TILE, :TILE].T.copy()
        F = f(np.sqrt((G.astype(np.float64) ** 2).sum()))
        gate = bool(F / f(R) > f(min_norm)) or plant == "gate"
        coef = (f(1.0 if plant == "two" else 2.0) / F) if gate and F > 0 else f(0.0)
        sc = coef if plant == "s" else f(s) * coef
        dw = (sc * (G @ W).astype(f)).astype(f)
        total += float(F) if gate else 0.0
        out.append((G, F, gate, coef, dw))
    return out, f(total)


def whole_rule_bounds(W, F, gate):
    """one matrix, for an implementation that takes EVERY stage in float32 from the float32 W (the reference run in float32, and the kernels
    end to end): (bound of its F, bound of dF / dW).  dF <= |dG|_F + 4 U F (the norm is 1-Lipschitz in G; its own sum, sqrt and rounding);
    the gradient (2 / F) G W moves by (2 / F)(dG |W| + (O + 4) U |G| |W|) for G's error and the second product, (dF / F + 2 U) |dw| for the
    factor; nothing where the gate is closed"""
    W = _f64(W)
    G, bG = gram64(W)
    bF = float(np.sqrt((bG * bG).sum())) + 4 * U * F
    if not gate or F == 0:
        return bF, np.zeros_like(W)
    dw = (2.0 / F) * (G @ W)
    return bF, (2.0 / F) * (bG @ np.abs(W) + (W.shape[0] + 4) * U * (np.abs(G) @ np.abs(W))) + (bF / F + 2 * U) * np.abs(dw)


# ---- NormLoss ---------------------------------------------------------------------------------------------------------------------------------
def norm_loss64(rows_w, eps=D):
    """from [W [R, L]] in float32: (loss, its bound, [per-tensor mean]); eps: the precision the sums are taken in — D for the kernels, U for a
    float32 implementation such as the reference run in float32"""
    total, slack, means = 0.0, 0.0, []
    for W in rows_w:
        W = _f64(W)
        R, L = W.shape
        n = np.sqrt((W * W).sum(1))
        e = (L + 2) * eps
        d = 2 * np.abs(1 - n) * n * e + (n * e) ** 2 + 2 * eps * (1 - n) ** 2  # (the subtraction and the square, rounded in eps)
        mean = float(((1 - n) ** 2).mean())
        slack += float(d.mean()) + (R + 2) * eps * mean
        total += mean
        means.append(mean)
    return total, U * abs(total) + slack + len(rows_w) * eps * abs(total), means


def norm_grad64(W, s, old=None, eps=D):
    """one tensor: dw = old + s (2 / R)(n_r - 1) / n_r w, 0 where n_r == 0: (reference, bound); eps as in norm_loss64"""
    W, s = _f64(W), float(np.float32(s))
    R, L = W.shape
    n = np.sqrt((W * W).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        fac = np.where(n > 0, s * (2.0 / R) * (n - 1.0) / n, 0.0)[:, None]
    ref = fac * W
    if old is not None:
        ref = _f64(old) + ref
    return ref, (2 * U * np.abs(fac) + abs(s) * (2.0 / R) * (L + 8) * eps) * np.abs(W) + 2 * U * np.abs(ref)


def norm_case(seed=5):
    """(flat float32 array, table): a conv, an FC-like matrix with a zero row, a BatchNorm weight of 64 (rows of one element, one of them 0), a
    long-row matrix, and what the rule leaves out — a bias, a BatchNorm of 32 and a buffer —, NaN in front, in every gap and behind"""
    rng = np.random.default_rng(seed)
    specs = [("conv.weight", 0, (64, 3, 7, 7)), ("conv.bias", 0, (64,)), ("bn.weight", 0, (64,)), ("bn.bias", 0, (64,)), ("fc.weight", 0, (10, 37)),
             ("small.weight", 0, (32,)), ("bn.running_var", 1, (64,)), ("long.weight", 0, (6, 4608, 1, 1)), ("wide.weight", 0, (300, 9, 1, 1))]
    table, off = [], 5
    for name, kind, shape in specs:
        table.append((name, kind, off, shape))
        off += int(np.prod(shape))
        off += 3 + (-off) % 4
    flat = np.full(off + 7, np.nan, dtype=np.float32)
    for name, kind, o, shape in table:
        n = int(np.prod(shape))
        scale = {"bn.weight": 1.0, "long.weight": 0.02, "fc.weight": 0.3}.get(name, 0.1)
        flat[o: o + n] = (scale * rng.standard_normal(n)).astype(np.float32)
    by = {t[0]: t for t in table}
    flat[by["fc.weight"][2] + 3 * 37: by["fc.weight"][2] + 4 * 37] = 0.0  # a zero row
    flat[by["bn.weight"][2] + 7] = 0.0
    return flat, table
