"""What the weight-transform tests share: the row rules of csrc/weight_std.hip restated in float64, their bounds, the test rows, and the
oracle — oracle.resnet50_ref with torch.nn.utils.parametrize on every Conv2d, which is what the reference's conv_to_ws_conv / ForwardWeightNorm do.

With u = 2^-24, a row w[0..L) in float32, and in float64 from those floats mu = mean(w), is = 1 / sqrt(var + eps) (standardise) or 1 (centre):

  forward   |w_hat - (w - mu) * is| <= 4u (|ref| + |mu| * is)
      the kernel rounds the (essentially exact, double) mean to float: at most u|mu|, which moves every element by u|mu| * is; the subtraction, is
      and the product are one rounding each: three on the result.  Four in all.
  invstd    within 2^-23 relative: one rounding of a double value whose own error is of the order of 2^-53.
  backward  |dw - is * (g - m1 - w_hat * m2)| <= 8u * is * (|g| + |m1| + |w_hat * m2|)  (+ u |beta * dw_old| when beta is 1)
      m1, m2 rounded to float, the product, two subtractions, the scaling: six roundings in the expression, plus the accumulate; each is relative
      to a partial result no larger than |g| + |m1| + |w_hat * m2|.
None of these comes from what the code under test gives."""
import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-5
STANDARDISE, CENTRE = 1, 2
MODES = {"standardise": STANDARDISE, "centre": CENTRE}
CONST = 0.5  # the constant row: its sum and mean are exact in double, so w - (float)mu is exactly 0


def make_rows(seed=0):
    """(flat float32 array, [(first element, row_len)], index of the constant row).  Rows of 147 (three, the first one element off a 16-byte
    boundary, so every alignment of head and tail occurs), 64, 576, 1024, 1152 and 4608 elements — one wave per row, nine rows: three workgroups,
    the last one with idle waves — and one constant row; NaN everywhere else: in front, in every gap between two tensors and behind."""
    rng = np.random.default_rng(seed)
    rows, off = [], 5  # 5 % 4 == 1: one element off a 16-byte boundary
    groups = [(147, 3), (64, 1), (576, 1), (1024, 1), (1152, 1), (4608, 1), (192, 1)]
    for L, n in groups:
        rows.extend((off + r * L, L) for r in range(n))
        off += n * L
        off += 3 + (-off) % 4 + (0 if L != 64 else 2)  # a gap of 3..8 elements: the next tensor starts on varying alignments
    flat = np.full(off + 7, np.nan, dtype=np.float32)
    means = [0.0, 0.05, -3.0, 1e3, 0.01, -0.2, 1.0, 0.0]
    sds = [1.0, 0.02, 1e-3, 1.0, 0.05, 0.3, 2.0, 1e-2]
    for k, (o, L) in enumerate(rows[:-1]):
        flat[o: o + L] = (means[k] + sds[k] * rng.standard_normal(L)).astype(np.float32)
    o, L = rows[-1]
    flat[o: o + L] = CONST
    return flat, rows, len(rows) - 1


def row_mask(n, rows):
    m = np.zeros(n, dtype=bool)
    for o, L in rows:
        m[o: o + L] = True
    return m


def fwd64(w, mode, eps=EPS):
    """one row, float32 -> (mu, is, w_hat) in float64"""
    w = np.asarray(w, dtype=np.float32).astype(np.float64)
    mu = w.mean()
    var = max((w * w).mean() - mu * mu, 0.0)
    inv = 1.0 / np.sqrt(var + eps) if mode == STANDARDISE else 1.0
    return mu, inv, (w - mu) * inv


def fwd_bound(mu, inv, ref):
    return 4 * U * (np.abs(ref) + abs(mu) * inv)


def bwd64(g, w_hat, inv, mode):
    """one row: float32 g and w_hat, the float invstd the kernel reads -> (reference in float64, its bound without the accumulate term)"""
    g = np.asarray(g, dtype=np.float32).astype(np.float64)
    wh = np.asarray(w_hat, dtype=np.float32).astype(np.float64)
    inv = float(inv)
    m1 = g.mean()
    m2 = (g * wh).mean() if mode == STANDARDISE else 0.0
    ref = inv * (g - m1 - wh * m2)
    return ref, 8 * U * inv * (np.abs(g) + abs(m1) + np.abs(wh * m2))


def worst(got, ref, bound):
    """max |got - ref| / bound; elements with a zero bound must match exactly (they count as 0, anything else as inf)"""
    d = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- the oracle: torch's own parametrisation on the torch model ------------------------------------------------------------------------------
class _Transform(torch.nn.Module):
    def __init__(self, mode):
        super().__init__()
        self.mode = mode

    def forward(self, w):
        from oracle.bresnet50_ref import ws

        return ws(w, EPS) if self.mode == STANDARDISE else w - w.mean(dim=(1, 2, 3), keepdim=True)


def parametrised_oracle(sd, mode, num_classes, double=False):
    """oracle.resnet50_ref.make_reference(sd) with the transform registered on every nn.Conv2d, as the reference registers it"""
    from torch.nn.utils import parametrize

    from oracle import resnet50_ref as O

    ref = O.make_reference(sd, num_classes=num_classes)
    if double:
        ref = ref.double()
    for m in list(ref.modules()):
        if isinstance(m, torch.nn.Conv2d):
            parametrize.register_parametrization(m, "weight", _Transform(mode))
    return ref


def oracle_step(sd, data, target, mode, num_classes, double):
    """one training forward + backward on ONE intra-op thread (the fp32 distance to fp64 depends on torch-CPU's reduction order):
    (logits, {parameter name as the native model has it: gradient})"""
    from oracle import resnet50_ref as O

    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref = parametrised_oracle(sd, mode, num_classes, double)
        ref.train()
        out = ref(data.double() if double else data)
        if double:
            lp = torch.log_softmax(out, 1)
            loss = (0.9 * -(lp * target.double()).sum(1) + 0.1 * -lp.mean(1)).mean()
        else:
            loss = O.smooth_ce(out, target, 0.1)
        loss.backward()
    finally:
        torch.set_num_threads(n)
    grads = {k.replace(".parametrizations.weight.original", ".weight"): p.grad.detach() for k, p in ref.named_parameters()}
    return out.detach(), grads


def flat_grads(names, grads):
    return torch.cat([grads[k].double().cpu().flatten() for k in names])
