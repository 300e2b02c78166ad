"""What the spectral-normalisation tests share: the rule of csrc/spectral_norm.hip restated in float64 stage by stage, the bounds, the test
matrices, and torch's own spectral_norm as the oracle.

Every stage is restated from what the kernel STORED for the stage before (float32 u, v), so roundings do not compound.  With U1 = 2^-23 (one
float32 ulp, relative), a stored float x against its float64 restatement ref, and a double sum of n terms taken in another order than numpy's
(slack n * 2^-52 * sum |terms|):

  u_r     |u - t_r / tau| <= U1 |ref| + dt_r / tau + |ref| dtau / tau            dt_r = L 2^-52 sum_c |W_rc v_c|,
                                                                                 dtau = |dt|_2 + (R + 4) 2^-52 tau   (Cauchy-Schwarz on sum t dt / tau)
  v_c     the same with rows and columns exchanged, from the stored u
  sigma   |sigma - sum_c s_c v_c| <= U1 |ref| + sum_c |v_c| ds_c + L 2^-52 sum_c |s_c v_c|          (eval: sum_r u_r t_r likewise)
  w_hat   |w_hat - W / sigma_ref| <= (2 U1 + dsigma / |sigma_ref|) |ref|         the stored sigma may be one ulp off, the division rounds once
  dw      with d = sum g w_hat, P = |d u_r v_c|: the kernel rounds d, d u_r and (d u_r) v_c (3 U on P, U = 2^-24), the subtraction (U (|g| + P)),
          the division (U |quotient|) — 7 U (|g| + P) / |sigma| covers them with room —, beta dw_old and the sum (2 U |beta dw_old|), and d
          carries the slack of its sum:  <= 7 U (|g| + P) / |sigma| + 2 U |beta dw_old| + n 2^-52 sum |g w_hat| |u_r v_c| / |sigma|
None of these comes from what the code under test gives."""
import numpy as np
import torch

from weight_std_common import worst  # noqa: F401  (max |got - ref| / bound)

U = 2.0 ** -24
U1 = 2.0 ** -23
D = 2.0 ** -52
EPS = float(np.float32(1e-12))
WARM_ITERS = 15

# (rows, row_len) of the regular test matrices: the stem at an element offset = 1 mod 4; fewer rows than a workgroup takes; one row (u = +-1);
# rows no multiple of 4 and shorter than a wave; the longest row; the tallest matrix (the column sum crosses workgroups and slabs)
SHAPES = [(64, 147), (5, 64), (1, 33), (130, 9), (16, 4608), (2048, 64)]
ZERO = (8, 64)


def make_case(seed=0):
    """(flat float32 array, mats [(off, L, R, u0, v0)], n_u, n_v, index of the zero matrix, index of the record that does not fit): the matrices
    of SHAPES, an all-zero one and a record that reaches past the array's end (it owns slots of u and v like the others), NaN in front, in every
    gap and behind"""
    rng = np.random.default_rng(seed)
    mats, off, u0, v0 = [], 5, 0, 0  # 5 % 4 == 1
    for R, L in SHAPES + [ZERO]:
        mats.append((off, L, R, u0, v0))
        off += R * L
        off += 3 + (-off) % 4 + (2 if L == 64 else 0)
        u0, v0 = u0 + R, v0 + L
    n = off + 7
    mats.append((n - 10, 64, 4, u0, v0))
    u0, v0 = u0 + 4, v0 + 64
    flat = np.full(n, np.nan, dtype=np.float32)
    scales = [0.1, 1.0, 3.0, 0.02, 0.01, 0.05]
    for k, (o, L, R, _, _) in enumerate(mats[: len(SHAPES)]):
        flat[o: o + R * L] = (scales[k] * rng.standard_normal(R * L) + (0.01 if k == 1 else 0.0)).astype(np.float32)
    o, L, R, _, _ = mats[len(SHAPES)]
    flat[o: o + R * L] = 0.0
    return flat, mats, u0, v0, len(SHAPES), len(SHAPES) + 1


def mat_mask(n, mats):
    m = np.zeros(n, dtype=bool)
    for o, L, R, _, _ in mats:
        if 0 <= o and o + R * L <= n:
            m[o: o + R * L] = True
    return m


def start_vectors(mats, n_u, n_v, seed=1):
    """normalised float32 N(0, 1) vectors for every matrix"""
    rng = np.random.default_rng(seed)
    u, v = np.zeros(n_u, dtype=np.float32), np.zeros(n_v, dtype=np.float32)
    for _, L, R, u0, v0 in mats:
        a, b = rng.standard_normal(R), rng.standard_normal(L)
        u[u0: u0 + R], v[v0: v0 + L] = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return u, v


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def normalise64(W, x):
    """y = W x, its norm, y / max(norm, eps) and the bound of the float32 result (W [m, n], x [n]; float64)"""
    y = W @ x
    nrm = np.sqrt((y * y).sum())
    den = max(nrm, EPS)
    ref = y / den
    dy = W.shape[1] * D * (np.abs(W) @ np.abs(x))
    dn = np.sqrt((dy * dy).sum()) + (W.shape[0] + 4) * D * nrm
    return y, dy, ref, U1 * np.abs(ref) + dy / den + np.abs(ref) * dn / den


def u_stage64(W, v):
    """from the matrix and the float32 v the kernel read: (reference u, bound)"""
    _, _, ref, bound = normalise64(_f64(W), _f64(v))
    return ref, bound


def v_stage64(W, u, v):
    """from the float32 u and v the kernel STORED: (reference v, its bound, reference sigma, its bound)"""
    W, u, v = _f64(W), _f64(u), _f64(v)
    s, ds, ref, bound = normalise64(W.T, u)
    sig = (s * v).sum()
    dsig = U1 * abs(sig) + (np.abs(v) * ds).sum() + W.shape[1] * D * np.abs(s * v).sum()
    return ref, bound, sig, dsig


def sigma_eval64(W, u, v):
    """sigma = u . (W v) from float32 u, v: (reference, bound)"""
    W, u, v = _f64(W), _f64(u), _f64(v)
    t = W @ v
    dt = W.shape[1] * D * (np.abs(W) @ np.abs(v))
    sig = (u * t).sum()
    return sig, U1 * abs(sig) + (np.abs(u) * dt).sum() + W.shape[0] * D * np.abs(u * t).sum()


def w_hat64(W, sig, dsig):
    ref = _f64(W) / sig
    return ref, (2 * U1 + dsig / abs(sig)) * np.abs(ref)


def iterate64(W, u, v, iters=1):
    """the whole rule in float64 without any float32 rounding (the host tests' restatement): (u, v, sigma)"""
    W = np.asarray(W, dtype=np.float64)
    for _ in range(iters):
        t = W @ v
        u = t / max(np.sqrt((t * t).sum()), 1e-12)
        s = W.T @ u
        v = s / max(np.sqrt((s * s).sum()), 1e-12)
    return u, v, (s * v).sum() if iters else (u * (W @ v)).sum()


def bwd64(g, w_hat, u, v, sigma, beta=0.0, old=None):
    """one matrix: float32 g, w_hat [R, L], u [R], v [L], the float sigma the kernel reads -> (reference in float64, bound)"""
    g, wh, u, v, sigma = _f64(g), _f64(w_hat), _f64(u), _f64(v), float(sigma)
    d = (g * wh).sum()
    uv = np.abs(np.outer(u, v))
    P = abs(d) * uv
    ref = (g - d * np.outer(u, v)) / sigma
    bound = 7 * U * (np.abs(g) + P) / abs(sigma) + g.size * D * np.abs(g * wh).sum() * uv / abs(sigma)
    if beta:
        prev = beta * _f64(old)
        ref, bound = prev + ref, bound + 2 * U * np.abs(prev)
    return ref, bound


def v_to_torch(v, K, Cin):
    """v of one conv from memory order (K, K, Cin) to torch's (Cin, K, K), flat"""
    return np.asarray(v).reshape(K, K, Cin).transpose(2, 0, 1).reshape(-1)


def v_from_torch(v, K, Cin):
    return np.asarray(v).reshape(Cin, K, K).transpose(1, 2, 0).reshape(-1)


def planted(R, L, rng):
    """U diag(2, 1 ... 0.1) V^T [R, L] in float32: the largest singular value is 2, the gap to the next a factor 2"""
    k = min(R, L)
    a, _ = np.linalg.qr(rng.standard_normal((R, k)))
    b, _ = np.linalg.qr(rng.standard_normal((L, k)))
    sv = np.concatenate([[2.0], np.linspace(1.0, 0.1, k - 1)]) if k > 1 else np.array([2.0])
    return ((a * sv) @ b.T).astype(np.float32)


# ---- the oracle: torch's own spectral_norm --------------------------------------------------------------------------------------------------
def torch_linear_sn(W, dtype, seed=0):
    """torch.nn.utils.parametrizations.spectral_norm on a Linear holding W [R, L] (dim 0, as on a Conv2d's [Cout, -1]): the module in train mode
    and its (u, v) after registration"""
    from torch.nn.utils.parametrizations import spectral_norm

    torch.manual_seed(seed)
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=False).to(dtype)
    with torch.no_grad():
        lin.weight.copy_(torch.as_tensor(W).to(dtype))
    lin = spectral_norm(lin)
    p = lin.parametrizations.weight[0]
    return lin.train(), p._u.detach().clone(), p._v.detach().clone()


def torch_sn_forward(lin):
    """one training forward of the parametrisation: (w_hat, sigma, u, v) — sigma as torch forms it, vdot(u, W v) with the advanced vectors"""
    w_hat = lin.weight.detach().clone()  # (one access = one power iteration)
    p = lin.parametrizations.weight[0]
    W = lin.parametrizations.weight.original.detach()
    u, v = p._u.detach().clone(), p._v.detach().clone()
    return w_hat, torch.vdot(u, torch.mv(W, v)), u, v


def sn_oracle(sd, num_classes, double, state=None):
    """oracle.resnet50_ref.make_reference(sd) with torch's spectral_norm on every nn.Conv2d, as the reference registers it; state: {conv name:
    (u, v [Cin, K, K])} forced into _u / _v"""
    from torch.nn.utils.parametrizations import spectral_norm

    from oracle import resnet50_ref as O

    ref = O.make_reference(sd, num_classes=num_classes)
    if double:
        ref = ref.double()
    for name, m in list(ref.named_modules()):
        if isinstance(m, torch.nn.Conv2d):
            spectral_norm(m)
            if state is not None:
                p = m.parametrizations.weight[0]
                with torch.no_grad():
                    p._u.copy_(state[name][0].reshape(-1).to(p._u))
                    p._v.copy_(state[name][1].reshape(-1).to(p._v))
    return ref


def oracle_step(sd, data, target, num_classes, double, state):
    """one training forward + backward on ONE intra-op thread: (logits, {native parameter name: gradient}, {conv name: (u, v) after the step})"""
    from oracle import resnet50_ref as O

    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref = sn_oracle(sd, num_classes, double, state)
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
    after = {name: (m.parametrizations.weight[0]._u.detach().clone(), m.parametrizations.weight[0]._v.detach().clone())
             for name, m in ref.named_modules() if isinstance(m, torch.nn.Conv2d)}
    return out.detach(), grads, after
