"""The forward spectral normalisation on the GPU: the kernels of csrc/spectral_norm.hip stage by stage against float64 on synthetic matrices, the
warm start on planted spectra, torch's own spectral_norm, the executor's wiring against a plain model fed w_hat, the whole step against the
parametrised torch oracle, and the ForwardSpectralNorm callback.  The bounds are those of tests/spectral_common.py; the wiring and callback tests
run at N=2, 64 px, 10 classes, the oracle step at N=8."""
import functools

import numpy as np
import pytest
import torch

import exec_gpu_common as E
import spectral_common as SN

pytestmark = pytest.mark.gpu
N, S, NC = 2, 64, 10
_model = functools.partial(E.model, num_classes=NC)
SENT = -7.0


@pytest.fixture(scope="module")
def case():
    flat, mats, n_u, n_v, zero, bad = SN.make_case()
    u, v = SN.start_vectors(mats, n_u, n_v)
    return dict(flat=flat, mats=mats, n_u=n_u, n_v=n_v, zero=zero, bad=bad, u=u, v=v, mask=SN.mat_mask(flat.size, mats))


def _forward(flat, mats, u, v, iters, dev, dest="out"):
    """one ops.spectral_fwd: dest "out" (w_hat into NaN), "in" (w_hat is w) or None (no division) -> numpy (w_hat or None, u, v, sigma)"""
    ops, item_plan = E.mods()
    w = torch.from_numpy(flat).to(dev)
    w_hat = {"out": torch.full_like(w, float("nan")), "in": w, None: None}[dest]
    ud, vd = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    sigma = torch.full((len(mats),), SENT, device=dev)
    ops.spectral_fwd(w, w_hat, ud, vd, sigma, ops.spectral_scratch(ud, vd), item_plan.pack_records(mats, dev, item_plan.SPECTRAL_FIELDS), iters)
    torch.cuda.synchronize()
    if dest != "in":
        assert E.np_same(w.cpu().numpy(), flat), "the source is read only"
    return (None if w_hat is None else w_hat.cpu().numpy()), ud.cpu().numpy(), vd.cpu().numpy(), sigma.cpu().numpy()


def _mat(flat, rec):
    o, L, R, _, _ = rec
    return flat[o: o + R * L].reshape(R, L)


def _check_iteration(c, v_in, got, tag):
    """one training iteration's outputs (w_hat, u, v, sigma) against the stages restated from the stored vectors; returns the worst ratios"""
    w_hat, u, v, sigma = got
    worst = dict(u=0.0, v=0.0, sigma=0.0, w_hat=0.0)
    for i, rec in enumerate(c["mats"]):
        o, L, R, u0, v0 = rec
        if i in (c["zero"], c["bad"]):
            continue
        W = _mat(c["flat"], rec)
        ref, bound = SN.u_stage64(W, v_in[v0: v0 + L])
        ru = SN.worst(u[u0: u0 + R], ref, bound)
        ref, bound, sig, dsig = SN.v_stage64(W, u[u0: u0 + R], v[v0: v0 + L])
        rv = SN.worst(v[v0: v0 + L], ref, bound)
        rs = abs(float(sigma[i]) - sig) / dsig
        ref, bound = SN.w_hat64(W, sig, dsig)
        rw = SN.worst(w_hat[o: o + R * L].reshape(R, L), ref, bound) if w_hat is not None else 0.0
        print(f"{tag} {R}x{L}: worst error / bound  u {ru:.3f}  v {rv:.3f}  sigma {rs:.3f}  w_hat {rw:.3f}")
        assert max(ru, rv, rs, rw) <= 1.0, (tag, R, L, ru, rv, rs, rw)
        for k, r in zip(worst, (ru, rv, rs, rw)):
            worst[k] = max(worst[k], r)
    return worst


def _check_untouched(c, before, got):
    """the zero matrix, the record that does not fit, the gaps"""
    w_hat, u, v, sigma = got
    o, L, R, u0, v0 = c["mats"][c["zero"]]
    assert sigma[c["zero"]] == 0.0 and (u[u0: u0 + R] == 0).all() and (v[v0: v0 + L] == 0).all(), "a zero matrix: zero vectors, sigma 0"
    o2, L2, R2, u2, v2 = c["mats"][c["bad"]]
    assert sigma[c["bad"]] == SENT and E.np_same(u[u2: u2 + R2], before[0][u2: u2 + R2]) and E.np_same(v[v2: v2 + L2], before[1][v2: v2 + L2])
    if w_hat is not None:
        assert np.isnan(w_hat[o: o + R * L]).all(), "0 / 0, as torch"
        assert np.isnan(w_hat[~c["mask"]]).all(), "gaps (the skipped record's among them) are neither read into a matrix nor written"
        keep = c["mask"].copy()
        keep[o: o + R * L] = False
        assert np.isfinite(w_hat[keep]).all(), "the neighbours of the zero matrix are unaffected"


# ---- 1. matrices, forward ------------------------------------------------------------------------------------------------------------------
def test_training_iteration_against_float64(dev, case):
    c = case
    got = _forward(c["flat"], c["mats"], c["u"], c["v"], 1, dev)
    w = _check_iteration(c, c["v"], got, "iters=1")
    print("iters=1 worst ratios:", {k: round(x, 3) for k, x in w.items()})
    _check_untouched(c, (c["u"], c["v"]), got)
    o, L, R, u0, v0 = c["mats"][2]
    assert R == 1 and abs(got[1][u0]) == 1.0, "one row: u = +-1"
    # bit for bit on a second run; in place (the bake) gives the bits of out of place, gaps untouched
    again = _forward(c["flat"], c["mats"], c["u"], c["v"], 1, dev)
    assert E.np_same(again[0][c["mask"]], got[0][c["mask"]]) and all(E.np_same(a, b) for a, b in zip(again[1:], got[1:]))
    ip = _forward(c["flat"], c["mats"], c["u"], c["v"], 1, dev, dest="in")
    assert E.np_same(ip[0][c["mask"]], got[0][c["mask"]]) and np.isnan(ip[0][~c["mask"]]).all()
    assert all(E.np_same(a, b) for a, b in zip(ip[1:], got[1:]))


def test_two_iterations_are_one_after_the_other(dev, case):
    c = case
    first = _forward(c["flat"], c["mats"], c["u"], c["v"], 1, dev, dest=None)
    second = _forward(c["flat"], c["mats"], first[1], first[2], 1, dev)
    _check_iteration(c, first[2], second, "second of two")
    both = _forward(c["flat"], c["mats"], c["u"], c["v"], 2, dev)
    assert E.np_same(both[0][c["mask"]], second[0][c["mask"]]) and all(E.np_same(a, b) for a, b in zip(both[1:], second[1:]))
    _check_untouched(c, (c["u"], c["v"]), both)


def test_eval_rule_leaves_the_vectors_alone(dev, case):
    c = case
    _, u1, v1, _ = _forward(c["flat"], c["mats"], c["u"], c["v"], 1, dev, dest=None)
    got = _forward(c["flat"], c["mats"], u1, v1, 0, dev)
    w_hat, u, v, sigma = got
    assert E.np_same(u, u1) and E.np_same(v, v1), "eval: u and v bit-unchanged"
    worst = 0.0
    for i, rec in enumerate(c["mats"]):
        o, L, R, u0, v0 = rec
        if i in (c["zero"], c["bad"]):
            continue
        W = _mat(c["flat"], rec)
        sig, dsig = SN.sigma_eval64(W, u[u0: u0 + R], v[v0: v0 + L])
        ref, bound = SN.w_hat64(W, sig, dsig)
        rs, rw = abs(float(sigma[i]) - sig) / dsig, SN.worst(w_hat[o: o + R * L].reshape(R, L), ref, bound)
        print(f"iters=0 {R}x{L}: worst error / bound  sigma {rs:.3f}  w_hat {rw:.3f}")
        assert rs <= 1.0 and rw <= 1.0, (R, L, rs, rw)
        worst = max(worst, rs, rw)
    _check_untouched(c, (u1, v1), got)
    ip = _forward(c["flat"], c["mats"], u1, v1, 0, dev, dest="in")
    assert E.np_same(ip[0][c["mask"]], w_hat[c["mask"]]) and np.isnan(ip[0][~c["mask"]]).all() and E.np_same(ip[3], sigma)


# ---- 2. matrices, backward -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forwarded(dev, case):
    """the state one training forward leaves: (w_hat, u, v, sigma) as numpy, with finite values put where the zero matrix gave NaN / 0"""
    c = case
    w_hat, u, v, sigma = _forward(c["flat"], c["mats"], c["u"], c["v"], 1, dev)
    o, L, R, u0, v0 = c["mats"][c["zero"]]
    rng = np.random.default_rng(11)
    w_hat[o: o + R * L] = rng.standard_normal(R * L).astype(np.float32)
    sigma[c["zero"]] = 1.5
    u[u0: u0 + R], v[v0: v0 + L] = 0.3, -0.1
    g = np.full(c["flat"].size, np.nan, dtype=np.float32)
    old = np.full(c["flat"].size, np.nan, dtype=np.float32)
    for k, (o, L, R, _, _) in enumerate(c["mats"]):
        if k != c["bad"]:
            g[o: o + R * L] = ((0.3 if k % 2 else -0.01) + 10.0 ** (-(k % 3)) * rng.standard_normal(R * L)).astype(np.float32)
            old[o: o + R * L] = (1.0 + rng.standard_normal(R * L)).astype(np.float32)
    return w_hat, u, v, sigma, g, old


def _backward(c, f, dw0, beta, dev, rows=None):
    ops, item_plan = E.mods()
    w_hat, u, v, sigma, g, _ = f
    t = [torch.from_numpy(x).to(dev) for x in (g, w_hat, u, v, sigma)]
    dw = torch.from_numpy(dw0).to(dev)
    kw = {} if rows is None else dict(row_begin=rows[0], row_end=rows[1])
    ops.spectral_bwd(t[0], t[1], t[2], t[3], t[4], dw, ops.spectral_scratch(t[2], t[3]),
                     item_plan.pack_records(c["mats"], dev, item_plan.SPECTRAL_FIELDS), beta=beta, **kw)
    torch.cuda.synchronize()
    return dw.cpu().numpy()


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_backward_against_float64(dev, case, forwarded, beta):
    c, f = case, forwarded
    w_hat, u, v, sigma, g, old = f
    start = old if beta else np.full_like(old, np.nan)  # with beta == 0 dw holds NaN beforehand and is never read
    got = _backward(c, f, start, beta, dev)
    assert np.isnan(got[~c["mask"]]).all(), "gaps are untouched"
    assert np.isfinite(got[c["mask"]]).all()
    worst = 0.0
    for i, (o, L, R, u0, v0) in enumerate(c["mats"]):
        if i == c["bad"]:
            continue
        sl = slice(o, o + R * L)
        ref, bound = SN.bwd64(g[sl].reshape(R, L), w_hat[sl].reshape(R, L), u[u0: u0 + R], v[v0: v0 + L], sigma[i], beta, old[sl].reshape(R, L))
        r = SN.worst(got[sl].reshape(R, L), ref, bound)
        print(f"beta={beta} {R}x{L}: worst error / bound {r:.3f}")
        assert r <= 1.0, (R, L, r)
        worst = max(worst, r)
    print(f"beta={beta}: worst error / bound {worst:.3f}")
    # a slice of u's rows: whole matrices inside it are written, the others — one that the slice cuts among them — keep their bits
    m1, m4 = c["mats"][1], c["mats"][4]
    part = _backward(c, f, start, beta, dev, rows=(m1[3], m4[3] + 3))
    for i, (o, L, R, u0, v0) in enumerate(c["mats"]):
        if i == c["bad"]:
            continue
        sl = slice(o, o + R * L)
        assert E.np_same(part[sl], got[sl] if 1 <= i < 4 else start[sl]), i
    assert E.np_same(_backward(c, f, start, beta, dev)[c["mask"]], got[c["mask"]]), "two runs, the same bits"


# ---- 3. warm start ------------------------------------------------------------------------------------------------------------------------
def _planted_case(seed):
    rng = np.random.default_rng(seed)
    shapes = [s for s in SN.SHAPES if s[0] > 1]
    mats, off, u0, v0, blocks = [], 5, 0, 0, []
    for R, L in shapes:
        mats.append((off, L, R, u0, v0))
        blocks.append(SN.planted(R, L, rng))
        off += R * L + 3 + (-(off + R * L)) % 4
        u0, v0 = u0 + R, v0 + L
    flat = np.full(off + 4, np.nan, dtype=np.float32)
    for (o, L, R, _, _), W in zip(mats, blocks):
        flat[o: o + R * L] = W.reshape(-1)
    return flat, mats, u0, v0


def test_warm_start_finds_a_planted_spectrum(dev):
    flat, mats, n_u, n_v = _planted_case(3)
    u, v = SN.start_vectors(mats, n_u, n_v, seed=4)
    w_hat, u, v, sigma = _forward(flat, mats, u, v, SN.WARM_ITERS, dev, dest=None)
    assert w_hat is None
    for (o, L, R, _, _), s in zip(mats, sigma):
        print(f"planted {R}x{L}: sigma after {SN.WARM_ITERS} iterations {s:.9f}, off 2 by {abs(s - 2) / 2:.2e}")
        assert abs(float(s) - 2.0) <= 1e-6 * 2.0, (R, L, s)


# ---- 4. against torch itself ----------------------------------------------------------------------------------------------------------------
def _dist(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("which", ["planted", "random"])
def test_one_iteration_against_torch_spectral_norm(dev, case, which):
    """torch's parametrisation on the CPU in float32 and float64, all three teacher-forced with the float32 module's _u, _v after registration:
    native sigma and w_hat are no further from torch-fp64 than 2 x torch-fp32's own distance + 2^-23 (relative max-norm)"""
    if which == "planted":
        flat, mats, n_u, n_v = _planted_case(3)
    else:
        mats = [m for i, m in enumerate(case["mats"]) if i < len(SN.SHAPES)]
        flat, n_u, n_v = case["flat"], case["n_u"], case["n_v"]
    u, v = np.zeros(n_u, dtype=np.float32), np.zeros(n_v, dtype=np.float32)
    refs = []
    for o, L, R, u0, v0 in mats:
        W = flat[o: o + R * L].reshape(R, L)
        l32, a, b = SN.torch_linear_sn(W, torch.float32)
        l64, _, _ = SN.torch_linear_sn(W, torch.float64)
        p = l64.parametrizations.weight[0]
        with torch.no_grad():
            p._u.copy_(a.double()), p._v.copy_(b.double())
        u[u0: u0 + R], v[v0: v0 + L] = a.numpy(), b.numpy()
        refs.append((SN.torch_sn_forward(l32), SN.torch_sn_forward(l64)))
    w_hat, u, v, sigma = _forward(flat, mats, u, v, 1, dev)
    for i, ((o, L, R, u0, v0), (t32, t64)) in enumerate(zip(mats, refs)):
        wn, w32, w64 = w_hat[o: o + R * L].reshape(R, L), t32[0].numpy(), t64[0].numpy()
        dn, d32 = _dist(wn, w64), _dist(w32, w64)
        sn_, s32 = abs(float(sigma[i]) - t64[1].item()) / abs(t64[1].item()), abs(t32[1].item() - t64[1].item()) / abs(t64[1].item())
        un, u32 = _dist(u[u0: u0 + R], t64[2].numpy()), _dist(t32[2].numpy(), t64[2].numpy())
        vn, v32 = _dist(v[v0: v0 + L], t64[3].numpy()), _dist(t32[3].numpy(), t64[3].numpy())
        print(f"{which} {R}x{L}: distance to torch-fp64, native / torch-fp32:  w_hat {dn:.2e} / {d32:.2e}  sigma {sn_:.2e} / {s32:.2e}  "
              f"u {un:.2e} / {u32:.2e}  v {vn:.2e} / {v32:.2e}")
        assert dn <= 2 * d32 + SN.U1 and sn_ <= 2 * s32 + SN.U1, (R, L, dn, d32, sn_, s32)
        assert un <= 2 * u32 + SN.U1 and vn <= 2 * v32 + SN.U1, (R, L, un, u32, vn, v32)


# ---- the model tests -----------------------------------------------------------------------------------------------------------------------
def _batch(index=0, n=N):
    from sota_imagenet_amd.synth import synthetic_batch

    return synthetic_batch(n, S, num_classes=NC, seed=3, index=index)


def _rows(t):
    """a conv tensor in torch's OIHW shape -> [Cout, K*K*Cin] in memory order, numpy"""
    return t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], -1).cpu().numpy()


def _debug(m, shape, convs):
    get = lambda k, s: m.debug_tensor(shape, k[: -len(".weight")] + s)  # noqa: E731
    return ({k: get(k, ".w_hat") for k in convs}, {k: get(k, ".sn_u").cpu().numpy() for k in convs},
            {k: get(k, ".sn_v").reshape(-1).cpu().numpy() for k in convs}, {k: get(k, ".sn_sigma").item() for k in convs})


def _check_conv_grads(ga, gb, w_hat, u, v, sigma, convs, tag, prev=None):
    worst = 0.0
    for k in convs:
        ref, bound = SN.bwd64(_rows(gb[k]), w_hat[k].reshape(w_hat[k].shape[0], -1).cpu().numpy(), u[k], v[k], sigma[k],
                              1.0 if prev is not None else 0.0, None if prev is None else _rows(prev[k]))
        x = SN.worst(_rows(ga[k]), ref, bound)
        worst = max(worst, x)
        assert x <= 1.0, (tag, k, x)
    print(f"{tag}: conv gradients, worst error / bound {worst:.3f}")


# ---- 5. the executor wiring, exactly ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_executor_wiring_is_exact(dev, dtype):
    data, target = _batch()
    a = _model(dtype).cuda()
    a.set_spectral_norm(True)
    assert a.spectral_norm and a.weight_transform == 0 and a.spectral_u.numel() == 26560 and a.spectral_v.numel() == 52883
    convs = E.conv_names(a)
    pa = dict(a.named_parameters())
    state0 = a.spectral_state()
    out_a, ga = E.step(a, data, target)
    w_hat, u, v, sigma = _debug(a, (N, S, S), convs)
    state1 = a.spectral_state()
    # what the executor reads is the model's own state, in torch's layout, and one iteration of the kernels' rule from the warmed state
    for k in ("conv1.weight", "layer1.0.conv2.weight", "layer4.0.downsample.0.weight"):
        name, (co, ci, kh, _) = k[: -len(".weight")], pa[k].shape
        assert np.array_equal(state1[name][0].cpu().numpy(), u[k]) and np.array_equal(SN.v_from_torch(state1[name][1].cpu().numpy(), kh, ci), v[k])
        W = _rows(pa[k])
        ref, bound = SN.u_stage64(W, SN.v_from_torch(state0[name][1].cpu().numpy(), kh, ci))
        assert SN.worst(u[k], ref, bound) <= 1.0, k
        ref, bound, sig, dsig = SN.v_stage64(W, u[k], v[k])
        assert SN.worst(v[k], ref, bound) <= 1.0 and abs(sigma[k] - sig) <= dsig, k
        ref, bound = SN.w_hat64(W, sig, dsig)
        assert SN.worst(w_hat[k].reshape(co, -1).cpu().numpy(), ref, bound) <= 1.0, k
        top = np.linalg.svd(W.astype(np.float64), compute_uv=False)[0]
        assert 0.5 * top < sigma[k] <= top * (1 + 1e-6), "u^T W v of unit vectors: at most the largest singular value, and near it after the warm start"

    # B: plain, its conv weights are A's w_hat
    b = _model(dtype).cuda()
    with torch.no_grad():
        for k, p in b.named_parameters():
            p.copy_(w_hat[k].permute(0, 3, 1, 2) if k in w_hat else pa[k])
    out_b, gb = E.step(b, data, target)
    assert E.same_bits(out_a, out_b), "the logits of A are those of a plain model on w_hat"
    for k in ga:
        if k not in w_hat:
            assert E.same_bits(ga[k], gb[k]), f"{k}: BatchNorm / FC gradients do not see the parametrisation"
    _check_conv_grads(ga, gb, w_hat, u, v, sigma, convs, f"{dtype} step 1")

    # a second step without zero_grad: u, v advance once more, so the rule is applied again, on top of the first step's gradients
    out_a2, ga2 = E.step(a, data, target, zero=False)
    w_hat2, u2, v2, sigma2 = _debug(a, (N, S, S), convs)
    assert any(not np.array_equal(u2[k], u[k]) for k in convs), "a training forward advances the state"
    with torch.no_grad():
        for k in convs:
            dict(b.named_parameters())[k].copy_(w_hat2[k].permute(0, 3, 1, 2))
    out_b2, gb2 = E.step(b, data, target)
    assert E.same_bits(out_a2, out_b2)
    _check_conv_grads(ga2, gb2, w_hat2, u2, v2, sigma2, convs, f"{dtype} step 2 (accumulated)", prev=ga)
    for k in ga:
        if k not in w_hat:
            assert E.same_bits(ga2[k], ga[k] + gb2[k]), f"{k}: accumulated gradient"

    # the backward in two segment calls (what the DDP hook does) gives the bits of one call: from the same state, by teacher forcing
    a.load_spectral_state(state1)
    out_r, gr = E.step(a, data, target)
    nseg = len(a.grad_segments)
    seen = []
    a.load_spectral_state(state1)
    a._grad_sync = lambda seg, lo, hi: seen.append(seg)
    a._grad_sync_points = {nseg // 2}
    try:
        out_s, gs = E.step(a, data, target)
    finally:
        a._grad_sync = a._grad_sync_points = None
    assert seen == list(range(nseg)) and E.same_bits(out_s, out_r) and E.same_bits(out_r, out_a2)
    for k in ga:
        assert E.same_bits(gs[k], gr[k]), f"{k}: segmented backward"

    # a second context of another batch shape continues the same u, v; an eval forward leaves them alone
    before = a.spectral_state()
    d3, t3 = _batch(index=1, n=3)
    a.eval()
    with torch.no_grad():
        a(d3.cuda())
    torch.cuda.synchronize()
    mid = a.spectral_state()
    assert all(torch.equal(before[k][0], mid[k][0]) and torch.equal(before[k][1], mid[k][1]) for k in before), "eval: no iteration"
    E.step(a, d3, t3)
    after = a.spectral_state()
    u3 = a.debug_tensor((3, S, S), "conv1.sn_u").cpu().numpy()
    assert np.array_equal(u3, after["conv1"][0].cpu().numpy()) and not torch.equal(after["conv1"][0], before["conv1"][0])
    ref, bound = SN.u_stage64(_rows(pa["conv1.weight"]), SN.v_from_torch(before["conv1"][1].cpu().numpy(), 7, 3))
    assert SN.worst(u3, ref, bound) <= 1.0, "the new context iterated from the state the first one left"

    # the library's mutual exclusion, on a live context
    from sota_imagenet_amd import native

    L, ctx = native.lib(), a._ctx(N, S, S)
    assert L.mi355_resnet50_set_weight_transform(ctx, 1) == -1 and "exclude" in native.last_error()
    with pytest.raises(RuntimeError):
        a.set_weight_transform("centre")
    assert a.weight_transform == 0

    # off again: the plain model's bits on the raw weights
    a.set_spectral_norm(False)
    assert not a.spectral_norm
    c = _model(dtype).cuda()
    out_off, g_off = E.step(a, data, target)
    out_c, g_c = E.step(c, data, target)
    assert E.same_bits(out_off, out_c) and all(E.same_bits(g_off[k], g_c[k]) for k in g_c)
    ws = _model(dtype, weight_standardization=True).cuda()
    ctx = ws._ctx(N, S, S)
    p = a.flat_params.data_ptr()
    assert L.mi355_resnet50_set_spectral_norm(ctx, 1, p, p) == -1 and "exclude" in native.last_error()


# ---- 6. against the oracle ---------------------------------------------------------------------------------------------------------------------
def test_fp32_step_matches_the_torch_spectral_norm_oracle(dev):
    """one fp32 training step at N=8 (at N=2 the gradient rule is batch luck: tests/test_weight_std_gpu.py) against oracle.resnet50_ref with
    torch's spectral_norm on every Conv2d; the native model is teacher-forced with the float32 oracle's _u, _v after registration, and so is
    the float64 oracle"""
    import weight_std_common as WS
    from sota_imagenet_amd.synth import synthetic_batch

    m = _model("fp32")
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    data, target = synthetic_batch(8, S, num_classes=NC, seed=0, index=3)
    torch.manual_seed(0)
    reg = SN.sn_oracle(sd, NC, double=False)
    state = {name: (mod.parametrizations.weight[0]._u.detach().clone(), mod.parametrizations.weight[0]._v.detach().clone().reshape(mod.weight.shape[1:]))
             for name, mod in reg.named_modules() if isinstance(mod, torch.nn.Conv2d)}
    o32, g32, s32 = SN.oracle_step(sd, data, target, NC, False, state)
    o64, g64, s64 = SN.oracle_step(sd, data, target, NC, True, state)
    m.set_spectral_norm(True)
    m.load_spectral_state(state)
    out, g = E.step(m, data, target)
    names = [k for k, _ in m.named_parameters()]
    assert set(names) == set(g64)
    e32, e64 = E.nerr(out, o32), E.nerr(out, o64)
    yard = E.l2err(WS.flat_grads(names, g32), WS.flat_grads(names, g64))
    got = E.l2err(WS.flat_grads(names, g), WS.flat_grads(names, g64))
    print(f"logits vs fp32 {e32:.3e}, vs fp64 {e64:.3e}; grad rel-L2 vs fp64: native {got:.3e}, torch-cpu fp32 {yard:.3e}")
    assert e32 < 1e-3 and e64 < 1e-3
    assert got < 1.5 * yard + 1e-3, f"grad rel-L2 vs fp64: native {got:.3e}, torch-cpu fp32 {yard:.3e}"
    after = m.spectral_state()
    wu = wv = 0.0
    for k in after:
        for j, worst in ((0, "u"), (1, "v")):
            ref = s64[k][j].reshape(-1).numpy()
            dn, d32 = _dist(after[k][j].reshape(-1).cpu().numpy(), ref), _dist(s32[k][j].reshape(-1).numpy(), ref)
            assert dn <= 2 * d32 + SN.U1, (k, worst, dn, d32)
            wu, wv = (max(wu, dn), wv) if j == 0 else (wu, max(wv, dn))
    print(f"u, v after the step: worst distance to torch-fp64 {wu:.2e}, {wv:.2e}")
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items() if k.endswith("conv1.weight")), "state_dict() keeps the raw weights"


# ---- 7. the callback ---------------------------------------------------------------------------------------------------------------------------
def test_forward_spectral_norm_callback(dev):
    from sota_imagenet_amd.callbacks import ForwardSpectralNorm, ForwardWeightNorm
    from sota_imagenet_amd.fit_wrapper import RunnerState
    from sota_imagenet_amd.optim import SGD

    m = _model("bf16").cuda()
    opt = SGD([{"params": list(m.parameters())}], lr=0.05, momentum=0.9, weight_decay=3e-5)
    opt.attach_model(m)
    cb = ForwardSpectralNorm()
    cb.set_state(RunnerState(model=m, optimizer=opt))
    cb.on_begin()
    assert m.spectral_norm and m.weight_transform == 0
    warmed = m.spectral_state()
    cb.on_begin()
    again = m.spectral_state()
    assert all(torch.equal(warmed[k][0], again[k][0]) and torch.equal(warmed[k][1], again[k][1]) for k in warmed), "a warmed state is left alone"
    other = ForwardWeightNorm()
    other.set_state(RunnerState(model=m, optimizer=opt))
    with pytest.raises(RuntimeError):
        other.on_begin()
    data, target = _batch(index=2)
    E.step(m, data, target)
    opt.step()
    torch.cuda.synchronize()
    stepped = {k: p.detach().clone() for k, p in m.named_parameters()}
    m.eval()
    with torch.no_grad():
        before = m(data.cuda()).clone()
    convs = E.conv_names(m)
    sigma = {k: m.debug_tensor((N, S, S), k[: -len(".weight")] + ".sn_sigma").item() for k in convs}
    cb.on_end()
    assert not m.spectral_norm
    with torch.no_grad():
        after = m(data.cuda()).clone()
    torch.cuda.synchronize()
    assert E.same_bits(before, after), "on_end leaves w / sigma behind: the same forward"
    for k, p in m.named_parameters():
        if p.dim() != 4:
            assert E.same_bits(p.detach(), stepped[k]), k
            continue
        ref = _rows(stepped[k]).astype(np.float64) / sigma[k]
        assert SN.worst(_rows(p), ref, 2 * SN.U1 * np.abs(ref)) <= 1.0, k
    cb.on_end()  # nothing to leave behind any more
    f8 = _model("fp8").cuda()
    cb.set_state(RunnerState(model=f8))
    with pytest.raises(ValueError):
        cb.on_begin()


def test_three_steps_of_the_smoke_config(dev):
    """Runner.fit on the synthetic loader with the callbacks of configs/hydra_exp/sn_test.yaml in its order"""
    from sota_imagenet_amd import callbacks, config as C
    from sota_imagenet_amd.data import SyntheticLoader
    from sota_imagenet_amd.fit_wrapper import Callback, Runner
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.optim import SGD

    cfg = C.to_plain(C.compose(None, ["+hydra_exp=sn_test"]))
    cbs = [C.call(e) for e in cfg["run"]["extra_callbacks"] if e["_target_"].startswith("src.callbacks.")]
    assert [type(c) for c in cbs] == [callbacks.OrthoInitClb, callbacks.ForwardSpectralNorm]
    m = _model("bf16").cuda()
    opt = SGD([{"params": list(m.parameters())}], lr=0.01, momentum=0.9, weight_decay=3e-5)
    opt.attach_model(m)
    seen = {}

    class Spy(Callback):
        def on_batch_end(self):
            seen.setdefault("u", []).append(m.spectral_u.clone())
            seen.setdefault("loss", []).append(float(self.state.loss_meter.val))
            seen["raw"] = all(k in m.state_dict() for k in ("conv1.weight", "layer4.2.conv3.weight")) and not any("parametrizations" in k for k in m.state_dict())
            seen["same"] = m.state_dict()["conv1.weight"].data_ptr() == dict(m.named_parameters())["conv1.weight"].data_ptr()

    r = Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=cbs + [Spy()])
    r.fit(SyntheticLoader(dict(batch_size=4, image_size=64, num_classes=NC), size=12, seed=0, device="cuda", pool=2), steps_per_epoch=3, epochs=1)
    torch.cuda.synchronize()
    assert len(seen["loss"]) == 3 and all(np.isfinite(x) for x in seen["loss"])
    assert not torch.equal(seen["u"][0], seen["u"][2]), "u advances with the training forwards"
    assert seen["raw"] and seen["same"], "state_dict() holds the raw conv weights under torchvision names"
    assert not m.spectral_norm, "on_end has baked and switched off"
