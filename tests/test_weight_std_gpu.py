"""The per-filter forward weight transform on the GPU: the row kernels of csrc/weight_std.hip against float64 on synthetic rows, the executor's
wiring against a plain model fed the transformed weights, the whole step against the parametrised torch oracle, and the ForwardWeightNorm callback.
The bounds are those of tests/weight_std_common.py; the model tests run at N=2, 64 px, 10 classes."""
import functools

import numpy as np
import pytest
import torch

import exec_gpu_common as E
import weight_std_common as WS

pytestmark = pytest.mark.gpu
N, S, NC = 2, 64, 10
_model = functools.partial(E.model, num_classes=NC)
MODE_IDS = sorted(WS.MODES)


@pytest.fixture(scope="module")
def rows_case():
    flat, rows, const = WS.make_rows()
    return flat, rows, const, WS.row_mask(flat.size, rows)


def _forward_rows(flat, rows, mode, dev):
    ops, item_plan = E.mods()
    w = torch.from_numpy(flat).to(dev)
    w_hat = torch.full_like(w, float("nan"))
    invstd = torch.full((len(rows),), float("nan"), device=dev)
    ops.weight_std_rows_fwd(w, w_hat, invstd, item_plan.pack_records(rows, dev), mode)
    torch.cuda.synchronize()
    return w, w_hat, invstd


# ---- 1. rows, forward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", MODE_IDS)
def test_rows_forward_against_float64(dev, rows_case, mode_name):
    flat, rows, const, mask = rows_case
    mode = WS.MODES[mode_name]
    w, w_hat, invstd = _forward_rows(flat, rows, mode, dev)
    got, inv = w_hat.cpu().numpy(), invstd.cpu().numpy()
    assert np.array_equal(w.cpu().numpy().view(np.int32), flat.view(np.int32)), "the source is read only"
    assert np.isnan(got[~mask]).all(), "gaps are neither read into a row nor written"
    assert np.isfinite(got[mask]).all() and np.isfinite(inv).all()
    for k, (o, L) in enumerate(rows):
        mu, is64, ref = WS.fwd64(flat[o: o + L], mode)
        r = WS.worst(got[o: o + L], ref, WS.fwd_bound(mu, is64, ref))
        rel = abs(float(inv[k]) - is64) / is64
        print(f"{mode_name} row {k} L={L}: worst error / bound {r:.3f}, invstd rel {rel:.2e}")
        assert r <= 1.0, (k, L, r)
        assert rel <= 2.0 ** -23, (k, L, rel)
    o, L = rows[const]
    assert (got[o: o + L] == 0).all(), "a constant row gives zeros"
    if mode == WS.CENTRE:
        assert (inv == 1.0).all()
    # bit for bit on a second run, and in place (the bake): the same bits as out of place, gaps untouched
    _, again, inv2 = _forward_rows(flat, rows, mode, dev)
    assert E.same_bits(again[torch.from_numpy(mask).to(dev)], w_hat[torch.from_numpy(mask).to(dev)]) and E.same_bits(inv2, invstd)
    ops, item_plan = E.mods()
    inplace = torch.from_numpy(flat).to(dev)
    ops.weight_std_rows_fwd(inplace, inplace, inv2, item_plan.pack_records(rows, dev), mode)
    torch.cuda.synchronize()
    ip = inplace.cpu().numpy()
    assert np.array_equal(ip[mask].view(np.int32), got[mask].view(np.int32)) and np.isnan(ip[~mask]).all()


def test_rows_that_do_not_fit_are_skipped(dev, rows_case):
    flat, rows, _, mask = rows_case
    ops, item_plan = E.mods()
    n = flat.size
    bad = [(-1, 64), (n - 10, 64), (0, 0), (n, 1), (5, n + 1)]
    w = torch.from_numpy(flat).to(dev)
    w_hat = torch.full_like(w, float("nan"))
    invstd = torch.full((len(bad) + 1,), -7.0, device=dev)
    ops.weight_std_rows_fwd(w, w_hat, invstd, item_plan.pack_records(bad + [rows[3]], dev), WS.STANDARDISE)
    dw = torch.full_like(w, 3.0)
    ops.weight_std_rows_bwd(w, w_hat, invstd, dw, item_plan.pack_records(bad + [rows[3]], dev), WS.STANDARDISE, beta=1.0)
    torch.cuda.synchronize()
    o, L = rows[3]
    keep = np.ones(n, dtype=bool)
    keep[o: o + L] = False
    assert np.isnan(w_hat.cpu().numpy()[keep]).all() and np.isfinite(w_hat.cpu().numpy()[~keep]).all()
    assert (invstd.cpu().numpy()[:-1] == -7.0).all() and invstd[-1].item() > 0
    assert (dw.cpu().numpy()[keep] == 3.0).all()


# ---- 2. rows, backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("mode_name", MODE_IDS)
def test_rows_backward_against_float64(dev, rows_case, mode_name, beta):
    flat, rows, _, mask = rows_case
    mode = WS.MODES[mode_name]
    ops, item_plan = E.mods()
    _, w_hat, invstd = _forward_rows(flat, rows, mode, dev)
    rng = np.random.default_rng(7)
    g = np.full(flat.size, np.nan, dtype=np.float32)
    old = np.full(flat.size, np.nan, dtype=np.float32)
    for k, (o, L) in enumerate(rows):
        g[o: o + L] = ((0.3 if k % 2 else -0.01) + 10.0 ** (-(k % 4)) * rng.standard_normal(L)).astype(np.float32)
        old[o: o + L] = (1.0 + rng.standard_normal(L)).astype(np.float32)
    tab = item_plan.pack_records(rows, dev)
    gd = torch.from_numpy(g).to(dev)
    dw = torch.from_numpy(old).to(dev)
    ops.weight_std_rows_bwd(gd, w_hat, invstd, dw, tab, mode, beta=beta)
    # a slice of the table: only its rows are written
    dw_slice = torch.from_numpy(old).to(dev)
    ops.weight_std_rows_bwd(gd, w_hat, invstd, dw_slice, tab, mode, beta=beta, row_begin=2, row_end=7)
    torch.cuda.synchronize()
    got, wh, inv = dw.cpu().numpy(), w_hat.cpu().numpy(), invstd.cpu().numpy()
    assert np.isnan(got[~mask]).all(), "gaps are untouched"
    for k, (o, L) in enumerate(rows):
        ref, bound = WS.bwd64(g[o: o + L], wh[o: o + L], inv[k], mode)
        if beta:
            prev = old[o: o + L].astype(np.float64)
            ref, bound = beta * prev + ref, bound + WS.U * np.abs(beta * prev)
        r = WS.worst(got[o: o + L], ref, bound)
        print(f"{mode_name} beta={beta} row {k} L={L}: worst error / bound {r:.3f}")
        assert r <= 1.0, (k, L, r)
        part = dw_slice.cpu().numpy()[o: o + L]
        want = got[o: o + L] if 2 <= k < 7 else old[o: o + L]
        assert np.array_equal(part.view(np.int32), want.view(np.int32)), k
    again = torch.from_numpy(old).to(dev)
    ops.weight_std_rows_bwd(gd, w_hat, invstd, again, tab, mode, beta=beta)
    torch.cuda.synchronize()
    m = torch.from_numpy(mask).to(dev)
    assert E.same_bits(again[m], dw[m])


# ---- the recorded bits ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded(dev):
    """tests/golden/row_kernels_bits.npz (make_row_kernels_golden.py) and what the same calls give on its stored inputs, computed once"""
    import row_bits_common as R

    z = np.load(R.FIXTURE)
    recs = [tuple(int(v) for v in r) for r in z["records"]]
    assert recs == R.layout()[0] and tuple(z["bwd_slice"]) == R.BWD_SLICE
    return R, z, recs, R.run_weight_std(recs, z["w"].copy(), z["g"].copy(), z["dw_old"].copy(), dev)


@pytest.mark.parametrize("mode_name", MODE_IDS)
def test_rows_forward_gives_the_recorded_bits(recorded, mode_name):
    """rows shorter than the scalar head, every head and tail, one lane short of a wave and one past: a difference means the arithmetic or the
    order of a sum has changed.  Out of place into sentinels and in place give the same array, gaps included."""
    R, z, recs, got = recorded
    mode = WS.MODES[mode_name]
    want, inv = z[f"fwd/{mode}/w_hat"], z[f"fwd/{mode}/invstd"]
    mask = R.row_mask(want.size, R.rows_of(recs))
    assert (want.view(np.int32)[~mask] == R.SENTINEL).all() and np.isfinite(want[mask]).all()
    for name in (f"fwd/{mode}/w_hat", f"fwd/{mode}/in_place"):
        assert np.array_equal(np.isnan(got[name]), ~mask) and (got[name].view(np.int32)[~mask] == R.SENTINEL).all(), name
        assert R.same_bits(got[name], want), name
    assert R.same_bits(got[f"fwd/{mode}/invstd"], inv) and R.same_bits(got[f"fwd/{mode}/in_place_invstd"], inv)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("mode_name", MODE_IDS)
def test_rows_backward_gives_the_recorded_bits(recorded, mode_name, beta):
    """a slice that starts and ends inside a group of four rows; with beta == 0 dw starts as NaN, which is never read"""
    R, z, recs, got = recorded
    mode = WS.MODES[mode_name]
    want, have = z[f"bwd/{mode}/{beta}/dw"], got[f"bwd/{mode}/{beta}/dw"]
    rows = R.rows_of(recs)
    sl = R.row_mask(want.size, rows[R.BWD_SLICE[0]: R.BWD_SLICE[1]])
    assert np.isfinite(want[sl]).all() and np.isfinite(have[sl]).all()
    outside = z["dw_old"][~sl] if beta else np.full(int((~sl).sum()), np.nan, dtype=np.float32)
    assert R.same_bits(want[~sl], outside) and R.same_bits(have[~sl], outside), "rows outside the slice and the gaps keep their bits"
    assert R.same_bits(have, want)


# ---- the model tests -----------------------------------------------------------------------------------------------------------------------------
def _batch(index=0):
    from sota_imagenet_amd.synth import synthetic_batch

    return synthetic_batch(N, S, num_classes=NC, seed=3, index=index)


# ---- 3. the executor wiring, exactly -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_name", MODE_IDS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_executor_wiring_is_exact(dev, dtype, mode_name):
    mode = WS.MODES[mode_name]
    data, target = _batch()
    a = _model(dtype).cuda()
    a.set_weight_transform(mode_name)
    out_a, ga = E.step(a, data, target)
    convs = E.conv_names(a)
    w_hat = {k: a.debug_tensor((N, S, S), k[: -len(".weight")] + ".w_hat") for k in convs}       # [Cout, K, K, Cin]
    invstd = {k: a.debug_tensor((N, S, S), k[: -len(".weight")] + ".ws_invstd") for k in convs}  # [Cout]

    # the transform itself, on the model's own weights (the stem's 147-element rows at the offsets the layout gives them)
    pa = dict(a.named_parameters())
    for k in ("conv1.weight", "layer1.0.conv1.weight", "layer4.2.conv2.weight"):
        w = pa[k].detach().permute(0, 2, 3, 1).reshape(pa[k].shape[0], -1).cpu().numpy()
        got = w_hat[k].reshape(w.shape).cpu().numpy()
        for r in range(0, w.shape[0], 17):
            mu, is64, ref = WS.fwd64(w[r], mode)
            assert WS.worst(got[r], ref, WS.fwd_bound(mu, is64, ref)) <= 1.0, (k, r)

    # B: plain, its conv weights are A's w_hat
    b = _model(dtype).cuda()
    with torch.no_grad():
        for k, p in b.named_parameters():
            p.copy_(w_hat[k].permute(0, 3, 1, 2) if k in w_hat else pa[k])
    out_b, gb = E.step(b, data, target)
    assert E.same_bits(out_a, out_b), "the logits of A are those of a plain model on w_hat"
    for k in ga:
        if k not in w_hat:
            assert E.same_bits(ga[k], gb[k]), f"{k}: BatchNorm / FC gradients do not see the transform"
    worst = 0.0
    for k in convs:
        co = ga[k].shape[0]
        g = gb[k].permute(0, 2, 3, 1).reshape(co, -1).cpu().numpy()      # the gradient wrt w_hat, in memory order
        wh = w_hat[k].reshape(co, -1).cpu().numpy()
        got = ga[k].permute(0, 2, 3, 1).reshape(co, -1).cpu().numpy()
        inv = invstd[k].cpu().numpy()
        for r in range(co):
            ref, bound = WS.bwd64(g[r], wh[r], inv[r], mode)
            x = WS.worst(got[r], ref, bound)
            worst = max(worst, x)
            assert x <= 1.0, (k, r, x)
    print(f"{dtype} {mode_name}: conv gradients, worst error / bound {worst:.3f}")

    # accumulation: a second identical step without zero_grad leaves exactly twice the gradients
    _, g2 = E.step(a, data, target, zero=False)
    for k in ga:
        assert E.same_bits(g2[k], 2 * ga[k]), f"{k}: accumulated gradient"

    # the backward in two segment calls (what the DDP hook does) gives the bits of one call
    nseg = len(a.grad_segments)
    seen = []
    a._grad_sync = lambda seg, lo, hi: seen.append(seg)
    a._grad_sync_points = {nseg // 2}
    try:
        out_s, gs = E.step(a, data, target)
    finally:
        a._grad_sync = a._grad_sync_points = None
    assert seen == list(range(nseg))
    assert E.same_bits(out_s, out_a)
    for k in ga:
        assert E.same_bits(gs[k], ga[k]), f"{k}: segmented backward"

    # off again: the plain model's bits on the raw weights
    a.set_weight_transform("off")
    c = _model(dtype).cuda()
    out_off, g_off = E.step(a, data, target)
    out_c, g_c = E.step(c, data, target)
    assert E.same_bits(out_off, out_c) and all(E.same_bits(g_off[k], g_c[k]) for k in g_c)


# ---- 4. against the oracle ---------------------------------------------------------------------------------------------------------------------
def test_fp32_standardised_step_matches_the_parametrised_oracle(dev):
    """The rule of test_resnet_gpu.test_fp32_forward_backward_matches_cpu on that test's own batch (synthetic_batch seed 0, index 3), at N=2, 64 px,
    10 classes.  Both distances are samples of the same rounding noise, amplified by BatchNorm over as few as 8 values per channel, and at this
    shape they scatter from batch to batch and from host CPU to host CPU: on an MI355X box, native / torch-CPU fp32 rel-L2 distance to fp64 was
    5.9e-2 / 5.7e-2 on this batch and 1.0e-2 / 4.6e-3, 4.3e-2 / 2.0e-2, 5.3e-3 / 1.4e-2 on three others (the plain model without the transform:
    ratios 0.6 to 1.3 on the same four); at N=8 all four batches kept the rule (ratios 0.8 to 1.4).  The batch was fixed as the rule's own before
    these were measured; two of the three others would miss 1.5x at N=2."""
    m = _model("fp32", weight_standardization=True)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    assert m.weight_transform == WS.STANDARDISE
    from sota_imagenet_amd.synth import synthetic_batch

    data, target = synthetic_batch(N, S, num_classes=NC, seed=0, index=3)
    o32, g32 = WS.oracle_step(sd, data, target, WS.STANDARDISE, NC, double=False)
    o64, g64 = WS.oracle_step(sd, data, target, WS.STANDARDISE, NC, double=True)
    out, g = E.step(m, data, target)
    names = [k for k, _ in m.named_parameters()]
    assert set(names) == set(g64)
    e32, e64 = E.nerr(out, o32), E.nerr(out, o64)
    yard = E.l2err(WS.flat_grads(names, g32), WS.flat_grads(names, g64))
    got = E.l2err(WS.flat_grads(names, g), WS.flat_grads(names, g64))
    print(f"logits vs fp32 {e32:.3e}, vs fp64 {e64:.3e}; grad rel-L2 vs fp64: native {got:.3e}, torch-cpu fp32 {yard:.3e}")
    assert e32 < 1e-3 and e64 < 1e-3
    assert got < 1.5 * yard + 1e-3, f"grad rel-L2 vs fp64: native {got:.3e}, torch-cpu fp32 {yard:.3e}"
    # state_dict() keeps the raw weights
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items() if k.endswith("conv1.weight"))


# ---- 5. the callback ---------------------------------------------------------------------------------------------------------------------------
def test_forward_weight_norm_callback(dev):
    from sota_imagenet_amd.callbacks import ForwardWeightNorm
    from sota_imagenet_amd.fit_wrapper import RunnerState
    from sota_imagenet_amd.optim import SGD

    m = _model("bf16").cuda()
    opt = SGD([{"params": list(m.parameters())}], lr=0.05, momentum=0.9, weight_decay=3e-5)
    opt.attach_model(m)
    cb = ForwardWeightNorm()
    cb.set_state(RunnerState(model=m, optimizer=opt))
    cb.on_begin()
    assert m.weight_transform == WS.CENTRE
    data, target = _batch(index=2)
    E.step(m, data, target)
    opt.step()
    torch.cuda.synchronize()
    stepped = {k: p.detach().clone() for k, p in m.named_parameters()}
    m.eval()
    with torch.no_grad():
        before = m(data.cuda()).clone()
    cb.on_end()
    assert m.weight_transform == 0
    with torch.no_grad():
        after = m(data.cuda()).clone()
    torch.cuda.synchronize()
    assert E.same_bits(before, after), "on_end leaves the parametrised weights behind: the same forward"
    for k, p in m.named_parameters():
        if p.dim() != 4:
            assert E.same_bits(p.detach(), stepped[k]), k
            continue
        co = p.shape[0]
        w = stepped[k].permute(0, 2, 3, 1).reshape(co, -1).cpu().numpy()
        got = p.detach().permute(0, 2, 3, 1).reshape(co, -1).cpu().numpy()
        for r in range(co):
            mu, is64, ref = WS.fwd64(w[r], WS.CENTRE)
            assert WS.worst(got[r], ref, WS.fwd_bound(mu, is64, ref)) <= 1.0, (k, r)


# ---- 6. fp8 --------------------------------------------------------------------------------------------------------------------------------------
def test_fp8_model_refuses_a_weight_transform(dev):
    from sota_imagenet_amd import native

    m = _model("fp8").cuda()
    for mode in (1, 2, "standardise", "centre"):
        with pytest.raises(ValueError):
            m.set_weight_transform(mode)
    m.set_weight_transform(0)
    L = native.lib()
    c = m._ctx(N, S, S)
    for mode in (1, 2):
        assert L.mi355_resnet50_set_weight_transform(c, mode) == -1 and "fp8" in native.last_error()
    assert L.mi355_resnet50_set_weight_transform(c, 0) == 0
    f = _model("fp32").cuda()
    c = f._ctx(N, S, S)
    for mode in (-1, 3):
        assert L.mi355_resnet50_set_weight_transform(c, mode) == -1
    with pytest.raises(ValueError):
        f.set_weight_transform(3)
