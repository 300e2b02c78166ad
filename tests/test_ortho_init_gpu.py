"""Orthogonal initialisation on the MI355X: the kernel of csrc/init_ortho.hip against an fp64 QR on the CPU, its status paths, the OrthoInitClb
callback on both flat-array models, and recipe 53's smoke config through the Runner.

The reference is Q64, the Q of torch.linalg.qr in float64 on the CPU with the signs of diag R folded in (what torch.nn.init.orthogonal_ computes,
sota_imagenet/callbacks.py:263), taken of the logical matrix, transposed when rows < cols.  The yardstick is the same computation in float32 on
the CPU (Q32), never anything computed by the code under test:
    max|Qdev - Q64|        <= 2 * max|Q32 - Q64|          + 2^-22
    max|Qdev^T Qdev - I|   <= 2 * max|Q32^T Q32 - I|      + 2^-22      (both formed in float64)
The factor 2 covers a different summation order; the floor is four roundings of an entry near 1, for the well-conditioned cases where both errors
are at rounding level."""
import math
import os
import sys

import pytest
import torch

from plan_common import layout as _layout

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -22
SENTINEL = 0x7FC0DEAD  # a NaN bit pattern: a gap that is read poisons what reads it

# (rows, chans, taps, rows of the tensor in memory): the last case is an FC weight of 10 rows followed by 6 zero padding rows
CASES = [(8, 4, 9, 8), (64, 3, 49, 64), (64, 64, 1, 64), (256, 64, 1, 256), (130, 127, 1, 130), (32, 3, 9, 32), (1, 16, 1, 1), (16, 1, 1, 16),
         (300, 40, 9, 300), (520, 260, 1, 520), (10, 32, 1, 16)]


# ---- the matrices of a flat array, and the reference -----------------------------------------------------------------------------------------------
def logical(flat, rec):
    """the logical rows x cols matrix of a record: M[r][ci*taps + t] = flat[off + r*cols + t*chans + ci]"""
    off, rows, chans, taps = rec
    return flat[off:off + rows * chans * taps].view(rows, taps, chans).permute(0, 2, 1).reshape(rows, chans * taps)


def to_memory(M, chans, taps):
    """the memory image of a logical matrix"""
    return M.view(M.shape[0], chans, taps).permute(0, 2, 1).reshape(-1)


def oriented(M):
    """the matrix whose COLUMNS are the vectors: the transpose when rows < cols"""
    return M.t() if M.shape[0] < M.shape[1] else M


def qr_fixed(X):
    Q, R = torch.linalg.qr(X)
    return Q * torch.sign(torch.diagonal(R)).unsqueeze(0)


def defect(Qx):
    Qd = Qx.double()
    return (Qd.t() @ Qd - torch.eye(Qd.shape[1], dtype=torch.float64)).abs().max().item()


def errors(Qx, Q64):
    return (Qx.double() - Q64).abs().max().item(), defect(Qx)


def _records(offs):
    return [(o, r, c, t) for o, (r, c, t, _) in zip(offs, CASES)]


def _launch(flat, recs, gain=1.0):
    from sota_imagenet_amd import item_plan, ops

    st = ops.ortho_init_(flat, recs, item_plan.pack_records(recs, flat.device, item_plan.ORTHO_FIELDS), gain)
    torch.cuda.synchronize()
    return st


def run_cases(dev):
    """ONE launch over all cases, and the references (tools/ortho_init_measure.py records the same figures)"""
    sizes = [mem_rows * c * t for _, c, t, mem_rows in CASES]
    offs, n = _layout(sizes)
    recs = _records(offs)
    host = torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32).clone()
    gauss = []
    for i, ((rows, chans, taps, mem_rows), off) in enumerate(zip(CASES, offs)):
        A = torch.randn(rows, chans * taps, generator=torch.Generator().manual_seed(100 + i))
        gauss.append(A)
        host[off:off + sizes[i]] = 0.0
        host[off:off + rows * chans * taps] = to_memory(A, chans, taps)
    flat = host.to(dev)
    status = _launch(flat, recs)
    refs = []
    for A in gauss:
        Q64 = qr_fixed(oriented(A).double())
        refs.append((Q64, errors(qr_fixed(oriented(A).clone()), Q64)))
    return dict(host=host, out=flat.cpu(), status=status.cpu(), recs=recs, refs=refs, n=n, offs=offs, sizes=sizes)


@pytest.fixture(scope="module")
def kernel_run(dev):
    """computed once, shared by the tests below, which leave it unchanged"""
    return run_cases(dev)


# ---- 1. the kernel against fp64 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=[f"{r}x{c}x{t}" for r, c, t, _ in CASES])
def test_kernel_against_fp64_qr(kernel_run, i):
    k = kernel_run
    assert k["status"].tolist() == [0] * len(CASES)
    Q64, (d32, o32) = k["refs"][i]
    ddev, odev = errors(oriented(logical(k["out"], k["recs"][i])), Q64)
    print(f"case {CASES[i][:3]}: device |Q - Q64| {ddev:.3e}, |QtQ - I| {odev:.3e}; float32 QR {d32:.3e}, {o32:.3e}")
    assert ddev <= 2 * d32 + FLOOR
    assert odev <= 2 * o32 + FLOOR


def test_gaps_and_padding_keep_their_bits(kernel_run):
    k = kernel_run
    mask = torch.ones(k["n"], dtype=torch.bool)
    for off, rows, chans, taps in k["recs"]:
        mask[off:off + rows * chans * taps] = False
    before, after = k["host"].view(torch.int32), k["out"].view(torch.int32)
    assert torch.equal(before[mask], after[mask])
    assert (before[mask] == SENTINEL).sum().item() == mask.sum().item() - 6 * 32  # the sentinel everywhere but in the FC case's padding rows ...
    off = k["offs"][-1]
    assert (k["out"][off + 10 * 32:off + 16 * 32] == 0).all()  # ... which are zero, as they were
    assert torch.isfinite(k["out"][~mask]).all() and not torch.equal(before[~mask], after[~mask])


def test_a_second_run_gives_the_same_bits_and_gain_is_one_multiply(kernel_run, dev):
    k = kernel_run
    again = k["host"].to(dev)
    assert _launch(again, k["recs"]).tolist() == [0] * len(CASES)
    assert torch.equal(again.cpu().view(torch.int32), k["out"].view(torch.int32))
    scaled = k["host"].to(dev)
    assert _launch(scaled, k["recs"], gain=1.7).tolist() == [0] * len(CASES)
    scaled, g = scaled.cpu(), torch.tensor(1.7, dtype=torch.float32)
    for off, rows, chans, taps in k["recs"]:
        sl = slice(off, off + rows * chans * taps)
        assert torch.equal(scaled[sl], k["out"][sl] * g)
    mask = torch.ones(k["n"], dtype=torch.bool)
    for off, rows, chans, taps in k["recs"]:
        mask[off:off + rows * chans * taps] = False
    assert torch.equal(scaled.view(torch.int32)[mask], k["host"].view(torch.int32)[mask])


# ---- 2. status paths ------------------------------------------------------------------------------------------------------------------------------
def test_status_paths_leave_the_neighbour_alone(dev):
    """a rank-deficient matrix (status 1, finite contents) and a record reaching past the array (status 2, memory untouched) in one launch with
    a valid record, which comes out right.  Every access is behind the record check: nothing here can fault."""
    n = 1024
    host = torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32).clone()
    g = torch.Generator().manual_seed(7)
    bad = torch.randn(6, 16, generator=g)
    bad[4] = bad[1]  # two equal rows
    good = torch.randn(24, 8, generator=g)
    host[0:96], host[128:320] = bad.reshape(-1), good.reshape(-1)
    recs = [(0, 6, 16, 1), (128, 24, 8, 1), (n - 10, 4, 8, 1), (512, 0, 8, 1), (-64, 4, 8, 1)]
    flat = host.to(dev)
    assert _launch(flat, recs).tolist() == [1, 0, 2, 2, 2]
    out = flat.cpu()
    assert torch.isfinite(out[0:96]).all()
    Q64 = qr_fixed(good.double())
    d32, o32 = errors(qr_fixed(good.clone()), Q64)
    ddev, odev = errors(out[128:320].view(24, 8), Q64)
    assert ddev <= 2 * d32 + FLOOR and odev <= 2 * o32 + FLOOR
    assert torch.equal(out[96:128].view(torch.int32), host[96:128].view(torch.int32))
    assert torch.equal(out[320:].view(torch.int32), host[320:].view(torch.int32))  # the gaps, and everything the refused records name
    # the rows before the repeated one are orthonormal
    first = out[0:64].view(4, 16).double()
    assert (first @ first.t() - torch.eye(4, dtype=torch.float64)).abs().max().item() <= 2 * defect(qr_fixed(bad[:4].t().clone())) + FLOOR


def test_overlapping_records_are_refused_by_the_wrapper(dev):
    from sota_imagenet_amd import item_plan, ops

    flat = torch.zeros(256, device=dev)
    recs = [(0, 4, 16, 1), (32, 4, 8, 1)]
    with pytest.raises(ValueError, match="overlaps"):
        ops.ortho_init_(flat, recs, item_plan.pack_records(recs, dev, item_plan.ORTHO_FIELDS), 1.0)
    with pytest.raises(ValueError):  # a table that does not match the host records
        ops.ortho_init_(flat, recs[:1], item_plan.pack_records(recs, dev, item_plan.ORTHO_FIELDS), 1.0)
    assert (flat == 0).all()


# ---- 3. the callback on the models ----------------------------------------------------------------------------------------------------------------
def _resnet50():
    from sota_imagenet_amd.models import resnet50

    return resnet50(dtype="bf16").cuda()


def _bresnet50():
    from sota_imagenet_amd.models import resnet50

    return resnet50(stem_type="deep", antialias=True, attn_type="eca", norm_layer="inplaceabn", norm_act="leaky_relu", dtype="bf16").cuda()


def _begin(model, seed=0, start_epoch=None, gain=1):
    """on_begin of a fresh callback on `model` with a stub state; returns (callback, the flat array between fill and orthogonalise or None)"""
    from sota_imagenet_amd.callbacks import OrthoInitClb
    from sota_imagenet_amd.fit_wrapper import RunnerState

    cb = OrthoInitClb(gain)
    state = RunnerState(model=model)
    state.random_seed = seed
    if start_epoch is not None:
        state.start_epoch = start_epoch
    cb.set_state(state)
    snap, orth = [], cb.orthogonalise

    def spy():
        snap.append(model.flat_params.detach().clone())
        orth()

    cb.orthogonalise = spy
    cb.on_begin()
    torch.cuda.synchronize()
    return cb, (snap[0].cpu() if snap else None)


def _initialised(make):
    m = make()
    before = (m.flat_params.detach().cpu().clone(), m._flat_buffers.detach().cpu().clone())
    cb, gauss = _begin(m, seed=3)
    return dict(model=m, cb=cb, before=before, gauss=gauss, after=m.flat_params.detach().cpu().clone())


@pytest.fixture(scope="module")
def r50(dev):
    return _initialised(_resnet50)


@pytest.fixture(scope="module")
def br50(dev):
    return _initialised(_bresnet50)


def _check_model(run, n_records):
    m, cb = run["model"], run["cb"]
    assert cb.has_been_init and len(cb.records) == n_records == len(cb.names) and cb.status.tolist() == [0] * n_records
    planned = torch.zeros(m._nparam, dtype=torch.bool)
    worst = (0.0, None)
    params = dict(m.named_parameters())
    for name, rec in zip(cb.names, cb.records):
        off, rows, chans, taps = rec
        planned[off:off + rows * chans * taps] = True
        p = params[name]
        assert tuple(p.shape)[:2] == (rows, chans) and p.numel() == rows * chans * taps
        assert torch.equal(p.detach().cpu().reshape(rows, -1), logical(run["after"], rec))  # the record is the parameter's logical matrix
        A = oriented(logical(run["gauss"], rec))
        odev, o32 = defect(oriented(logical(run["after"], rec))), defect(qr_fixed(A.clone()))
        assert odev <= 2 * o32 + FLOOR, (name, odev, o32)
        worst = max(worst, (odev, name))
        assert torch.isfinite(A).all() and 0.5 < A.std().item() < 1.5  # the snapshot is a Gaussian matrix: finite, of unit scale
    print(f"{type(m).__name__}: {n_records} matrices, largest |QtQ - I| {worst[0]:.3e} ({worst[1]})")
    # every other element of the flat parameter array and all buffers: the bits they had
    p0, b0 = run["before"]
    assert torch.equal(run["after"].view(torch.int32)[~planned], p0.view(torch.int32)[~planned])
    assert torch.equal(run["gauss"].view(torch.int32)[~planned], p0.view(torch.int32)[~planned])  # the fill stays inside the plan as well
    assert torch.equal(m._flat_buffers.detach().cpu().view(torch.int32), b0.view(torch.int32))
    assert not torch.equal(run["after"][planned], p0[planned])
    return planned


def test_resnet50_weights_are_orthogonal_and_nothing_else_moved(r50):
    m = r50["model"]
    planned = _check_model(r50, 54)
    # by name: BatchNorm weights and biases, fc.bias and the FC padding rows are among the untouched
    table = {name: (off, shape) for name, kind, off, shape in m._table if kind == 0}
    for name in ("bn1.weight", "bn1.bias", "layer4.2.bn3.weight", "fc.bias"):
        off, shape = table[name]
        assert not planned[off:off + math.prod(shape)].any()
    off, shape = table["fc.weight"]
    assert shape == (1000, 2048) and not planned[off + 1000 * 2048:off + 1024 * 2048].any()
    assert (r50["after"][off + 1000 * 2048:off + 1024 * 2048] == 0).all()
    assert torch.isfinite(r50["after"]).all()


def test_a_second_on_begin_changes_nothing(r50):
    m, cb = r50["model"], r50["cb"]
    cb.on_begin()
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params.detach().cpu().view(torch.int32), r50["after"].view(torch.int32))


def test_same_seed_same_bits_another_seed_not(r50):
    m2 = _resnet50()
    _begin(m2, seed=3)
    assert torch.equal(m2.flat_params.detach().cpu().view(torch.int32), r50["after"].view(torch.int32))
    _, gauss = _begin(m2, seed=4)
    assert gauss is not None and not torch.equal(m2.flat_params.detach().cpu(), r50["after"])


def test_a_fit_that_starts_later_keeps_the_weights_and_gain_scales(dev):
    m = _resnet50()
    before = m.flat_params.detach().clone()
    cb, gauss = _begin(m, seed=3, start_epoch=1)
    assert gauss is None and cb.has_been_init and torch.equal(m.flat_params.detach(), before)
    cb.on_begin()  # and stays skipped
    assert torch.equal(m.flat_params.detach(), before)
    _begin(m, seed=3, start_epoch=0)
    one = m.flat_params.detach().clone()
    cb2, _ = _begin(m, seed=3, gain=1.7)
    off, rows, chans, taps = cb2.records[0]
    sl = slice(off, off + rows * chans * taps)
    assert torch.equal(m.flat_params.detach()[sl], one[sl] * torch.tensor(1.7, dtype=torch.float32, device=dev))


def test_a_rank_deficient_weight_raises_through_the_callback(dev):
    from sota_imagenet_amd.callbacks import OrthoInitClb
    from sota_imagenet_amd.fit_wrapper import RunnerState

    m = _resnet50()
    cb = OrthoInitClb()
    cb.set_state(RunnerState(model=m))
    cb.fill()
    with torch.no_grad():
        m.conv1.weight[5].copy_(m.conv1.weight[2])
    with pytest.raises(RuntimeError, match=r"conv1\.weight"):
        cb.orthogonalise()
    assert torch.isfinite(m.flat_params).all()


def test_bresnet50_weights_are_orthogonal_and_the_eca_weights_are_untouched(br50):
    m = br50["model"]
    n_records = sum(kind == 0 and len(shape) in (2, 4) for _, kind, _, shape in m._table)
    planned = _check_model(br50, n_records)
    eca = [(off, shape) for _, kind, off, shape in m._table if kind == 0 and len(shape) == 3]
    assert eca and all(not planned[off:off + math.prod(shape)].any() for off, shape in eca)
    assert (32, 3, 9) in [r[1:] for r in br50["cb"].records]  # the deep stem's tall 32 x 27 matrix went through
    assert torch.isfinite(br50["after"]).all()


# ---- 4. through the Runner ------------------------------------------------------------------------------------------------------------------------
def test_recipe_53_smoke_config_through_the_runner(dev):
    """adamw_rep_test at the smallest legal shape (bs 8, 32 px), two training steps: conv1.weight, viewed as 64 x 147, has orthonormal rows before
    step 1 and the loss is finite after both steps"""
    sys.path.insert(0, ROOT)
    from sota_imagenet_amd import callbacks, config as C, fit_wrapper as fw, optim
    from sota_imagenet_amd.synth import synthetic_batch

    cfg = C.compose(None, ["+hydra_exp=adamw_rep_test"])
    model_cfg = dict(C.to_plain(cfg.model), dtype="bf16")
    m = C.call(model_cfg)
    m.reset_parameters(seed=0, gamma=cfg.init_gamma)
    m = m.cuda()
    opt = C.call(cfg.optim, [{"params": list(m.parameters())}])
    assert type(opt) is optim.AdamW
    seen, losses = [], []

    class Spy(fw.Callback):
        def on_batch_begin(self):
            if self.state.step == 0:
                seen.append(m.conv1.weight.detach().reshape(64, 147).double().cpu())

        def on_batch_end(self):
            losses.append(float(self.state.loss_meter.avg))

    made = [C.call(cb) for cb in cfg.run.extra_callbacks]
    assert type(made[0]) is callbacks.OrthoInitClb
    gauss, orth = [], made[0].orthogonalise

    def spy():  # the Gaussian conv1.weight between fill and orthogonalise: the yardstick's input
        gauss.append(m.conv1.weight.detach().reshape(64, 147).cpu())
        orth()

    made[0].orthogonalise = spy
    lr = fw.PhasesScheduler([dict(ep=(0, 1), lr=(1e-4, 2e-3))])

    class Loader:
        batch_size = 8

        def __len__(self):
            return 2

        def __iter__(self):
            return iter([synthetic_batch(8, 32, seed=1, index=i, device="cuda") for i in range(2)])

    runner = fw.Runner(m, opt, C.call(cfg.criterion).cuda(), callbacks=[lr] + made + [Spy()])
    runner.state.random_seed = 0
    runner.fit(Loader(), epochs=1)
    torch.cuda.synchronize()
    assert made[0].has_been_init and runner.state.start_epoch == 0
    W = seen[0]
    assert len(gauss) == 1 and (W @ W.t() - torch.eye(64, dtype=torch.float64)).abs().max().item() <= 2 * defect(qr_fixed(gauss[0].t().clone())) + FLOOR
    assert len(losses) == 2 and all(math.isfinite(x) for x in losses)
    assert torch.isfinite(m.flat_params).all()
