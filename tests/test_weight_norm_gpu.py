"""Backward centred weight normalisation on the MI355X: the kernel of csrc/weight_norm.hip against the float64 restatement of the rule
(tests/weight_norm_common.py) on a synthetic flat array, its refusal of items that do not fit, the reference's recorded run, the WeightNorm
callback on both flat-array models through the Runner, and recipe 14's smoke config through train.py.

With u = 2^-24 and M, N, Y the float64 mean, centred norm and result of an fp32 input row (weight_norm_common.rule64):
    native bound      |y - Y| <= 8u|Y| + 4u|M| / N                                       (derived there; never tuned to the kernel)
    a second application y -> y': |y' - y| <= what the native bound implies (weight_norm_common.reapply_bound): the native bound of y taken as
        an input, plus the distance of y to its own exact image, which the first bound limits through y's mean and norm.
    of the rows y of a model after a step: |mean y| <= mean of the bound over the row, | ||y|| - 1 | <= the 2-norm of the bound over the row
        (y = Y + e with |e_i| <= bound_i, mean Y = 0, ||Y|| = 1)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import exec_gpu_common as E
import weight_norm_common as WN

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SENTINEL = 0x7FC0DEAD  # a NaN bit pattern: a gap that is read poisons what reads it


def _launch(flat, items):
    ops, item_plan = E.mods()
    st = ops.weight_norm_rows_(flat, items, item_plan.pack_records(items, flat.device))
    torch.cuda.synchronize()
    return st


def _shapes():
    """(skew of the first element against a 64-element boundary, rows, row_len)"""
    ops, _ = E.mods()
    T, W = ops.WNORM_WAVE_ROW_MAX, ops.WNORM_ITEM_ELEMS
    return [(3, 5, 147), (0, 4, 64), (1, 3, 65), (2, 1, 4608), (1, 2, T - 1), (0, 2, T), (3, 2, T + 1), (1, 1, 20011), (2, 130, 2),
            (0, W // 64 + 1, 64)]


def _rows(rows, L, mean, sd, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, L, generator=g, dtype=torch.float64) * sd + mean).to(torch.float32)


def run_kernel(dev):
    """ONE launch over every shape at every (mean, sd) of the grid, plus a record whose middle row is constant; the float64 rule of every row"""
    ops, item_plan = E.mods()
    recs, data, off = [], [], 64
    for g, (mean, sd) in enumerate(WN.GRID):
        for s, (skew, rows, L) in enumerate(_shapes()):
            recs.append((off + skew, rows, L))
            data.append(_rows(rows, L, mean, sd, 1000 * g + s))
            off = (off + skew + rows * L + 63) // 64 * 64 + 64  # at least 64 sentinels between two records
    const = _rows(3, 100, 0.0, 1.0, 77)
    const[1] = 0.25
    recs.append((off + 1, 3, 100))
    data.append(const)
    n = (off + 1 + 300 + 63) // 64 * 64 + 64
    host = torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32).clone()
    for (o, rows, L), x in zip(recs, data):
        host[o:o + rows * L] = x.reshape(-1)
    items = item_plan.wnorm_items(recs, ops.WNORM_ITEM_ELEMS)
    flat = host.to(dev)
    status = _launch(flat, items)
    return dict(host=host, out=flat.cpu(), status=status.cpu(), recs=recs, items=items, data=data, n=n, ref=[WN.rule64(x.numpy()) for x in data])


@pytest.fixture(scope="module")
def kernel_run(dev):
    """computed once, shared by the tests below, which leave it unchanged"""
    return run_kernel(dev)


def _planned(k):
    mask = torch.zeros(k["n"], dtype=torch.bool)
    for o, rows, L in k["recs"]:
        mask[o:o + rows * L] = True
    return mask


# ---- 1. the kernel against the float64 rule ------------------------------------------------------------------------------------------------------
def test_the_layout_sits_on_the_boundaries(kernel_run):
    ops, _ = E.mods()
    k = kernel_run
    T, W = ops.WNORM_WAVE_ROW_MAX, ops.WNORM_ITEM_ELEMS
    assert k["n"] < 400_000 and len(k["recs"]) == 4 * 10 + 1
    assert {L for _, _, L in k["recs"]} >= {2, 64, 65, 147, T - 1, T, T + 1, 4608, 20011}
    assert {o & 3 for o, _, _ in k["recs"]} == {0, 1, 2, 3}  # every alignment of a first element
    spans = [(o, rows) for o, rows, L in k["recs"] if L == 64 and rows == W // 64 + 1]
    assert len(spans) == 4 and all(sum(1 for f, L, nr in k["items"] if o <= f < o + rows * 64) == 2 for o, rows in spans)  # two items each
    assert len(k["items"]) > 1


def test_every_element_is_within_the_native_bound(kernel_run):
    k = kernel_run
    assert k["status"].tolist() == [0] * len(k["items"])
    worst = (0.0, None)
    for (o, rows, L), x, (M, N, Y) in zip(k["recs"], k["data"], k["ref"]):
        ok = N[:, 0] > 0
        got = k["out"][o:o + rows * L].view(rows, L).numpy()
        assert np.isfinite(got[ok]).all()
        r = WN.worst_ratio(got[ok], Y[ok], WN.native_bound(M[ok], N[ok], Y[ok]))
        worst = max(worst, (r, (rows, L, float(x.double().mean()))))
        assert r <= 1.0, (o, rows, L, r)
    print(f"largest |y - Y| / native bound: {worst[0]:.3f} at (rows, L, mean) = {worst[1]}")


def test_sentinels_keep_their_bits(kernel_run):
    k = kernel_run
    gap = ~_planned(k)
    before, after = k["host"].view(torch.int32), k["out"].view(torch.int32)
    assert gap.sum().item() >= 64 * len(k["recs"]) and (before[gap] == SENTINEL).all()
    assert torch.equal(before[gap], after[gap])
    assert not torch.equal(before[~gap], after[~gap])


def test_a_second_run_gives_the_same_bits(kernel_run, dev):
    k = kernel_run
    again = k["host"].to(dev)
    assert _launch(again, k["items"]).tolist() == [0] * len(k["items"])
    assert torch.equal(again.cpu().view(torch.int32), k["out"].view(torch.int32))
    # ... and so does another cut of the same rows into items: a row's result does not depend on the item or the workgroup that took it,
    # as long as its length keeps it on the same side of WNORM_WAVE_ROW_MAX
    _, item_plan = E.mods()
    other = k["host"].to(dev)
    items = item_plan.wnorm_items(k["recs"], 1000)
    assert len(items) > len(k["items"]) and _launch(other, items).tolist() == [0] * len(items)
    assert torch.equal(other.cpu().view(torch.int32), k["out"].view(torch.int32))


def test_a_second_application_moves_nothing_beyond_the_bound(kernel_run, dev):
    k = kernel_run
    twice = k["out"].to(dev)
    assert _launch(twice, k["items"]).tolist() == [0] * len(k["items"])
    twice = twice.cpu()
    for (o, rows, L), (M, N, Y) in zip(k["recs"], k["ref"]):
        ok = N[:, 0] > 0
        y1, y2 = (t[o:o + rows * L].view(rows, L).numpy() for t in (k["out"], twice))
        assert WN.worst_ratio(y2[ok], y1[ok], WN.reapply_bound(WN.native_bound(M[ok], N[ok], Y[ok]), y1[ok])) <= 1.0, (o, rows, L)
    gap = ~_planned(k)
    assert torch.equal(twice.view(torch.int32)[gap], k["host"].view(torch.int32)[gap])


def test_a_constant_row_becomes_nan_and_its_neighbours_do_not(kernel_run):
    k = kernel_run
    o, rows, L = k["recs"][-1]
    got = k["out"][o:o + rows * L].view(rows, L)
    assert (rows, L) == (3, 100) and torch.isnan(got[1]).all() and torch.isfinite(got[0]).all() and torch.isfinite(got[2]).all()
    M, N, Y = k["ref"][-1]
    assert N[1, 0] == 0 and WN.worst_ratio(got[[0, 2]].numpy(), Y[[0, 2]], WN.native_bound(M[[0, 2]], N[[0, 2]], Y[[0, 2]])) <= 1.0


def test_the_recorded_bits(dev):
    """tests/golden/row_kernels_bits.npz (make_row_kernels_golden.py): the same call on the stored input gives the stored bits — rows shorter than
    the scalar head, every head and tail, both sides of WNORM_WAVE_ROW_MAX, items of one, three and six rows —, NaN rows and sentinel gaps included.
    A difference means the arithmetic or the order of a sum has changed; the file is not made again from the kernel it tests."""
    import row_bits_common as R

    z = np.load(R.FIXTURE)
    recs = [tuple(int(v) for v in r) for r in z["records"]]
    assert recs == R.layout()[0]
    got = R.run_weight_norm(recs, z["w"].copy(), dev)
    want = z["wnorm/out"]
    assert got["wnorm/status"].tolist() == z["wnorm/status"].tolist() == [0] * len(recs)
    mask = R.row_mask(want.size, R.rows_of(recs))
    o, rows, L = recs[R.CONST_RECORD]
    const = slice(o + R.CONST_ROW * L, o + (R.CONST_ROW + 1) * L)
    assert np.isnan(want[const]).all() and np.isfinite(want[o:o + L]).all() and np.isfinite(want[o + 2 * L:o + 3 * L]).all()
    assert np.array_equal(np.isnan(got["wnorm/out"]), np.isnan(want)), "the NaN pattern: the constant row, the row of one element, the gaps"
    assert np.array_equal(got["wnorm/out"][const].view(np.int32), want[const].view(np.int32))
    assert (want.view(np.int32)[~mask] == SENTINEL).all() and (got["wnorm/out"].view(np.int32)[~mask] == SENTINEL).all()
    assert R.same_bits(got["wnorm/out"], want)


# ---- 2. items that do not fit --------------------------------------------------------------------------------------------------------------------
def test_items_that_do_not_fit_are_refused_and_their_memory_untouched(dev):
    """an item that ends past n, one that starts before 0 and two with an empty shape in one launch with two valid items, which come out right.
    Every access is behind the item check: nothing here can reach outside the array."""
    n = 2048
    host = torch.full((n,), SENTINEL, dtype=torch.int32).view(torch.float32).clone()
    a, b = _rows(4, 33, 0.05, 0.02, 5), _rows(1, 1500, 0.0, 1.0, 6)
    host[5:5 + 132], host[256:1756] = a.reshape(-1), b.reshape(-1)
    host[1800:n] = _rows(1, n - 1800, 0.0, 1.0, 7).reshape(-1)  # finite values where the refused items point
    items = [(5, 33, 4), (n - 10, 8, 2), (256, 1500, 1), (-64, 8, 2), (1800, 0, 4), (1800, 4, 0)]
    flat = host.to(dev)
    assert _launch(flat, items).tolist() == [0, 2, 0, 2, 2, 2]
    out = flat.cpu()
    huge = host.to(dev)  # row_len * n_rows far beyond n (and beyond 2^32): a launch of its own, the wrapper would call it an overlap
    assert _launch(huge, [(0, 2 ** 31 - 1, 2 ** 31 - 1)]).tolist() == [2]
    assert torch.equal(huge.cpu().view(torch.int32), host.view(torch.int32))
    for x, (o, rows, L) in ((a, (5, 4, 33)), (b, (256, 1, 1500))):
        M, N, Y = WN.rule64(x.numpy())
        assert WN.worst_ratio(out[o:o + rows * L].view(rows, L).numpy(), Y, WN.native_bound(M, N, Y)) <= 1.0
    keep = torch.ones(n, dtype=torch.bool)
    keep[5:5 + 132], keep[256:1756] = False, False
    assert torch.equal(out.view(torch.int32)[keep], host.view(torch.int32)[keep])


def test_overlapping_items_are_refused_by_the_wrapper(dev):
    ops, item_plan = E.mods()
    flat = torch.ones(256, device=dev)
    items = [(0, 16, 4), (32, 8, 2)]
    with pytest.raises(ValueError, match="overlaps"):
        ops.weight_norm_rows_(flat, items, item_plan.pack_records(items, dev))
    with pytest.raises(ValueError):  # a table that does not match the host items
        ops.weight_norm_rows_(flat, items[:1], item_plan.pack_records(items, dev))
    assert (flat == 1).all()


# ---- 3. the reference's recorded run -------------------------------------------------------------------------------------------------------------
def test_against_the_reference_fixture(dev):
    """the fixture's weights laid out as a flat array under a hand-made table (the raw OIHW arrays: a row is the same set of elements in either
    memory order), planned by item_plan.wnorm_records: within the native bound plus the reference bound of what the reference's own callback
    left; what the planner does not select — biases, the Conv1d, both BatchNorm weights — keeps its bits, where the reference turned the
    64-channel BatchNorm weight into NaN"""
    ops, item_plan = E.mods()
    z = np.load(os.path.join(HERE, "golden", "weight_norm_ref.npz"))
    names = json.loads(bytes(z["names"]))
    for d in range(2):
        table, off, chunks = [], 3, []
        for name in names:
            for kind in ("before", "bias_before"):
                key = f"d{d}/{name}/{kind}"
                if key in z:
                    table.append((f"{name}.{'weight' if kind == 'before' else 'bias'}", 0, off, tuple(z[key].shape)))
                    chunks.append((off, torch.from_numpy(z[key].reshape(-1).copy())))
                    off += z[key].size + 5
        host = torch.full((off + 64,), SENTINEL, dtype=torch.int32).view(torch.float32).clone()
        for o, t in chunks:
            host[o:o + t.numel()] = t
        recs = item_plan.wnorm_records(table)
        by_off = {o: nm for nm, _, o, _ in table}
        assert [by_off[r[0]] for r in recs] == ["stem.weight", "point.weight", "conv3.weight", "fc.weight", "flat.weight"]
        items = item_plan.wnorm_items(recs, ops.WNORM_ITEM_ELEMS)
        flat = host.to(dev)
        assert _launch(flat, items).tolist() == [0] * len(items)
        out = flat.cpu()
        mask = torch.zeros(host.numel(), dtype=torch.bool)
        for o, rows, L in recs:
            mask[o:o + rows * L] = True
            name = by_off[o][: -len(".weight")]
            x = z[f"d{d}/{name}/before"].reshape(rows, L)
            want = z[f"d{d}/{name}/after"].reshape(rows, L)
            got = out[o:o + rows * L].view(rows, L).numpy()
            M, N, Y = WN.rule64(x)
            ok = N[:, 0] > 0
            assert np.isnan(got[~ok]).all() and np.isnan(want[~ok]).all() and (~ok).sum() == (name == "flat")
            bound = WN.native_bound(M[ok], N[ok], Y[ok]) + WN.reference_bound(x[ok], M[ok], N[ok], Y[ok])
            assert WN.worst_ratio(got[ok], want[ok], bound) <= 1.0, (d, name)
        assert torch.equal(out.view(torch.int32)[~mask], host.view(torch.int32)[~mask])
        bn64 = next(o for nm, _, o, _ in table if nm == "bn64.weight")
        assert torch.isfinite(out[bn64:bn64 + 64]).all() and np.isnan(z[f"d{d}/bn64/after"]).all()


# ---- 4. the callback on the models, through the Runner -----------------------------------------------------------------------------------------------
def _resnet50(dtype):
    from sota_imagenet_amd.models import resnet50

    return resnet50(dtype=dtype)


def _bresnet50(dtype):
    from sota_imagenet_amd.models import resnet50

    return resnet50(stem_type="deep", antialias=True, attn_type="eca", norm_layer="inplaceabn", norm_act="leaky_relu", dtype=dtype)


def _row_defects(pre, post, recs):
    """on the device, in float64: the largest |mean y| / (mean of the bound) and | ||y|| - 1 | / (2-norm of the bound) over all planned rows,
    the bound taken of what the optimizer step left (pre)"""
    worst_m = torch.zeros((), dtype=torch.float64, device=pre.device)
    worst_n = torch.zeros((), dtype=torch.float64, device=pre.device)
    for off, rows, L in recs:
        x = pre[off:off + rows * L].view(rows, L).double()
        y = post[off:off + rows * L].view(rows, L).double()
        M = x.mean(-1, keepdim=True)
        C = x - M
        N = C.pow(2).sum(-1, keepdim=True).sqrt()
        B = 8 * WN.U * (C / N).abs() + 4 * WN.U * M.abs() / N
        worst_m = torch.maximum(worst_m, (y.mean(-1).abs() / B.mean(-1)).max())
        worst_n = torch.maximum(worst_n, ((y.pow(2).sum(-1).sqrt() - 1).abs() / B.pow(2).sum(-1).sqrt()).max())
    return worst_m.item(), worst_n.item()


@pytest.mark.parametrize("make,dtype", [(_resnet50, "fp32"), (_resnet50, "bf16"), (_bresnet50, "bf16")], ids=["resnet50-fp32", "resnet50-bf16", "bresnet50-bf16"])
def test_three_runner_steps_with_adamw(dev, monkeypatch, make, dtype):
    from sota_imagenet_amd import callbacks, fit_wrapper as fw, item_plan, ops, optim
    from sota_imagenet_amd.losses import CrossEntropyLoss
    from sota_imagenet_amd.synth import synthetic_batch

    N, S, STEPS = 4, 64, 3
    m = make(dtype).cuda()
    opt = optim.AdamW([{"params": list(m.parameters())}], lr=1e-3, weight_decay=1e-2, eps=1e-6)
    calls, launch = [], ops.weight_norm_rows_

    def spy(flat, items_host, items_dev):
        calls.append(flat.data_ptr())
        return launch(flat, items_host, items_dev)

    monkeypatch.setattr(ops, "weight_norm_rows_", spy)
    pre, post, losses = [], [], []

    class Before(fw.Callback):  # in front of WeightNorm: what the optimizer step left
        def on_batch_end(self):
            if self.state.is_train:
                pre.append((m.flat_params.detach().clone(), m._flat_buffers.detach().clone()))

    class After(fw.Callback):
        def on_batch_end(self):
            if self.state.is_train:
                post.append((m.flat_params.detach().clone(), m._flat_buffers.detach().clone()))
                losses.append(self.state.loss_meter.avg)

    wn = callbacks.WeightNorm()
    batches = [synthetic_batch(N, S, seed=1, index=i, device="cuda") for i in range(STEPS)]

    class Loader:
        batch_size = N

        def __len__(self):
            return len(batches)

        def __iter__(self):
            return iter(batches)

    runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1).cuda(), callbacks=[Before(), wn, After()])
    w0 = m.flat_params.detach().clone()
    runner.fit(Loader(), epochs=1)
    torch.cuda.synchronize()
    # one launch per training batch, on the model's own flat array
    assert calls == [m.flat_params.data_ptr()] * STEPS and wn.launches == STEPS and len(pre) == len(post) == STEPS
    assert wn.status.tolist() == [0] * len(wn.items)
    recs = wn.records
    assert recs == item_plan.wnorm_records(m._table) and len(wn.names) == len(recs)
    if make is _resnet50:
        assert len(recs) == 54 and sum(r * L for _, r, L in recs) == 25502912
    planned = torch.zeros(m._nparam, dtype=torch.bool, device=dev)
    for off, rows, L in recs:
        planned[off:off + rows * L] = True
    by_name = {name: (off, shape) for name, kind, off, shape in m._table if kind == 0}
    for name, (off, shape) in by_name.items():  # BatchNorm tensors, biases and (BResNet-50) the ECA Conv1d weights are outside the plan
        if len(shape) < 2 or math.prod(shape) < 64:
            assert not planned[off:off + math.prod(shape)].any(), name
    off, shape = by_name["fc.weight"]
    assert planned[off:off + math.prod(shape)].all() and not planned[off + math.prod(shape):off + math.prod(shape) + 2048].any()  # the padding rows
    assert not torch.equal(pre[0][0], w0)  # the first forward and step used the initial weights, the step moved them
    for k in range(STEPS):
        (p0, b0), (p1, b1) = pre[k], post[k]
        dm, dn = _row_defects(p0, p1, recs)
        print(f"step {k}: largest |mean| / bound {dm:.3f}, | norm - 1 | / bound {dn:.3f}")
        assert dm <= 1.0 and dn <= 1.0
        assert torch.equal(p0.view(torch.int32)[~planned], p1.view(torch.int32)[~planned])  # BatchNorm tensors, biases, gaps, padding
        assert torch.equal(b0.view(torch.int32), b1.view(torch.int32))                      # the buffers
        assert not torch.equal(p0[planned], p1[planned])
        assert torch.isfinite(p1).all() and math.isfinite(float(losses[k]))
    # step 1 == one step without the callback (which had not acted yet: the snapshot in front of it) followed by ops.weight_norm_rows_
    alone = pre[0][0].clone()
    items = item_plan.wnorm_items(recs, ops.WNORM_ITEM_ELEMS)
    assert launch(alone, items, item_plan.pack_records(items, dev)).tolist() == [0] * len(items)
    assert torch.equal(alone.view(torch.int32), post[0][0].view(torch.int32))
    # the next forward reads the normalised weights: the logits of a fresh model loaded from state_dict()
    assert torch.equal(m.flat_params.detach().view(torch.int32), post[-1][0].view(torch.int32))
    fresh = make(dtype)
    fresh.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    fresh = fresh.cuda().eval()
    m.eval()
    with torch.no_grad():
        data = batches[0][0]
        assert torch.equal(m(data), fresh(data))
    # an evaluate() pass changes no parameter and launches nothing
    runner.evaluate(Loader())
    torch.cuda.synchronize()
    assert len(calls) == STEPS and wn.launches == STEPS
    assert torch.equal(m.flat_params.detach().view(torch.int32), post[-1][0].view(torch.int32))


# ---- 5. train.py -------------------------------------------------------------------------------------------------------------------------------------
def test_train_py_runs_recipe_14_smoke_config(dev, tmp_path, monkeypatch):
    """adamw_std_test.yaml through train.py: the alias puts the callback behind the parameter average's place in the list, both debug epochs
    run, every training batch is one launch, the weights end normalised and finite"""
    sys.path.insert(0, ROOT)
    import train
    from sota_imagenet_amd import callbacks

    made = []
    init = callbacks.WeightNorm.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append(self)

    monkeypatch.setattr(callbacks.WeightNorm, "__init__", spy)
    logdir = os.path.relpath(str(tmp_path), ROOT)
    val_loss, metrics = train.main(["+hydra_exp=adamw_std_test", f"log.dir={logdir}", "random_seed=0", "data.pool=2"])
    assert val_loss == val_loss and 0.0 <= metrics["Acc@1"].avg <= 100.0
    assert len(made) == 1 and made[0].launches == 20 and len(made[0].records) == 54  # two debug epochs of 10 training steps
    assert made[0].status.tolist() == [0] * len(made[0].items)
    m = made[0].state.model
    assert torch.isfinite(m.flat_params).all()
    w = m.conv1.weight.detach().reshape(64, 147).double()
    assert (w.pow(2).sum(-1).sqrt() - 1).abs().max().item() < 1e-5 and w.mean(-1).abs().max().item() < 1e-5
