"""The BACKWARD of the ResNet-50 executor, teacher forced against the oracle segment by segment (the forward's counterpart is
test_resnet_gpu.py::test_teacher_forced_layers).

Every backward segment (head, layer4.2 ... layer1.0, stem: `m.grad_segments` order) is re-derived in fp64 by
oracle/resnet50_bwd_ref.py FROM THE EXECUTOR'S OWN stored activations and from the gradient the executor itself handed to that
segment (`grad.cur`, recorded between two native calls), so a segment's result differs from the reference by that segment's own
wiring and kernels only — no chaotic amplification through the blocks above, and nothing shared with the code under test: the
whole-model tests allow 5e-2 on the flat gradient, and the A/B tests compare the executor with itself (bn_bwd_apply, the on-the-fly
ReLU masks, the shortcut addend, the half-resolution downsample gradient, gap_bwd / the FC kernels and the stem's argmax codes are
common to both of their arms).

Checked per segment: every parameter gradient by name (`.grad` views), the segment's whole slice of `flat_grads`, the outgoing
gradient (the next `grad.cur`), and `dpooled` for the head.  Bound per quantity: l2err(native, fp64) < 1.5 * yard + floor, where
  yard   the reference's own `lowprec` chain (fp32 arithmetic / bf16 storage points) against its fp64 chain on the same tensors
  1.5    what test_resnet_gpu.py grants native over torch-CPU
  floor  2e-5 in fp32 (the per-op fp32 tolerance: MFMA summation order), 2**-9 in bf16 (one more bf16 rounding of every element
         moves the relative L2 by at most the unit roundoff)
tests/test_resnet_bwd_ref_host.py shows on the CPU that the chain equals autograd, that the yardsticks stay under the per-op
tolerances at these batches, and that planted wiring errors exceed this bound.

Measured on an MI355X (every arm passes; native/yard over every checked quantity of every segment whose yard is not zero):

  arm                        largest native/bound   native/yard       per segment, worst quantity: native (yard)
  fp32 4 x 64                0.060                  0.55 ... 3.9      head 2.7e-7 (2.4e-7), blocks 6.6e-7 ... 1.3e-6 (6.2e-7 ... 1.2e-6), stem 1.2e-6 (1.7e-6)
  fp32 3 x 96                0.068                  0.40 ... 7.3      head 2.6e-7 (6.6e-7), blocks 6.6e-7 ... 1.5e-6 (6.2e-7 ... 1.4e-6), stem 1.0e-6 (1.3e-6)
  bf16 4 x 64                0.636                  0.981 ... 1.020   head 1.77e-3, blocks 3.8e-3 ... 6.5e-3, stem 2.74e-2 (every yard the same to 2 %)
  bf16 3 x 96                0.632                  0.977 ... 1.020   head 1.69e-3, blocks 3.8e-3 ... 5.3e-3, stem 2.37e-2
  bf16 4 x 64 FUSE_BN_BWD=0  0.635                  0.984 ... 1.012   as the default arm; stem 2.64e-2
  bf16 4 x 64 STEM_FUSED=0   0.636                  0.981 ... 1.020   as the default arm
  bf16 4 x 64 DS_COMPACT=0   0.636                  0.981 ... 1.020   as the default arm
  bf16 4 x 64 DCONV=0        0.634                  0.991 ... 1.010   head 1.75e-3, blocks 3.7e-3 ... 5.5e-3, stem 2.53e-2

In fp32 every quantity sits at 1e-6, a twentieth of the bound (the ratios above 2 belong to quantities whose yard is below 2e-7).  In
bf16 the executor's distance to the fp64 chain IS the yardstick's to within 2 %: the lowprec chain rounds where the executor rounds, so
the two land on nearly the same values, and half of every bound is the floor.  Quantities whose bf16 yard is zero (sums the executor
forms in fp32 from bf16 tensors: bn3 / downsample BN of the incoming gradient, fc, dpooled) are at most 2.8e-7 from fp64.
The largest yard is the stem's bn1.bias: 2.4e-2 ... 2.7e-2 on the executor's tensors, above the 1.7e-2 / 1.8e-2 the same batches give on the
oracle's stand-in tensors (test_resnet_bwd_ref_host.py explains the cancellation); every other yard is below 7e-3.
Two deliberately wrong builds of resnet_exec.cpp (identity shortcut addend without `out_bits`; `M - 1` handed to
launch_bn_bwd_finalize) fail every arm they were run on (the six 4 x 64 arms, on the batch of seed 5, index 0): the first in `out` of every identity block, 0.36 ... 0.38
against a bound of 7e-3; the second in fp32 on every block, in bf16 on layers 3 and 4 (M = 16 and 64: 7e-3 ... 1e-1 against 5e-3 ... 8e-3).
"""
import pytest
import torch

from oracle import ops_ref as R
from oracle import resnet50_bwd_ref as B
from sota_imagenet_amd.synth import synthetic_batch
from test_resnet_bwd_ref_host import FLOOR, SHAPES, TDT  # the batches, floors and storage types the host test judges the reference at
from test_resnet_gpu import _segmented_backward, build, l2err, nerr

pytestmark = pytest.mark.gpu

ARMS = [("fp32", (4, 64), {}), ("fp32", (3, 96), {}), ("bf16", (4, 64), {}), ("bf16", (3, 96), {}),
        ("bf16", (4, 64), {"MI355_FUSE_BN_BWD": "0"}), ("bf16", (4, 64), {"MI355_STEM_FUSED": "0"}),
        ("bf16", (4, 64), {"MI355_DS_COMPACT": "0"}), ("bf16", (4, 64), {"MI355_DCONV": "0"})]


def _stored_names():
    names = ["conv1.y", "stem.p0", "pooled"]
    for pre, _ in B.BLOCKS:
        names += [f"{pre}.conv1.y", f"{pre}.a1", f"{pre}.conv2.y", f"{pre}.a2", f"{pre}.conv3.y", f"{pre}.out"]
        if pre.endswith(".0"):
            names.append(f"{pre}.downsample.0.y")
    return names


def _step(dtype, shape, record):
    """a fresh model, one training forward + loss at the arm's batch, the stored tensors read BEFORE the backward, then the backward
    (one native call per segment with `grad.cur` recorded, or the plain one)"""
    from sota_imagenet_amd.losses import CrossEntropyLoss

    N, S = shape
    key = (N, S, S)
    m, sd = build(dtype)
    data, target = synthetic_batch(N, S, **SHAPES[shape])
    m.train()
    out = m(data.cuda())
    loss = CrossEntropyLoss(smoothing=0.1)(out, target.cuda())
    if not record:
        loss.backward()
        torch.cuda.synchronize()
        return m
    T = {n: m.debug_tensor(key, n).float().cpu() for n in _stored_names()}
    rec = []
    _segmented_backward(m, loss, key, record=rec)
    T["dpooled"] = m.debug_tensor(key, "dpooled").float().cpu()
    _, dlogits = R.smooth_ce_bwd(out.detach().float().cpu(), target, 0.1)
    return m, sd, data, T, [g.float().cpu() for g in rec], dlogits


@pytest.mark.parametrize("dtype,shape,env", ARMS, ids=[f"{d}-{n}x{s}" + "".join(f"-{k[6:]}={v}" for k, v in e.items()) for d, (n, s), e in ARMS])
def test_backward_segments_teacher_forced_against_the_fp64_chain(dev, dtype, shape, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, sd, data, T, rec, dlogits = _step(dtype, shape, record=True)
    segs = m.grad_segments
    assert len(segs) == len(B.SEGMENTS) == len(rec) + 1
    P = {k: v.float() for k, v in sd.items()}
    params = dict(m.named_parameters())
    flat = m.flat_grads.detach().cpu()
    base = m.flat_grads.data_ptr()
    seen, bad, ratios, exact, worst = set(), [], [], 0.0, 0.0
    for k, seg in enumerate(B.SEGMENTS):
        G = dlogits if k == 0 else rec[k - 1]
        ref = B.segment_bwd(seg, T.__getitem__, P, G, TDT[dtype], None, image=data)
        low = B.segment_bwd(seg, T.__getitem__, P, G, TDT[dtype], dtype, image=data)
        b, e = segs[k]
        got = {"flat": flat[b:e]}
        ref["flat"], low["flat"] = torch.zeros(e - b, dtype=torch.float64), torch.zeros(e - b, dtype=torch.float64)
        for name in [n for n in ref if n in params]:
            g = params[name].grad
            got[name] = g.detach().cpu()
            off = (g.data_ptr() - base) // 4 - b
            assert 0 <= off and off + g.numel() <= e - b, f"{name} lies outside segment {k}"
            for r in (ref, low):
                v = r[name].double()
                r["flat"][off: off + g.numel()] = (v.permute(0, 2, 3, 1) if v.dim() == 4 else v).reshape(-1)  # (KRSC in the flat array)
            seen.add(name)
        if "out" in ref:
            got["out"] = rec[k]
        if "dpooled" in ref:
            got["dpooled"] = T["dpooled"]
        assert set(got) == set(ref), (seg, set(got) ^ set(ref))
        line = None
        for name in ref:
            err, yard = l2err(got[name], ref[name]), l2err(low[name], ref[name])
            bound = 1.5 * yard + FLOOR[dtype]
            if not err < bound:
                bad.append(f"{seg} {name}: native {err:.3e}, yard {yard:.3e}, bound {bound:.3e} (max-norm error {nerr(got[name], ref[name]):.3e})")
            if yard > 0:
                ratios.append(err / yard)
            else:  # bf16: quantities the executor forms in fp32 from bf16 tensors (bn3 / downsample sums of the incoming gradient, the head)
                exact = max(exact, err)
            if line is None or err / bound > line[0]:
                line = (err / bound, name, err, yard)
        worst = max(worst, line[0])
        print(f"{seg:9s} worst {line[1]:28s} native {line[2]:.3e}  yard {line[3]:.3e}  native/yard {line[2] / max(line[3], 1e-30):9.3g}  native/bound {line[0]:.3f}")
    print(f"arm {dtype} {shape} {env}: largest native/bound {worst:.3f}; native/yard {min(ratios):.3f} ... {max(ratios):.3f}; largest native error where yard = 0: {exact:.2e}")
    table = m.kernel_table((shape[0], shape[1], shape[1]))
    if env.get("MI355_DCONV") == "0":  # this arm is the implicit-GEMM backward; the others run the generated kernels wherever the rules pick them
        assert all(v["dgrad"].startswith(("igemm<", "-")) and v["wgrad"].startswith("wgrad<") for v in table.values()), table
    elif dtype == "bf16":
        assert any(not v["dgrad"].startswith(("igemm<", "-")) for v in table.values()) and any(not v["wgrad"].startswith("wgrad<") for v in table.values()), table
    assert seen == set(params), set(params) ^ seen
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_recorded_segmented_backward_leaves_the_bits_of_a_plain_backward(dev, dtype):
    """the test above judges the backward as one native call per segment with `grad.cur` read in between: that must be the path training
    takes (one call), bit for bit"""
    seg = _step(dtype, (4, 64), record=True)[0].flat_grads.detach().clone()
    plain = _step(dtype, (4, 64), record=False).flat_grads.detach()
    assert seg.abs().max() > 0 and torch.equal(seg, plain)
