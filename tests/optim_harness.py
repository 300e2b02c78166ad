"""What the optimizer / SAM tests share (test_adam, test_madgrad_adais, test_layerwise, test_layerwise_unit, test_adamp, test_sam, test_sam_lw,
test_grad_dist and their *_common.py fixture modules), each stated once: the yardstick rule, the base of the recorded-trajectory fixtures, the
flat test buffers, the model-scale helpers, the ModelEma comparison and the train.py smoke run.  Imports on a machine without a GPU.

The yardstick rule of this family: a native tensor may be no further from the float64 reference than FACTOR times the distance of the
reference's own float32 run from it (the yardstick, stored in the fixture or computed from a restatement, never from the code under test), plus a
floor of 4 * 2^-24 (two float32 ulps) of the largest reference magnitude.  FACTOR = 1.5 is the project's factor
(test_resnet_gpu.py::test_fp32_forward_backward_matches_cpu)."""
import glob
import json
import math
import os
import re
import sys

import numpy as np
import torch

from plan_common import layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
FACTOR = 1.5
NAN = float("nan")


# ---- the yardstick rule --------------------------------------------------------------------------------------------------------------------
def bound(yard, ref_max):
    """the largest error the rule accepts"""
    return FACTOR * yard + 4 * U * ref_max


def within_yardstick(got, ref, yard, label, floor_in_ratio=False, yard_name="reference fp32"):
    """one tensor against its float64 reference: prints the figures, asserts the rule and returns the ratio the callers report as "worst",
    err / yard, or err / max(yard, floor) with floor_in_ratio (where a yardstick may lie below the floor, or be zero)"""
    ref = ref.detach().double().cpu()
    err = (got.detach().double().cpu() - ref).abs().max().item()
    ref_max = ref.abs().max().item()
    floor = bound(0.0, ref_max)
    ratio = err / (max(yard, floor) if floor_in_ratio else yard)
    line = f"{label}: native {err:.3e}  {yard_name} {yard:.3e}" + ("" if floor_in_ratio else f"  ratio {ratio:.2f}") + f"  floor {floor:.2e}"
    print(line)
    assert err <= bound(yard, ref_max), line  # (this way round: a NaN error fails)
    return ratio


# ---- the recorded trajectories -------------------------------------------------------------------------------------------------------------
def _js(a):
    return json.loads(bytes(a).decode())


class TrajectoryFixture:
    """what the files tests/golden/*_ref_trajectories.npz share, for one case: the problem (shapes, param groups, p0), the case's constructor
    arguments and lr per step and, where the file records an optimizer's own trajectory, the float64 parameters after every step with their
    yardstick and the state after step 5.  A record is the case's own ("<case>/<name>") or, failing that, the file's."""

    GOLDEN = None  # the subclass's file
    YARD_NAME = "reference fp32"

    def __init__(self, case):
        self.case, self.z = case, np.load(self.GOLDEN)
        self.shapes, self.groups = _js(self.rec("shapes")), _js(self.rec("groups"))
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.offs = np.cumsum([0] + self.sizes)
        self.p0 = torch.from_numpy(self.rec("p0"))
        self.hyper = _js(self.rec("hyper"))
        self.cls = self.hyper.pop("cls", None)
        self.lrs = [float(x) for x in self.rec("lrs")]
        if self.has("p64"):
            self.p64, self.yard = torch.from_numpy(self.rec("p64")), self.rec("yard")
        if self.has("state_keys"):
            self.state_keys, self.state_shapes = _js(self.rec("state_keys")), _js(self.rec("state_shapes"))
        self.state5 = self.states("state5")

    def has(self, name):
        return f"{self.case}/{name}" in self.z.files

    def rec(self, name):
        return self.z[f"{self.case}/{name}" if self.has(name) else name]

    def states(self, name):
        """{state key: flat tensor} of the optimizer state recorded under "<case>/<name>/" """
        prefix = f"{self.case}/{name}/"
        return {k[len(prefix):]: torch.from_numpy(self.z[k]) for k in self.z.files if k.startswith(prefix)}

    def split(self, flat):
        return [flat[self.offs[i]:self.offs[i + 1]] for i in range(len(self.shapes))]

    def tensor_label(self, i):
        return f"tensor {i}"

    def check_tensors(self, got, ref_flat, yards, label, **kw):
        """got: native values, flat in the fixture's tensor order or already split; every tensor by the yardstick rule; returns the worst ratio"""
        got = self.split(got.detach().cpu()) if torch.is_tensor(got) else got
        return max(within_yardstick(g, r, y, f"{label} {self.tensor_label(i)}", yard_name=self.YARD_NAME, **kw)
                   for i, (g, r, y) in enumerate(zip(got, self.split(ref_flat), yards)))

    def check(self, k, got, what):
        """got: the native parameters after step k + 1"""
        return self.check_tensors(got, self.p64[k], self.yard[k], f"{what} step {k + 1}")


# ---- flat test buffers ---------------------------------------------------------------------------------------------------------------------
def flat_params(sizes, shapes, values, dev, order=None, separate=False, grad_fill=NAN):
    """parameters as views of one flat parameter / gradient buffer under the 64-element alignment rule (plan_common.layout: zero in every gap
    of p, grad_fill in every gap of g), or each in its own allocation; returns (params in tensor order, flat p, flat g, element offsets)"""
    offs, n = layout(sizes, order)
    fp, fg = torch.zeros(n, device=dev), torch.full((n,), grad_fill, device=dev)
    ps = []
    for o, s, shape, val in zip(offs, sizes, shapes, values):
        if separate:
            p = torch.nn.Parameter(val.to(dev).clone().view(shape))
            p.grad = torch.zeros(s, device=dev).view(shape)
        else:
            fp[o:o + s] = val.to(dev).reshape(-1)
            p = torch.nn.Parameter(fp[o:o + s].view(shape))
            p.grad = fg[o:o + s].view(shape)
        ps.append(p)
    return ps, fp, fg, offs


def fixture_problem(fx, dev, p_flat0=None, separate=False, grad_fill=NAN):
    """the fixture's tensors laid out group by group, and its two param groups; returns (params, groups, flat p, flat g, offsets)"""
    order = [i for idx in fx.groups for i in idx]
    ps, fp, fg, offs = flat_params(fx.sizes, fx.shapes, fx.split(fx.p0 if p_flat0 is None else p_flat0), dev, order, separate, grad_fill)
    groups = [{"params": [ps[i] for i in fx.groups[0]]}, {"params": [ps[i] for i in fx.groups[1]], "weight_decay": 0}]
    return ps, groups, fp, fg, offs


def make_opt(fx, groups, lr):
    from sota_imagenet_amd import optim

    return getattr(optim, fx.cls)(groups, lr=lr, **fx.hyper)


def set_grads(ps, grads, mult=1.0):
    for p, g in zip(ps, grads):
        p.grad.copy_((g * mult).view(p.shape))


def gather(ps):
    return torch.cat([p.detach().reshape(-1) for p in ps])


def gaps(ps, fp):
    """the elements of the flat buffer that belong to no parameter"""
    mask = torch.ones_like(fp, dtype=torch.bool)
    for p in ps:
        o = (p.data_ptr() - fp.data_ptr()) // 4
        mask[o:o + p.numel()] = False
    return mask


# ---- model scale ---------------------------------------------------------------------------------------------------------------------------
def padding_mask(m):
    return gaps(m.parameters(), m.flat_params)


def grads_for(m, seed, scale=1e-2, pad=NAN):
    """one flat gradient for every parameter of a flat model, `pad` in the padding (0.0: what a backward leaves there)"""
    g = torch.full_like(m.flat_grads, pad)
    for i, (name, p) in enumerate(m.named_parameters()):
        off = (p.data_ptr() - m.flat_params.data_ptr()) // 4
        gen = torch.Generator().manual_seed(seed * 1000 + i)
        g[off: off + p.numel()] = (torch.randn((p.numel(),), generator=gen) * scale).to(g.device)
    return g


def flat_steps(m, opt, seeds, lr, pad=NAN):
    for s in seeds:
        m.flat_grads.copy_(grads_for(m, s, pad=pad))
        for g in opt.param_groups:
            g["lr"] = lr
        if hasattr(opt, "attach_model"):  # (a stock torch optimizer's zero_grad would unbind the flat gradient views)
            opt.zero_grad()
        opt.step()
    torch.cuda.synchronize()


def model_opt(cls_name, kwargs, lr, groups_of=None):
    """a flat fp32 resnet50 on the device and the native optimizer attached to it"""
    from sota_imagenet_amd import optim
    from sota_imagenet_amd.models import resnet50

    m = resnet50(dtype="fp32").cuda()
    groups = groups_of(m) if groups_of else [{"params": list(m.parameters())}]
    opt = getattr(optim, cls_name)(groups, lr=lr, **kwargs)
    opt.attach_model(m)
    return m, opt


def count_launches(monkeypatch, names, calls=None):
    """wraps ops.<name> for every name so that each call appends its name to `calls`"""
    from sota_imagenet_amd import ops

    calls = [] if calls is None else calls
    for name in names:
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda f, n: lambda *a, **k: (calls.append(n), f(*a, **k))[1])(fn, name))
    return calls


class Loader:
    """n synthetic batches of 4 images at 64 px on the device"""

    batch_size = 4

    def __init__(self, n=3, seed=6):
        from sota_imagenet_amd.synth import synthetic_batch

        self.batches = [synthetic_batch(4, 64, seed=seed, index=i, device="cuda") for i in range(n)]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


# ---- the ModelEma comparison ---------------------------------------------------------------------------------------------------------------
def ema_matches_callback(make_model_opt, lr, callbacks=(), val_loader=None, after_fit=None):
    """one epoch of three batches through Runner, lr ramping from lr to 2 * lr, with the average advanced inside the step kernel (attach_ema)
    and by ModelEma's own lerp after every batch: the parameters and buffers are the same bits either way, the average is finite, is not the
    parameters and agrees to 1e-6 of its magnitude.  callbacks: classes built anew for each run and appended behind ModelEma; after_fit gets
    their instances.  Returns the two averages."""
    from sota_imagenet_amd import fit_wrapper as fw
    from sota_imagenet_amd.losses import CrossEntropyLoss

    res = []
    for fused in (True, False):
        m, opt = make_model_opt()
        ema = fw.ModelEma(m, 0.9)
        if not fused:
            ema.on_begin = lambda: None
        extra = [cb() for cb in callbacks]
        runner = fw.Runner(m, opt, CrossEntropyLoss(smoothing=0.1), callbacks=[fw.PhasesScheduler([dict(ep=(0, 1), lr=(lr, 2 * lr))]), ema, *extra])
        runner.fit(Loader(), val_loader=val_loader or Loader(), epochs=1)
        assert ema._fused == fused and not ema._swapped
        if after_fit:
            after_fit(*extra)
        res.append((m.flat_params.clone(), ema.ema[0].clone(), ema.ema[1].clone()))
    (p_a, e_a, b_a), (p_b, e_b, b_b) = res
    assert torch.equal(p_a, p_b) and torch.equal(b_a, b_b)
    assert not torch.equal(e_a, p_a) and torch.isfinite(e_a).all()
    assert ((e_a - e_b).abs().max() / e_b.abs().max()).item() < 1e-6
    return e_a, e_b


# ---- the train.py smoke run ----------------------------------------------------------------------------------------------------------------
def run_smoke_config(name, tmp_path, overrides, resume_eval=False):
    """train.py on configs/hydra_exp/<name>.yaml with the log directory under tmp_path: the validation loss is finite and Acc@1 a percentage;
    with resume_eval the checkpoint then evaluates after a resume.  Returns (val_loss, metrics, run directory, the "Train loss:" figures)."""
    sys.path.insert(0, ROOT)
    import train

    logdir = os.path.relpath(str(tmp_path), ROOT)
    val_loss, metrics = train.main([f"+hydra_exp={name}", f"log.dir={logdir}", *overrides])
    assert math.isfinite(val_loss) and 0.0 <= metrics["Acc@1"].avg <= 100.0
    run = glob.glob(os.path.join(str(tmp_path), f"*_{name}", "*"))[0]
    with open(os.path.join(run, "logs.txt")) as fh:
        losses = [float(x) for x in re.findall(r"Train loss: ([0-9.]+)", fh.read())]
    if resume_eval:
        loss2, m2 = train.main([f"+hydra_exp={name}", f"log.dir={logdir}", f"run.resume={os.path.join(run, 'model.chpn')}", "run.evaluate=true",
                                "data.pool=2"])
        assert math.isfinite(loss2) and 0.0 <= m2["Acc@1"].avg <= 100.0
    return val_loss, metrics, run, losses
