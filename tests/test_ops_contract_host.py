"""The argument contract of sota_imagenet_amd/ops.py, on the host: every public wrapper that takes tensors has a row with a VALID argument set
at the smallest legal extents (N = 1, H = W = 4, C = 64, tables of one record).
 (a) unpatched: the valid CPU call is refused by _on_device and reaches no enqueueing entry point; one tensor argument at a time made wrong (dtype,
     one element short, one extra dimension, a non-contiguous view, None) is refused by _arg with the wrapper's and the argument's name;
 (b) with the placement test patched out and the library behind a recording proxy: the valid call reaches the entry points it should, with as
     many arguments as the header declares and no null in a required pointer position; the seven EMA wrappers reach their twin with the two
     extra arguments in the header's positions."""
import ctypes
import inspect
import types

import numpy as np
import pytest
import torch

from sota_imagenet_amd import native, ops

F32, F64, I32, I64, U8, BF16 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bfloat16
N, H, W, C = 1, 4, 4, 64
XS = (N, H, W, C)

# wrappers that take no tensor: nothing for the contract to test
EXEMPT = {
    "last_conv_kernel": "no argument", "lw_item_elems": "no argument", "adais_workspace_elems": "an integer", "absbin_edges": "no argument",
    "absbin_log10_limits": "no argument", "tbbin_edges": "no argument", "ortho_loss_scratch": "sizes and a device: it allocates",
    "norm_loss_scratch": "sizes and a device: it allocates", "spectral_scratch": "reads two sizes and a device: it allocates",
    "keep_scale": "sizes and a device: it allocates", "wnorm_check_items": "a host list",
}
CROP = np.dtype([("raw", "u1", (40,))])
AUG = np.dtype([("color", "f4", (12,)), ("blur_sigma", "f4"), ("rest", "u1", (76,))])


def z(dtype, *shape):
    return torch.zeros(shape, dtype=dtype)


def act(*shape):
    return z(BF16, *shape)


def f(*shape):
    return z(F32, *shape)


def tab(cols=2, dtype=I64):
    return z(dtype, 1, cols)


def flat4(*names, n=8):
    return {k: f(n) for k in names}


def ol_tables():
    return dict(mats=tab(4), tiles=tab(2), items=tab(1), gitems=tab(2))


ROWS = {}


def row(name, build, free="", rank="", opt="", calls=None, null_ok=""):
    """build() -> the keyword arguments of a valid call.  free: tensor arguments whose extent the contract leaves open (one element fewer is
    still legal); rank: those whose rank it fixes (one more dimension is not); opt: those that may be None; calls: the entry points the valid
    call reaches (default mi355_<name>); null_ok: C parameters that are null in it"""
    ROWS[name] = types.SimpleNamespace(fn=getattr(ops, name.split("[")[0]), build=build, free=set(free.split()), rank=set(rank.split()),
                                       opt=set(opt.split()), calls=calls or ["mi355_" + name], null_ok=set(null_ok.split()))


def xpad():
    return z(U8, ops._L().mi355_stem_xpad_bytes(native.BF16, N, H, W))


row("conv2d_fwd", lambda: dict(x=act(*XS), w=act(C, 1, 1, C)), rank="x w")
row("conv2d_fwd[stats]", lambda: dict(x=act(*XS), w=act(C, 1, 1, C), stats=True), rank="x w", calls=["mi355_conv2d_fwd_stats"])
row("conv2d_fwd_bn_in", lambda: dict(y_in=act(*XS), scale=f(C), shift=f(C), w=act(C, 3, 3, C)), rank="y_in w")
row("quantize_fp8", lambda: dict(x=f(8)), free="x")
row("conv2d_fwd_fp8", lambda: dict(xq=z(U8, *XS), wq=z(U8, C, 1, 1, C)), rank="xq wq")
row("conv2d_dgrad_fp8", lambda: dict(dyq=z(U8, *XS), wq=z(U8, C, 1, 1, C), x_shape=XS), rank="dyq wq", opt="wt")
row("conv2d_wgrad_fp8", lambda: dict(dyq=z(U8, *XS), xq=z(U8, *XS), KH=1, KW=1), rank="dyq xq")
row("ingest_u8", lambda: dict(packed=z(U8, 48), table_host=np.zeros(1, CROP), table_dev=z(U8, 40), S=4), free="packed", opt="aug_dev")
row("ingest_u8[aug]", lambda: dict(packed=z(U8, 48), table_host=np.zeros(1, CROP), table_dev=z(U8, 40), S=4, aug_host=np.zeros(1, AUG), aug_dev=z(U8, 128)),
    free="packed", calls=["mi355_ingest_u8_aug"], null_ok="scratch")
row("conv2d_dgrad", lambda: dict(dy=act(*XS), w=act(C, 1, 1, C), x_shape=XS), rank="dy w", opt="addend", null_ok="addend")
row("conv2d_dgrad_bn", lambda: dict(dy=act(*XS), w=act(C, 1, 1, C), x_shape=XS), rank="dy w", opt="addend addend_bits bn_y bn_bits bn_mean bn_invstd",
    calls=["mi355_conv2d_dgrad_bn_leaky"], null_ok="addend addend_bits bn_y bn_bits bn_mean bn_invstd partial")
row("conv2d_dgrad_bn[bn]", lambda: dict(dy=act(*XS), w=act(C, 1, 1, C), x_shape=XS, addend=act(*XS), addend_bits=z(U8, N, H, W, C // 8), bn_y=act(*XS),
                                        bn_bits=z(U8, N, H, W, C // 8), bn_mean=f(C), bn_invstd=f(C)),
    rank="dy w addend addend_bits bn_y bn_bits", opt="addend addend_bits bn_y bn_bits bn_mean bn_invstd", calls=["mi355_conv2d_dgrad_bn_leaky"])
row("conv2d_wgrad", lambda: dict(dy=act(*XS), x=act(*XS), KH=1, KW=1), rank="dy x", opt="dw")
row("stem_ingest", lambda: dict(x_nchw=f(N, 3, H, W), dtype=BF16), rank="x_nchw")
row("stem_fwd", lambda: dict(xpad=xpad(), w=f(64, 7, 7, 3), N=N, H=H, W=W, dtype=BF16), rank="w")
row("stem_wgrad", lambda: dict(dy=act(N, H // 2, W // 2, 64), xpad=xpad(), N=N, H=H, W=W), rank="dy")
row("bn_fwd_train", lambda: dict(x=act(*XS), gamma=f(C), beta=f(C), running_mean=f(C), running_var=f(C)), free="x",
    opt="running_mean running_var residual stats", null_ok="residual")
row("bn_fwd_train[stats]", lambda: dict(x=act(*XS), gamma=f(C), beta=f(C), running_mean=f(C), running_var=f(C), residual=act(*XS), stats=f(1, 2, C)),
    free="x", rank="residual stats", opt="running_mean running_var residual stats", calls=["mi355_bn_fwd_train_partial"])
row("bn_fwd_eval", lambda: dict(x=act(*XS), gamma=f(C), beta=f(C), running_mean=f(C), running_var=f(C)), free="x", opt="residual", null_ok="residual")
row("bn_bwd", lambda: dict(dout=act(*XS), out=act(*XS), x=act(*XS), gamma=f(C), save_mean=f(C), save_invstd=f(C)), free="x", rank="dout out",
    opt="dgamma dbeta", null_ok="dz_out")
row("bn_apply", lambda: dict(x=act(*XS), scale=f(C), shift=f(C)), free="x", opt="residual x2 scale2 shift2", null_ok="residual x2 scale2 shift2 bits")
row("bn_bwd_bits", lambda: dict(g=act(*XS), bits=z(U8, N * H * W * C // 8), x=act(*XS), gamma=f(C), mean=f(C), invstd=f(C), dgamma=f(C), dbeta=f(C)),
    free="x", rank="g", opt="bits dx dz_out dgamma dbeta partial", null_ok="dz_out partial")
row("maxpool_fwd", lambda: dict(x=act(*XS)), rank="x")
row("maxpool_bwd", lambda: dict(dy=act(N, 2, 2, C), idx=z(U8, N, 2, 2, C), x_shape=XS), rank="dy idx")
row("bn_relu_maxpool", lambda: dict(y=act(*XS), scale=f(C), shift=f(C)), rank="y")
row("stem_bwd", lambda: dict(dp=act(N, 2, 2, C), idx=z(U8, N, 2, 2, C), bits=z(U8, N, H, W, C // 8), y=act(*XS), gamma=f(C), mean=f(C), invstd=f(C)),
    rank="dp idx bits y", opt="dgamma dbeta")
row("gap_fwd", lambda: dict(x=act(*XS)), rank="x")
row("gap_bwd", lambda: dict(dpooled=f(N, C), x_shape=XS, dtype=BF16), rank="dpooled")
row("ce_loss", lambda: dict(logits=f(1, 4), target=f(1, 4)), rank="logits target")
row("sgd_step", lambda: dict(**flat4("p", "g", "m"), lr=0.1), free="p", opt="ema")
row("adam_step", lambda: dict(**flat4("p", "g", "m", "v"), step=0, lr=0.1), free="p", opt="ema")
row("madgrad_step", lambda: dict(**flat4("p", "g", "grad_sum_sq", "s", "x0"), k=0, lr=0.1), free="p", opt="ema")
row("adais_step", lambda: dict(**flat4("p", "g", "m", "v", "beta1_prod"), mean=f(1), step=1, lr=0.1), free="p", opt="ema")
row("lw_update", lambda: dict(rule=0, **flat4("p", "g", "m"), items=tab(), coef=f(1, 4), lr=0.1), free="p", rank="items coef", opt="ema")
row("lw_unit_update", lambda: dict(rule=0, **flat4("p", "g", "m"), items=tab(), tensors=tab(), den=f(1), beta1=0.9, lr=0.1, weight_decay=0.0), free="p",
    rank="items tensors den", opt="ema")
row("adamp_update", lambda: dict(**flat4("p", "g", "m", "v"), items=tab(), tensors=tab(), coef=f(1, 2), wdf=f(1), step=1, lr=0.1), free="p",
    rank="items tensors coef wdf", opt="ema")
row("adais_moments", lambda: dict(**flat4("g", "v"), step=1, beta2=0.99, workspace=z(F64, ops.adais_workspace_elems(8))), free="v")
row("adais_mean", lambda: dict(workspace=z(F64, 1), param_size=8, mean=f(1)), rank="workspace")
row("lw_sumsq", lambda: dict(src=f(8), items=tab(), partial=z(F64, 1), n_tensors=1), free="src", rank="items")
row("lw_coef", lambda: dict(rule=0, flags=0, partial=z(F64, 1), tensors=tab(), v=f(1), coef=f(1, 4), sums=z(F64, 1), beta1=0.9, beta2=0.99, eps=1e-8, lr=0.1,
                            weight_decay=0.0), rank="partial tensors")
row("lw_unit_sumsq", lambda: dict(src=f(8), pieces=tab(), partial=z(F64, 1), n_slots=1), free="src", rank="pieces")
row("lw_unit_coef", lambda: dict(partial=z(F64, 1), slots=tab(2, I32), v=f(1), den=f(1), sums=z(F64, 1), beta2=0.99, eps=1e-8), rank="partial slots")
row("adamp_unit_sums", lambda: dict(**flat4("p", "g", "m", "v"), pieces=tab(), partial=z(F64, 1, 4), n_slots=1, step=1), free="p", rank="pieces")
row("adamp_coef", lambda: dict(partial=z(F64, 1, 4), slots=tab(2, I32), decide=tab(4, I32), coef=f(1, 2), wdf=f(1), mode=z(I32, 1), lr=0.1, weight_decay=0.0),
    rank="partial slots decide coef wdf")
row("sam_sumsq", lambda: dict(**flat4("p", "g"), items=tab(), kind=z(I32, 1), partial=z(F64, 1), eta=0.01), free="p", rank="items kind")
row("sam_scale", lambda: dict(partial=z(F64, 1), rho=0.05, out=f(2)), rank="partial")
row("sam_perturb", lambda: dict(**flat4("p", "g", "eps"), items=tab(), kind=z(I32, 1), out=f(2), eta=0.01), free="p", rank="items kind")
row("sam_restore", lambda: dict(**flat4("p", "eps"), items=tab(), n_tensors=1), free="p", rank="items")
row("sam_lw_sumsq", lambda: dict(**flat4("p", "g"), items=tab(), partial=z(F64, 2), n_tensors=1), free="p", rank="items")
row("sam_unit_sumsq", lambda: dict(**flat4("p", "g"), pieces=tab(), partial=z(F64, 2), n_slots=1), free="p", rank="pieces")
row("sam_lw_coef", lambda: dict(partial=z(F64, 2), slots=tab(2, I32), coef=f(1), norms=f(2)), free="partial", rank="partial slots coef")
row("sam_lw_perturb", lambda: dict(**flat4("p", "g", "eps"), items=tab(), tensors=tab(), coef=f(1), rho=0.05), free="p", rank="items tensors coef")
row("ortho_init_", lambda: dict(flat=f(16), records_host=[(0, 2, 2, 1)], records_dev=tab(3)), free="flat", rank="records_dev", calls=["mi355_ortho_init"])
row("weight_norm_rows_", lambda: dict(flat=f(16), items_host=[(0, 4, 2)], items_dev=tab()), free="flat", rank="items_dev", calls=["mi355_weight_norm_rows"])
row("weight_std_rows_fwd", lambda: dict(**flat4("w", "w_hat", n=16), invstd=f(1), rows_dev=tab(), mode=ops.WS_STANDARDISE), free="w", rank="rows_dev")
row("weight_std_rows_bwd", lambda: dict(**flat4("g", "w_hat", "dw", n=16), invstd=f(1), rows_dev=tab(), mode=ops.WS_STANDARDISE), free="g", rank="rows_dev")
row("spectral_fwd", lambda: dict(**flat4("w", "w_hat", n=16), u=f(1), v=f(1), sigma=f(1), scratch=ops.spectral_scratch(f(1), f(1)), mats_dev=tab(4), iters=1),
    free="w", rank="u v mats_dev", opt="w_hat")
row("spectral_bwd", lambda: dict(**flat4("g", "w_hat", "dw", n=16), u=f(1), v=f(1), sigma=f(1), scratch=ops.spectral_scratch(f(1), f(1)), mats_dev=tab(4)),
    free="g", rank="u v mats_dev")
row("ortho_loss_fwd", lambda: dict(w=f(16), tables=ol_tables(), scratch=ops.ortho_loss_scratch(4, 1, 1, 1, "cpu"), min_norm=0.0), free="w gram",
    rank="mats tiles items gitems gram")
row("ortho_loss_bwd", lambda: dict(w=f(16), dw=f(16), tables=ol_tables(), scratch=ops.ortho_loss_scratch(4, 1, 1, 1, "cpu"), s=f(1)), free="w gram",
    rank="mats tiles items gitems gram")
row("norm_loss_fwd", lambda: dict(w=f(16), items_dev=tab(), tensors_dev=tab(), scratch=ops.norm_loss_scratch(1, 1, "cpu")), free="w",
    rank="items_dev tensors_dev")
row("norm_loss_bwd", lambda: dict(w=f(16), dw=f(16), items_dev=tab(), tensors_dev=tab(), s=f(1)), free="w", rank="items_dev tensors_dev")
row("absbin_hist", lambda: dict(src=f(8), items=tab(), hist=z(I32, 1, ops.ABSBIN_BINS)), free="src", rank="items hist")
row("subsample_counts", lambda: dict(hist=z(I32, 1, ops.ABSBIN_BINS), rep=z(I32, 1), subsample=1, counts=z(I64, ops.ABSBIN_BINS)), rank="hist rep counts")
row("tbbin_hist", lambda: dict(src=f(8), items=tab(), hist=z(I32, 1, ops.TBBIN_ROW), partial=z(F64, 1, ops.TBBIN_STATS)), free="src", rank="items hist partial")
row("blurpool_fwd", lambda: dict(x=act(*XS)), rank="x")
row("blurpool_bwd", lambda: dict(dy=act(N, 2, 2, C), x_shape=XS), rank="dy")
row("avgpool2_fwd", lambda: dict(x=act(*XS)), rank="x")
row("avgpool2_bwd", lambda: dict(dy=act(N, 2, 2, C), x_shape=XS), rank="dy")
row("maxpool3s1_fwd", lambda: dict(x=act(*XS)), rank="x")
row("maxpool3s1_bwd", lambda: dict(dy=act(*XS), idx=z(U8, *XS)), rank="dy idx")
row("eca_fwd", lambda: dict(x=act(*XS), w=f(3)), free="w", rank="x")
row("eca_bwd", lambda: dict(dy=act(*XS), x=act(*XS), w=f(3), pooled=f(N, C), gate=f(N, C)), free="w", rank="dy x pooled gate", opt="dw")
row("weight_std_fwd", lambda: dict(w=f(2, 8)), free="w")
row("weight_std_bwd", lambda: dict(dw_hat=f(2, 8), w_hat=f(2, 8), invstd=f(2)), free="w_hat", opt="dw")
row("residual_act_fwd", lambda: dict(branch=act(*XS)), free="branch", opt="shortcut scale_n", null_ok="scale_n shortcut")
row("residual_act_bwd", lambda: dict(dout=act(*XS), out=act(*XS)), free="out", rank="dout", opt="scale_n", null_ok="scale_n")
EMA = ("sgd_step", "adam_step", "madgrad_step", "adais_step", "lw_update", "lw_unit_update", "adamp_update")


def test_every_public_wrapper_has_a_row():
    public = {n for n, fn in vars(ops).items() if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not n.startswith("_")}
    rows = {n.split("[")[0] for n in ROWS}
    assert rows | set(EXEMPT) == public and not rows & set(EXEMPT), (public - rows - set(EXEMPT), (rows | set(EXEMPT)) - public)
    assert all(EXEMPT.values())


# ---- the library behind a proxy: sizing calls go through, everything else is recorded and not made ----------------------------------------------
class Recorder:
    PURE = ("_bytes", "_elems", "_doubles", "_floats")

    def __init__(self):
        self.calls, self.lib = [], native.lib()

    def __getattr__(self, name):
        if name.endswith(self.PURE):
            return getattr(self.lib, name)
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(ops, "_L", lambda: rec)
    return rec


def slots(kw):
    """the tensor arguments of a call: [(name, the dict that holds it)], the members of `tables` and `scratch` by their own names"""
    out = []
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            out.append((k, kw))
        elif isinstance(v, dict):
            out.extend((kk, v) for kk, vv in v.items() if isinstance(vv, torch.Tensor))
    return out


def with_(kw, name, holder, value):
    """the call with one tensor argument replaced"""
    if holder is kw:
        return {**kw, name: value}
    return {k: ({**v, name: value} if v is holder else v) for k, v in kw.items()}


def strided(t):
    """t's shape and dtype as every second element of a buffer twice as long, or None where no extent is 2 or more"""
    for d, n in enumerate(t.shape):
        if n >= 2:
            big = torch.zeros(t.shape[:d] + (2 * n,) + t.shape[d + 1:], dtype=t.dtype)
            view = big[(slice(None),) * d + (slice(None, None, 2),)]
            assert view.shape == t.shape and not view.is_contiguous()
            return view
    return None


def mutations(r, name, t):
    yield "dtype", t.to(F32 if t.dtype == F64 else F64)
    if name not in r.free:
        yield "one element short", t.reshape(-1)[:-1].clone()
    if name in r.rank:
        yield "one more dimension", t.unsqueeze(0)
    if strided(t) is not None:
        yield "not contiguous", strided(t)
    if name not in r.opt:
        yield "None", None


# ---- (a) the unpatched module -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROWS))
def test_a_valid_cpu_call_is_refused_for_its_placement_alone(name, recorder):
    r = ROWS[name]
    with pytest.raises(ValueError, match=r"must be a CUDA \(ROCm\) tensor") as e:
        r.fn(**r.build())
    assert name.split("[")[0] + ":" in str(e.value) and recorder.calls == []


@pytest.mark.parametrize("name", list(ROWS))
def test_each_malformed_tensor_is_refused_by_name(name, recorder):
    r, who = ROWS[name], name.split("[")[0]
    kw = r.build()
    tried = 0
    for arg, holder in slots(kw):
        for what, bad in mutations(r, arg, holder[arg]):
            with pytest.raises(ValueError) as e:
                r.fn(**with_(kw, arg, holder, bad))
            msg = str(e.value)
            assert msg.startswith(who + ": " + arg) and "must be a contiguous" in msg, (arg, what, msg)
            tried += 1
    assert tried >= 2 * len(slots(kw)) and recorder.calls == []


def test_the_order_of_the_two_tests_is_form_first_then_placement():
    with pytest.raises(ValueError, match="sgd_step: g must be a contiguous torch.float32 tensor of 8 elements, got torch.float64"):
        ops.sgd_step(f(8), z(F64, 8), f(8), 0.1)
    with pytest.raises(ValueError, match=r"lw_sumsq: items must be a contiguous torch.int64 tensor \[n, 2\], got torch.int64 \(0, 2\)"):
        ops.lw_sumsq(f(8), z(I64, 0, 2), z(F64, 1), 1)
    with pytest.raises(ValueError, match="sgd_step: ema must be a contiguous"):  # no assert that python -O would drop
        ops.sgd_step(f(8), f(8), f(8), 0.1, ema=f(7))
    with pytest.raises(ValueError, match="conv2d_fwd: w must be .* 64\\], got torch.bfloat16 \\(64, 1, 1, 32\\)"):  # w.shape[3] is Cin
        ops.conv2d_fwd(act(*XS), act(C, 1, 1, 32))
    with pytest.raises(ValueError, match="conv2d_dgrad: dy must be"):  # dy is the conv's output shape
        ops.conv2d_dgrad(act(N, H, W - 1, C), act(C, 1, 1, C), XS)


# ---- _on_device itself --------------------------------------------------------------------------------------------------------------------------
class OnDevice:
    """a CPU tensor that says it lives on a device (tests/test_grad_dist_host.py::_FakeCuda, with a .device)"""
    is_cuda = True

    def __init__(self, t, index):
        self.t, self.device = t, torch.device("cuda", index)

    def __getattr__(self, k):
        return getattr(self.t, k)


def test_on_device_names_the_tensor_that_is_elsewhere():
    a, b, c = OnDevice(f(1), 0), OnDevice(f(1), 0), OnDevice(f(1), 1)
    assert ops._on_device("op", "x skipped y", a, None, b) == torch.device("cuda", 0)
    with pytest.raises(ValueError, match="op: y lives on cuda:1, the arguments before it on cuda:0"):
        ops._on_device("op", "x y z", a, c, b)
    with pytest.raises(ValueError, match="op: z lives on cuda:0, the arguments before it on cuda:1"):
        ops._on_device("op", "x y z", c, None, b)
    with pytest.raises(ValueError, match=r"op: y must be a CUDA \(ROCm\) tensor, got one on cpu"):
        ops._on_device("op", "x y", a, f(1))


@pytest.mark.parametrize("name", list(ROWS))
def test_every_tensor_of_a_wrapper_goes_to_on_device(name, recorder, monkeypatch):
    """so the direct test above holds for every wrapper: _on_device is called once, with ALL the tensors of the call under their names"""
    r, seen = ROWS[name], []

    def spy(who, names, *ts):
        assert len(names.split()) >= len(ts)
        seen.append((who, dict(zip(names.split(), ts))))
        raise ValueError("seen")

    monkeypatch.setattr(ops, "_on_device", spy)
    kw = r.build()
    with pytest.raises(ValueError, match="seen"):
        r.fn(**kw)
    (who, named), = seen
    given = {k: holder[k] for k, holder in slots(kw)}
    assert who == name.split("[")[0] and {k for k, t in named.items() if t is not None} == set(given)
    assert all(named[k] is t for k, t in given.items()) and recorder.calls == []


# ---- (b) the placement test patched out ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def placed(monkeypatch, recorder):
    monkeypatch.setattr(ops, "_on_device", lambda who, names, *ts: torch.device("cpu"))
    monkeypatch.setattr(ops, "cur_stream", lambda: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))  # the key of conv2d_wgrad_fp8's cache
    monkeypatch.setattr(ops, "_WGRAD_WS", {})
    return recorder


def params(entry):
    """the C parameter names of an entry point, and which of them are pointers"""
    decls = native.prototypes()[entry][1]
    return [d.replace("*", " ").replace("[", " ").split()[-1] if "[" not in d else d.split("[")[0].split()[-1] for d in decls], ["*" in d or "[" in d for d in decls]


def is_null(a):
    return a is None or a == 0 or (isinstance(a, ctypes.c_void_p) and not a.value)


def check_calls(r, calls):
    assert [c for c, _ in calls] == r.calls
    for entry, args in calls:
        names, pointer = params(entry)
        assert len(args) == len(names), (entry, len(args), names)
        null = {n for n, a, p in zip(names, args, pointer) if p and is_null(a)} - {"stream"}
        assert null <= r.null_ok, (entry, null)


@pytest.mark.parametrize("name", list(ROWS))
def test_the_valid_call_reaches_its_entry_points(name, placed):
    r = ROWS[name]
    r.fn(**r.build())
    check_calls(r, placed.calls)


def plain(a):
    return a.value if isinstance(a, ctypes.c_void_p) else a


@pytest.mark.parametrize("name", EMA)
def test_the_ema_twin_takes_the_same_arguments_and_the_two_of_the_average(name, placed):
    r = ROWS[name]
    kw = r.build()
    r.fn(**kw)
    ema = f(8)
    r.fn(**kw, ema=ema, ema_decay=0.75)
    (e0, a0), (e1, a1) = placed.calls
    assert (e0, e1) == ("mi355_" + name, "mi355_" + name + "_ema")
    n0, n1 = params(e0)[0], params(e1)[0]
    assert len(a0) == len(n0) and len(a1) == len(n1) and [n for n in n1 if n not in ("ema", "ema_decay")] == n0
    i, j = n1.index("ema"), n1.index("ema_decay")
    assert plain(a1[i]) == ema.data_ptr() and a1[j] == 0.75
    assert [plain(a) for k, a in enumerate(a1) if k not in (i, j)] == [plain(a) for a in a0]
    with pytest.raises(ValueError, match=name + ": ema must be a contiguous"):
        r.fn(**kw, ema=f(8).double())
