"""The C-ABI library loads on a GPU-less host, exports every symbol include/mi355rn.h declares, and fails loudly
(status + message, no crash, no CPU fallback) when asked to compute without a device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from sota_imagenet_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_symbols_are_exported():
    protos = native.parse_header()
    assert len(protos) >= 35
    out = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(mi355_\w+)", out))
    assert set(protos) <= exported, sorted(set(protos) - exported)
    assert exported <= set(protos), f"exported but undeclared: {sorted(exported - set(protos))}"
    # no torch types leak into the signatures
    for name, (ret, params) in protos.items():
        for p in params:
            assert "Tensor" not in p and "at::" not in p and "torch" not in p, (name, p)


def test_library_is_built_for_gfx950():
    out = subprocess.run(["strings", "-n", "6", native.LIB_PATH], capture_output=True, text=True).stdout
    assert "gfx950" in out


# (model, extra create arguments, forward / training GFLOP per image at 224 px, tensors in the table, a forward's arguments after ctx)
LAYOUT_ONLY = [("resnet50", (), 8.178, 24.30, 161 + 106, (None, None, 1, 0.1, None)),  # 8.178 / 24.30 GFLOP per image
               ("bresnet50", (1,), 10.739, 32.02, 183 + 110, (None, None, 1, 0.1, 0, None, None, None))]


@pytest.mark.parametrize("model,extra,gf_fwd,gf_train,ntensors,fwd_args", LAYOUT_ONLY, ids=[m[0] for m in LAYOUT_ONLY])
def test_layout_only_context_and_param_table(model, extra, gf_fwd, gf_train, ntensors, fwd_args):
    L = native.lib()
    fn = lambda name: getattr(L, f"mi355_{model}_{name}")  # noqa: E731
    assert L.mi355_version() >= 100
    ctx = ctypes.c_void_p()
    native.check(fn("create")(ctypes.byref(ctx), -1, native.F32, 256, 224, 224, 1000, *extra))
    try:
        f, t = ctypes.c_double(), ctypes.c_double()
        native.check(fn("flops")(ctx, ctypes.byref(f), ctypes.byref(t)))
        assert abs(f.value / 256 / 1e9 - gf_fwd) < 2e-3 and abs(t.value / 256 / 1e9 - gf_train) < 5e-3
        assert fn("num_segments")(ctx) == 18
        assert fn("num_tensors")(ctx) == ntensors
        # layout-only contexts refuse to compute, and to be bound (MI355_E_STATE)
        rc = fn("forward")(ctx, *fwd_args)
        assert rc != 0 and native.last_error()
        buf = (ctypes.c_float * 64)()
        rc = fn("bind")(ctx, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p))
        assert rc == -3 and "layout-only" in native.last_error()
    finally:
        fn("destroy")(ctx)


def test_bad_arguments_return_status_not_crash():
    L = native.lib()
    rc = L.mi355_resnet50_create(None, -1, 0, 1, 32, 32, 10)
    assert rc == -1 and "null" in native.last_error()
    ctx = ctypes.c_void_p()
    assert L.mi355_resnet50_create(ctypes.byref(ctx), -1, 7, 1, 32, 32, 10) == -1  # bad dtype
    assert L.mi355_resnet50_create(ctypes.byref(ctx), -1, 0, 1, 33, 32, 10) == -1  # H not a multiple of 32
    assert L.mi355_conv2d_fwd(0, None, None, None, 1, 8, 8, 60, 64, 3, 3, 1, 1, None) == -1  # Cin % 64
    assert "Cin" in native.last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-side refusal, called with dummy pointers: never sent to a GPU")
@pytest.mark.parametrize("dtype", [7, native.FP8])
def test_elementwise_entry_points_refuse_a_dtype_outside_their_set(dtype):
    """The launchers directly behind the C-ABI accept MI355_F32 and MI355_BF16 only: any other code (a stray integer, or MI355_FP8, which other
    calls do take) is refused with MI355_E_ARG before anything is launched — not run as the bf16 instance over a grid sized for fp32."""
    L = native.lib()
    p = torch.zeros(64).data_ptr()  # non-null, never dereferenced
    N, H, W, C, HW = 1, 8, 8, 64, 64
    calls = {"mi355_stem_ingest": (dtype, p, p, N, H, W, None),
             "mi355_maxpool_fwd": (dtype, p, p, p, N, H, W, C, None),
             "mi355_maxpool_bwd": (dtype, p, p, p, N, H, W, C, None),
             "mi355_gap_fwd": (dtype, p, p, N, HW, C, None),
             "mi355_gap_bwd": (dtype, p, p, N, HW, C, None),
             "mi355_bn_relu_maxpool": (dtype, p, p, p, p, p, p, N, H, W, C, 0, None),
             "mi355_stem_bwd": (dtype, p, p, p, p, p, p, p, p, p, p, 0.0, N, H, W, C, p, 1 << 30, None),
             "mi355_bn_fwd_train": (dtype, p, p, p, p, p, p, p, p, p, HW, C, 1e-5, 0.1, 1, p, 1 << 30, None),
             "mi355_bn_fwd_train_partial": (dtype, p, p, p, p, p, p, p, p, p, HW, C, 1e-5, 0.1, 1, p, 1, p, 1 << 30, None),
             "mi355_bn_fwd_eval": (dtype, p, p, p, p, p, p, p, HW, C, 1e-5, 1, p, 1 << 30, None),
             "mi355_bn_bwd": (dtype, p, p, p, p, p, p, p, p, p, p, 0.0, HW, C, 1, p, 1 << 30, None),
             "mi355_bn_apply": (dtype, p, p, p, None, None, None, None, p, p, HW, C, 1, None),
             "mi355_bn_bwd_bits": (dtype, p, p, p, p, p, p, p, None, p, p, 0.0, HW, C, 1, p, 1, p, 1 << 30, None)}
    for name, args in calls.items():
        rc = getattr(L, name)(*args)
        assert rc == -1 and "dtype" in native.last_error(), (name, rc, native.last_error())


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-side refusal, called with dummy pointers: never sent to a GPU")
def test_stem_tail_entry_points_refuse_what_their_kernels_cannot_run():
    """A forced form of the fused BN + ReLU + max pool that the shape or dtype does not allow is MI355_E_ARG before any launch — never another form in
    its place; the stem backward keeps its launchers' refusals (64 channels, even H and W, 32-bit buffer offsets)."""
    L = native.lib()
    p = torch.zeros(64).data_ptr()  # non-null, never dereferenced

    def pool(dtype, H, W, form, C=64):
        return L.mi355_bn_relu_maxpool(dtype, p, p, p, p, p, p, 2, H, W, C, form, None)

    def bwd(dtype, N, H, W, C):
        return L.mi355_stem_bwd(dtype, p, p, p, p, p, p, p, p, p, p, 0.0, N, H, W, C, p, 1 << 30, None)

    for dtype in (native.F32, native.BF16):
        for H, W in ((4, 6), (6, 4), (6, 10)):  # an odd pooled height or width: one thread per window is the only form
            for form in (2, 3):
                assert pool(dtype, H, W, form) == -1 and "form %d" % form in native.last_error(), (dtype, H, W, form, native.last_error())
        for form in (-1, 4):
            assert pool(dtype, 8, 8, form) == -1 and "outside 0..3" in native.last_error()
        assert pool(dtype, 7, 8, 0) == -1 and "H=7" in native.last_error()
        assert pool(dtype, 8, 8, 1, C=60) == -1 and "C=60" in native.last_error()
        assert bwd(dtype, 2, 8, 8, 128) == -1 and "64 channels" in native.last_error()
        assert bwd(dtype, 2, 7, 8, 64) == -1 and "H=7" in native.last_error()
        assert bwd(dtype, 2, 8, 6 + 1, 64) == -1 and "W=7" in native.last_error()
    assert pool(native.F32, 8, 8, 3) == -1 and "bf16 only" in native.last_error()  # packed keys
    assert bwd(native.F32, 1024, 128, 128, 64) == -1 and "32-bit offsets" in native.last_error()  # 2^32 bytes
    assert bwd(native.BF16, 2048, 128, 128, 64) == -1 and "32-bit offsets" in native.last_error()
    assert L.mi355_bn_relu_maxpool(native.F32, None, p, p, p, p, p, 2, 8, 8, 64, 0, None) == -1 and "null" in native.last_error()
    assert L.mi355_stem_bwd(native.F32, p, p, p, p, p, p, p, p, p, p, 0.0, 2, 8, 8, 64, p, 16, None) == -1 and "workspace" in native.last_error()


def test_bn_per_op_prototypes():
    """the two per-op BatchNorm calls that mirror the executors' bn_apply / bn_backward: argument order and types, as tests/test_bn_gpu.py and ops.py
    pass them"""
    protos = native.parse_header()
    norm = lambda ps: [re.sub(r"\s+", " ", q) for q in ps]  # noqa: E731
    assert protos["mi355_bn_apply"][0] == "int" and norm(protos["mi355_bn_apply"][1]) == [
        "int dtype", "const void* x", "const float* scale", "const float* shift", "const void* residual", "const void* x2", "const float* scale2",
        "const float* shift2", "void* out", "uint8_t* bits", "int M", "int C", "int relu", "void* stream"]
    assert protos["mi355_bn_bwd_bits"][0] == "int" and norm(protos["mi355_bn_bwd_bits"][1]) == [
        "int dtype", "const void* g", "const uint8_t* bits", "const void* x", "const float* gamma", "const float* mean", "const float* invstd",
        "void* dx", "void* dz_out", "float* dgamma", "float* dbeta", "float beta_acc", "int M", "int C", "int relu", "const float* partial", "int nblk",
        "void* ws", "size_t ws_bytes", "void* stream"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="host-side refusal, called with dummy pointers: never sent to a GPU")
def test_bn_entry_points_refuse_before_any_launch():
    """Every BatchNorm entry point refuses a null required pointer and M < 1 (M = 0 would divide by zero in the finalize); the two per-op calls refuse the
    combinations their kernels do not have — never silently another form.  All MI355_E_ARG with a message, before anything is launched."""
    L = native.lib()
    p = torch.zeros(64).data_ptr()  # non-null, never dereferenced
    C, BIG = 64, 1 << 30

    def refused(rc, word):
        assert rc == -1 and word in native.last_error(), (rc, word, native.last_error())

    calls = {  # name -> (arguments as a list, indices of the required pointers, index of M)
        "mi355_bn_fwd_train": ([native.F32, p, None, p, p, p, p, p, p, p, 8, C, 1e-5, 0.1, 1, p, BIG, None], (1, 3, 4, 5, 8, 9), 10),
        "mi355_bn_fwd_train_partial": ([native.F32, p, None, p, p, p, p, p, p, p, 8, C, 1e-5, 0.1, 1, p, 1, p, BIG, None], (1, 3, 4, 5, 8, 9), 10),
        "mi355_bn_fwd_eval": ([native.F32, p, None, p, p, p, p, p, 8, C, 1e-5, 1, p, BIG, None], (1, 3, 4, 5, 6, 7), 8),
        "mi355_bn_bwd": ([native.F32, p, p, p, p, p, p, p, None, p, p, 0.0, 8, C, 1, p, BIG, None], (1, 2, 3, 4, 5, 6, 7, 9, 10), 12),
        "mi355_bn_apply": ([native.F32, p, p, p, None, None, None, None, p, None, 8, C, 1, None], (1, 2, 3, 8), 10),
        "mi355_bn_bwd_bits": ([native.F32, p, p, p, p, p, p, p, None, p, p, 0.0, 8, C, 1, None, 0, p, BIG, None], (1, 3, 4, 5, 6, 7, 9, 10), 12),
    }
    for name, (args, required, m_at) in calls.items():
        fn = getattr(L, name)
        for i in required:
            a = list(args)
            a[i] = None
            refused(fn(*a), "null pointer")
        for M in (0, -3):
            a = list(args)
            a[m_at] = M
            refused(fn(*a), f"M={M}")
        a = list(args)
        a[m_at + 1] = 96  # C
        refused(fn(*a), "C=96")
    # a running mean without a running variance
    a = list(calls["mi355_bn_fwd_train"][0])
    a[6] = None
    refused(L.mi355_bn_fwd_train(*a), "null pointer")

    def apply(relu, residual=None, x2=None, sc2=None, sh2=None, bits=None, dtype=native.BF16):
        return L.mi355_bn_apply(dtype, p, p, p, residual, x2, sc2, sh2, p, bits, 8, C, relu, None)

    for dtype in (native.F32, native.BF16):
        refused(apply(1, residual=p, x2=p, sc2=p, sh2=p, dtype=dtype), "residual and second branch together")
        refused(apply(2, residual=p, bits=p, dtype=dtype), "leaky bit-mask form")
        refused(apply(2, x2=p, sc2=p, sh2=p, bits=p, dtype=dtype), "leaky bit-mask form")
        refused(apply(0, bits=p, dtype=dtype), "a bit mask needs an activation")
        refused(apply(1, x2=p, sc2=None, sh2=p, dtype=dtype), "null pointer")
        for relu in (-1, 3):
            refused(apply(relu, dtype=dtype), "outside 0..2")

    def bwd(relu, bits, partial=None, nblk=0, ws_bytes=BIG):
        return L.mi355_bn_bwd_bits(native.BF16, p, bits, p, p, p, p, p, None, p, p, 0.0, 8, C, relu, partial, nblk, p, ws_bytes, None)

    refused(bwd(0, p), "relu=0 takes no bit mask")
    refused(bwd(1, None), "relu=1 needs a bit mask")
    refused(bwd(2, None), "relu=2 needs a bit mask")
    refused(bwd(3, p), "outside 0..2")
    refused(bwd(1, p, partial=p, nblk=0), "nblk=0 with partial rows")
    refused(bwd(1, p, partial=None, nblk=4), "nblk=4 without partial rows")
    refused(bwd(1, p, ws_bytes=16), "workspace")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the GPU-less failure mode")
def test_no_cpu_fallback_without_gpu():
    L = native.lib()
    assert L.mi355_device_count() == 0
    x = torch.zeros(64 * 4)
    rc = L.mi355_sgd_step(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.numel(), 0.1, 0.9, 0.0, 1.0, None)
    assert rc == -2 and "hip" in native.last_error().lower()  # MI355_E_HIP: the launch fails, nothing is computed
    assert torch.count_nonzero(x) == 0
    from sota_imagenet_amd import ops

    with pytest.raises(ValueError):
        ops.conv2d_fwd(torch.zeros(1, 8, 8, 64), torch.zeros(64, 1, 1, 64))
