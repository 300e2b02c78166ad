"""No GPU: the BatchNorm per-op tests of tests/test_bn_gpu.py can fail, and their bounds hold where they claim to.

tests/bn_common.py restates the kernels of csrc/bn.hip in fp32, in their order.  Here (1) the case tables are shown to land on every reduce layout and
every finalize form they claim, (2) the restatement runs through the very verify_* functions the GPU file uses, on every case — on exact data it must
reproduce the fp64 reference bit for bit, on random data it must stay within the derived bounds with the excluded share under its cap — and (3) errors
are planted into the restatement one at a time, each of which must break the check of the smallest case that reaches it (and none before)."""
import pytest
import torch

import bn_common as B

F32, BF16 = torch.float32, torch.bfloat16
HOST = B.HostBackend()
ids = lambda c: "-".join(str(v).replace("torch.", "") for v in (c if isinstance(c, tuple) else (c,)))  # noqa: E731


# ---- (1) the tables reach what they claim ---------------------------------------------------------------------------------------------------
def test_case_tables_reach_every_layout_and_finalize_form():
    layouts = {dt: set() for dt in B.DTYPES}
    forms = set()   # of the real reduce
    for dt, C, M in B.REDUCE_CASES + B.THRESHOLD_CASES:
        lay = B.reduce_layout(dt, M, C)
        layouts[dt].add((lay.tpr, lay.rpp, lay.gy))
        forms.add(B.fin_form(C, lay.nblk))
    # (threads per row, row lanes, workgroups across the channels) for C = 64 ... 4096
    assert layouts[F32] == {(16, 16, 1), (32, 8, 1), (64, 4, 1), (128, 2, 1), (256, 1, 1), (256, 1, 2), (256, 1, 4)}
    assert layouts[BF16] == {(8, 32, 1), (16, 16, 1), (32, 8, 1), (64, 4, 1), (128, 2, 1), (256, 1, 1), (256, 1, 2)}
    assert forms == {"four", "one"}   # the wide form needs more rows than the reduce ever writes: synthetic rows below
    L = B.reduce_layout
    assert (L(F32, 2032, 512).nblk, L(F32, 2048, 512).nblk) == (127, 128) and (B.fin_form(512, 127), B.fin_form(512, 128)) == ("four", "one")
    assert L(BF16, 32768, 64).nblk == 128 and L(BF16, 32768, 64).chain == 8 and B.fin_form(64, 128) == "one"
    for dt, C, M in ((BF16, 2048, 4100), (F32, 2048, 2100)):   # at the cap: a thread's ninth row
        lay = L(dt, M, C)
        assert lay.nblk * lay.gy == B.MAXBLK and lay.chain == 9, (dt, C, M, lay)
    assert L(F32, 33, 4096).gy == 4 and L(BF16, 33, 4096).gy == 2
    # M below the row lanes, M no multiple of a workgroup's round, one workgroup and more than one
    for dt in B.DTYPES:
        for C in B.CHANNELS:
            lays = [L(dt, M, C) for M in B.ragged_ms(dt, C)]
            assert any(M < lay.rpp for M, lay in zip(B.ragged_ms(dt, C), lays)) or lays[0].rpp == 1
            assert {1, 2} <= {lay.nblk for lay in lays}, (dt, C)
    assert L(BF16, 5, 64).rpp == 32
    # synthetic rows: every form, in one pass of its slices and in more than one
    seen = {}
    for C, nblk in B.SYNTH_CASES:
        f = B.fin_form(C, nblk)
        seen.setdefault(f, set()).add(nblk > B.fin_slices(f) * 8)
    assert seen == {"four": {False, True}, "one": {False, True}, "wide": {False, True}}, seen
    assert [B.fin_form(64, n) for n in (65, 512, 4096, 4097)] == ["four", "one", "one", "wide"]
    assert len(B.APPLY_FORMS) == 13 and len(B.BWD_FORMS) == 30


def test_exact_data_is_exact_and_has_the_edges():
    for dt, C, M in B.REDUCE_CASES + B.THRESHOLD_CASES:
        assert B.stats_sums_are_exact(B.exact_stats_data(M, C, dt).x), (dt, C, M)
        d = B.exact_bwd_data(M, C, dt)
        assert B.bwd_sums_are_exact(B.ref_bwd(d.g, d.bits, d.x, d.gamma, d.mean, d.invstd, 1)), (dt, C, M)
    for dt in B.DTYPES:
        d = B.exact_bwd_data(B.BWD_M, B.BWD_C, dt)
        for relu in (0, 1):
            assert B.bwd_dx_is_exact(B.ref_bwd(d.g, d.bits if relu else None, d.x, d.gamma, d.mean, d.invstd, relu), B.BWD_M)
        for M, C in B.APPLY_SHAPES:
            a = B.exact_apply_data(M, C, dt)
            assert a.x.dtype == dt
            for ad in B.ADDENDS:
                r = B.ref_apply(a.x, a.scale, a.shift, relu=1, **B.apply_args(a, ad))
                assert (r.a == 0).any() and not r.bits[r.a == 0].any()   # exact zeros, their bit clear
                assert (B.rounded(r.out, dt) == r.out).all()
            assert (torch.signbit(a.x.float()) & (a.x == 0)).any() and (torch.signbit(a.shift) & (a.shift == 0)).any()   # -0.0 in both addends


# ---- (2) the restatement through the GPU file's own assertions --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.REDUCE_CASES + B.THRESHOLD_CASES, ids=ids)
def test_reduce_layouts(case):
    dt, C, M = case
    for tier in ("exact", "random"):
        B.verify_stats(HOST, dt, C, M, tier)
        B.verify_bwd(HOST, dt, C, M, tier, 1)


@pytest.mark.parametrize("case", B.SYNTH_CASES, ids=ids)
def test_finalize_forms_from_synthetic_rows(case):
    C, nblk = case
    for dt in B.DTYPES:
        B.verify_stats(HOST, dt, C, B.SYNTH_M, "exact", partial_nblk=nblk)
        fig = B.verify_bwd(HOST, dt, C, B.SYNTH_M, "exact", 1, partial_nblk=nblk)
        assert fig.get("dx_exact")


def test_wrong_finalize_order_is_harmless_on_exact_data():
    """the partition is exact, so the form (the order of the fp64 sums) cannot show: what the GPU returns must not depend on it"""
    for form in B.FIN_FORMS:
        be = B.HostBackend(form=form)
        B.verify_stats(be, F32, 64, B.SYNTH_M, "exact", partial_nblk=2049)
        B.verify_bwd(be, F32, 64, B.SYNTH_M, "exact", 1, partial_nblk=2049)


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
@pytest.mark.parametrize("shape", B.APPLY_SHAPES, ids=ids)
def test_apply_forms(dtype, shape):
    M, C = shape
    for ad, relu, bits in B.APPLY_FORMS:
        for tier in ("exact", "random"):
            B.verify_apply(HOST, dtype, M, C, tier, ad, relu, bits)


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
def test_bwd_forms(dtype):
    for relu, dz, acc, alias in B.BWD_FORMS:
        if alias != "none":   # aliasing is the GPU's business
            continue
        for tier in ("exact", "random"):
            B.verify_bwd(HOST, dtype, B.BWD_C, B.BWD_M, tier, relu, dz, acc)


@pytest.mark.parametrize("dtype", B.DTYPES, ids=ids)
def test_constant_channel_and_single_row(dtype):
    for M in (1, B.CONST_M):
        for momentum in (0.1, 0.25):
            B.verify_constant(HOST, dtype, M, momentum)


def test_offset_data_bounds():
    """|mean| >> std: the pivot path within its bound; the plain-sum path within its own, far wider one, its measured loss printed (and recorded in
    bn_common.py / DESIGN.md: it documents the path)"""
    for name in B.OFFSET_CASES:
        piv, plain = B.verify_offset(HOST, name, "pivot"), B.verify_offset(HOST, name, "plain")
        print(f"{name}: relative error of invstd, pivot path {piv:.3g}, plain-sum rows {plain:.3g}")
        assert abs(plain - B.PLAIN_SUM_LOSS_MEASURED[name]) <= 0.05 * B.PLAIN_SUM_LOSS_MEASURED[name] + 1e-12, (name, plain)


# ---- (3) planted errors -----------------------------------------------------------------------------------------------------------------------
# name -> (the smallest case that reaches the error: must fail, a case just before it: must pass)
PLANTS = {
    "no_pivot": (lambda be: B.verify_offset(be, "f32_ratio100", "pivot"), lambda be: B.verify_stats(be, F32, 64, 777, "random")),
    "row_twice": (lambda be: B.verify_stats(be, F32, 64, 16 * 8 + 1, "exact"), lambda be: B.verify_stats(be, F32, 64, 16 * 8 - 1, "exact")),
    "stale_c0": (lambda be: B.verify_apply(be, F32, 33, 4096, "exact", "none", 1, True),
                 lambda be: B.verify_apply(be, F32, 777, 256, "exact", "none", 1, True)),
    "bit_shift": (lambda be: B.verify_apply(be, F32, 5, 64, "exact", "none", 1, True),
                  lambda be: B.verify_apply(be, F32, 5, 64, "exact", "none", 1, False)),
    "mask_twice": (lambda be: B.verify_bwd(be, BF16, B.BWD_C, B.BWD_M, "random", 2, dz_out=True),   # a ReLU mask is idempotent: only the leaky one shows
                   lambda be: B.verify_bwd(be, BF16, B.BWD_C, B.BWD_M, "random", 1, dz_out=True)),
    "no_beta_acc": (lambda be: B.verify_bwd(be, F32, B.BWD_C, B.BWD_M, "exact", 1, beta_acc=1.0),
                    lambda be: B.verify_bwd(be, F32, B.BWD_C, B.BWD_M, "exact", 1, beta_acc=0.0)),
    "biased_running_var": (lambda be: B.verify_stats(be, F32, 64, 2, "exact"), lambda be: B.verify_stats(be, F32, 64, 1, "exact")),
    "no_m1_guard": (lambda be: B.verify_stats(be, F32, 64, 1, "exact"), lambda be: B.verify_stats(be, F32, 64, 2, "exact")),
    "swap_k": (lambda be: B.verify_bwd(be, F32, B.BWD_C, B.BWD_M, "exact", 1), None),
}


@pytest.mark.parametrize("name", sorted(PLANTS))
def test_planted_error_breaks_its_check(name):
    fails, passes = PLANTS[name]
    be = B.HostBackend(plant={name})
    with pytest.raises(AssertionError):
        fails(be)
    fails(HOST)
    if passes is not None:
        passes(be)


@pytest.mark.parametrize("case", [(1024, 512, 513), (64, 2048, 2049), (64, 4096 * 2, 8193)], ids=ids)
def test_planted_skipped_rows_break_every_form(case):
    """a finalize that stops after its first pass of SL * 8 rows: harmless up to that many, caught one row later, forward and backward"""
    C, ok, bad = case
    be = B.HostBackend(plant={"skip_rows"})
    B.verify_stats(be, F32, C, B.SYNTH_M, "exact", partial_nblk=ok)
    B.verify_bwd(be, F32, C, B.SYNTH_M, "exact", 1, partial_nblk=ok)
    with pytest.raises(AssertionError):
        B.verify_stats(be, F32, C, B.SYNTH_M, "exact", partial_nblk=bad)
    with pytest.raises(AssertionError):
        B.verify_bwd(be, F32, C, B.SYNTH_M, "exact", 1, partial_nblk=bad)


def test_planted_row_twice_breaks_the_backward_too():
    be = B.HostBackend(plant={"row_twice"})
    with pytest.raises(AssertionError):
        B.verify_bwd(be, BF16, 64, 32 * 8 + 1, "exact", 1)
    B.verify_bwd(be, BF16, 64, 32 * 8 - 1, "exact", 1)
