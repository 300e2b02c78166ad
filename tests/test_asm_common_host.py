"""Host tests of sota_imagenet_amd/csrc/asm/asm_common.py, the vocabulary the gfx950 assembly generators share: the even merge, the counted-wait
resolver and its protocol on Emitter, the placement function under each generator's rule, and the snippet functions (instruction count as their
docstrings state it, no register named beyond the ones passed in).  Positions and counts are worked out by hand here.  No GPU needed."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sota_imagenet_amd", "csrc", "asm"))

import asm_common as A  # noqa: E402


def M(n):
    return ["m%d" % i for i in range(n)]


def G(k):
    return [["g%d" % j] for j in range(k)]


# ---- merge ---------------------------------------------------------------------------------------------------------------
def test_merge_spreads_evenly_and_keeps_the_tail():
    a = ["a0", "a1", "a2", "a3"]
    assert A.merge(a, ["b0", "b1"]) == ["a0", "a1", "b0", "a2", "a3", "b1"]          # b_i behind the first a with (i + 1) * 4 <= (a + 1) * 2
    assert A.merge(["a0", "a1"], ["b0", "b1", "b2"]) == ["a0", "b0", "a1", "b1", "b2"]
    assert A.merge(["a0"], ["b0", "b1", "b2"]) == ["a0", "b0", "b1", "b2"]
    assert A.merge([], ["b0", "b1"]) == ["b0", "b1"]                                  # nothing to spread through: all tail
    assert A.merge(a, []) == a and A.merge(a, []) is not a


# ---- resolve_waits -------------------------------------------------------------------------------------------------------
def test_resolve_waits_searches_back_cyclically():
    # the wait stands BEFORE the operation it names: steady state, that operation was issued in the previous trip; younger: C (previous trip) and A
    ev = [("op", "A", False), ("wait", "w", ["B"]), ("op", "B", False), ("op", "C", False)]
    assert A.resolve_waits(ev) == {"w": 2}


def test_resolve_waits_does_not_count_a_conditional_operation():
    ev = [("op", "A", False), ("op", "X", True), ("op", "Y", False), ("wait", "w", ["A"])]
    assert A.resolve_waits(ev) == {"w": 1}


def test_resolve_waits_takes_the_minimum_over_tags():
    ev = [("op", "A", False), ("op", "B", False), ("op", "C", False), ("wait", 0, ["A", "B"]), ("wait", 1, ["C"])]
    assert A.resolve_waits(ev) == {0: 1, 1: 0}


def test_resolve_waits_refuses_a_missing_tag_and_an_empty_wait():
    with pytest.raises(AssertionError):
        A.resolve_waits([("op", "A", False), ("wait", 0, ["B"])])
    with pytest.raises(AssertionError):
        A.resolve_waits([("op", "A", False), ("wait", 0, [])])


# ---- spread: group j of k behind MFMA first + (j * span) // k -----------------------------------------------------------
def test_spread_rule_of_dconv_and_pk():
    # span = n - first - 1
    assert A.spread(M(4), G(2)) == ["m0", "m1", "g0", "m2", "g1", "m3"]                # span 2: positions 1, 2
    assert A.spread(M(4), G(2), first=0) == ["m0", "g0", "m1", "g1", "m2", "m3"]       # span 3: positions 0, 1 (the fp8 columns)
    assert A.spread(M(4), []) == M(4)
    assert A.spread(M(2), G(3)) == ["m0", "m1", "g0", "g1", "g2"]                      # k > n: span 0, all behind MFMA 1
    assert A.spread(M(1), G(1)) == ["m0"]                                              # position 1 is no MFMA: dropped, as ever
    assert A.spread(M(3), [["x", "y"], ["z"]]) == ["m0", "m1", "x", "y", "z", "m2"]    # span 1: positions 1, 1; a group stays together


def test_spread_rule_of_po():
    # span = max(1, n - first - 1), position <= n - 1
    kw = dict(clamp=True)
    assert A.spread(M(4), G(2), **kw) == ["m0", "m1", "g0", "m2", "g1", "m3"]
    assert A.spread(M(1), G(1), **kw) == ["m0", "g0"]                                  # span 1, position 1 clamped to 0
    assert A.spread(M(2), G(3), **kw) == ["m0", "m1", "g0", "g1", "g2"]
    assert A.spread(M(3), G(4), **kw) == ["m0", "m1", "g0", "g1", "g2", "g3", "m2"]    # span 1: 1 + j // 4 = 1
    assert A.spread(M(3), G(2), first=0, **kw) == ["m0", "g0", "m1", "g1", "m2"]       # span 2: positions 0, 1
    assert A.spread(M(3), [], **kw) == M(3)


def test_spread_rule_of_wg_and_wg1():
    # span = int((n - first) * rspan / 100)
    assert A.spread(M(4), G(2), tail=0) == ["m0", "m1", "g0", "m2", "g1", "m3"]                      # span 3: positions 1, 2
    assert A.spread(M(4), G(2), tail=0, percent=50) == ["m0", "m1", "g0", "g1", "m2", "m3"]          # span 1: positions 1, 1
    assert A.spread(M(4), G(4), tail=0) == ["m0", "m1", "g0", "g1", "m2", "g2", "m3", "g3"]          # 1 + (0, 3, 6, 9) // 4
    assert A.spread(M(4), G(2), first=0, tail=0, percent=50) == ["m0", "g0", "m1", "g1", "m2", "m3"]  # span 2: positions 0, 1
    assert A.spread(M(2), G(5), tail=0) == ["m0", "m1", "g0", "g1", "g2", "g3", "g4"]                # k > n: span 1, all at 1
    assert A.spread(M(4), [], tail=0, percent=50) == M(4)


def test_spread_rule_of_pw_and_its_skip():
    # position (j * n) // k from MFMA 0 on
    kw = dict(first=0, tail=0)
    assert A.spread(M(4), G(2), **kw) == ["m0", "g0", "m1", "m2", "g1", "m3"]
    assert A.spread(M(2), G(4), **kw) == ["m0", "g0", "g1", "m1", "g2", "g3"]          # k > n: positions 0, 0, 1, 1
    assert A.spread(M(3), [], **kw) == M(3)
    g = G(4)
    assert A.spread(M(2), g, skip=[g[1]], **kw) == ["m0", "g0", "m1", "g2", "g3"]      # left out, the others where they were
    same = [["x"], ["x"]]                                                              # skip is by identity, not by value
    assert A.spread(M(2), same, skip=[same[0]], **kw) == ["m0", "m1", "x"]
    assert A.spread(M(2), [["a", "b"], ["c"]], **kw) == ["m0", "a", "b", "m1", "c"]    # whole groups


# ---- the counted-wait protocol on Emitter ---------------------------------------------------------------------------------
LOAD = "buffer_load_dword v%d, v0, s[4:7], 0 offen"


def test_counted_wait_protocol_toy_trip():
    g = A.Emitter(None)
    g.e("s_nop 0")
    g.trip_open()
    g.put([A.vm("A", LOAD % 1)])
    g.wait_vm(["B"], "cyclic")           # B of the previous trip; younger: C of the previous trip, A -> 2
    g.put(["s_nop 1", A.vm("B", LOAD % 2), A.vm("C", LOAD % 3)])
    g.wait_vm(["A", "B"])                # A: younger B, C -> 2; B: younger C -> 1; the minimum
    g.trip_close()
    assert g.out == ["\ts_nop 0", "\t" + LOAD % 1, "\ts_waitcnt vmcnt(2)\t; cyclic", "\ts_nop 1", "\t" + LOAD % 2, "\t" + LOAD % 3, "\ts_waitcnt vmcnt(1)"]
    assert g.trip is None
    g.put([A.vm("A", LOAD % 4)])         # outside a trip: the plain instruction
    assert g.out[-1] == "\t" + LOAD % 4
    assert A.vm("", LOAD % 5) == LOAD % 5 and A.vm(None, LOAD % 5) == LOAD % 5   # no tag: no entry (the copies outside a loop)


def test_counted_wait_protocol_conditional_and_uncounted_copies():
    g = A.Emitter(None)
    g.trip_open()
    g.put([A.vm("A", LOAD % 1), A.vm("R", LOAD % 2, True), A.vm("B", LOAD % 3)])
    g.put([A.vm("A", LOAD % 1), A.vm("B", LOAD % 3)], count=False)   # the second copy of the stretch: emitted, tagged, not counted again
    g.wait_vm(["A"])                   # younger: R (conditional: not counted), B -> 1
    g.trip_close()
    assert g.out[-1] == "\ts_waitcnt vmcnt(1)" and len(g.out) == 6


def test_counted_wait_protocol_refuses_an_untagged_buffer_instruction():
    g = A.Emitter(None)
    g.trip_open()
    g.put([A.vm("A", LOAD % 1)])
    g.e(LOAD % 2)
    g.wait_vm(["A"])
    with pytest.raises(AssertionError, match="untagged"):
        g.trip_close()


def test_counted_wait_protocol_needs_an_open_trip():
    g = A.Emitter(None)
    with pytest.raises(AssertionError):
        g.wait_vm(["A"])
    with pytest.raises(AssertionError):
        g.trip_close()
    g.trip_open()
    with pytest.raises(AssertionError):
        g.trip_open()


def test_counted_wait_protocol_range_of_the_counter():
    for clamp in (False, True):
        g = A.Emitter(None)
        g.trip_open()
        g.put([A.vm("A", LOAD % 1)] + [A.vm("B", LOAD % 2)] * 70)
        g.wait_vm(["A"])
        if clamp:
            g.trip_close(clamp=True)
            assert g.out[-1] == "\ts_waitcnt vmcnt(63)"
        else:
            with pytest.raises(AssertionError):
                g.trip_close()


# ---- snippet functions: (call, instructions, registers it may name) -------------------------------------------------------
def regs(p, first, n=1):
    return {(p, first + i) for i in range(n)}


def named(insts):
    out = set()
    for ins in insts:
        for p, a, b in re.findall(r"\b([vsa])\[(\d+):(\d+)\]", ins):
            out |= regs(p, int(a), int(b) - int(a) + 1)
        for p, a in re.findall(r"\b([vsa])(\d+)\b", ins):
            out.add((p, int(a)))
    return out


TV, XR, S1, S2 = list(range(10, 18)), list(range(20, 28)), list(range(30, 38)), list(range(40, 48))
V8 = regs("v", 10, 8)


def vs(*lists):
    return {("v", r) for lst in lists for r in lst}


SNIPPETS = {
    "mfma": (lambda: [A.mfma(8, 20, 30)], 1, regs("a", 8, 4) | regs("v", 20, 4) | regs("v", 30, 4)),
    "mfma zero": (lambda: [A.mfma(8, 20, 30, zero=True, afile="a")], 1, regs("a", 8, 4) | regs("a", 20, 4) | regs("v", 30, 4)),
    "mfma f8": (lambda: [A.mfma(8, 24, 32, f8=True)], 1, regs("a", 8, 4) | regs("v", 24, 8) | regs("v", 32, 8)),
    "acc_pair_read": (lambda: A.acc_pair_read(TV, 64, 72), 8, V8 | regs("a", 64, 4) | regs("a", 72, 4)),
    "pack4": (lambda: A.pack4(50, TV), 4, V8 | regs("v", 50, 4)),
    "unpack8": (lambda: A.unpack8(XR, 50), 8, regs("v", 20, 8) | regs("v", 50, 4)),
    "stats_acc": (lambda: A.stats_acc(S1, S2, XR), 16, vs(S1, S2, XR)),
    "bn_bwd_acc relu": (lambda: A.bn_bwd_acc(S1, S2, XR, 60, 5, [6] * 8, (7, 8)), 40, vs(S1, S2, XR, range(60, 64), [5, 6, 7, 8])),
    "bn_bwd_acc leaky": (lambda: A.bn_bwd_acc(S1, S2, XR, 60, 5, TV, (7, 8), leaky=TV[1:] + TV[:1]), 48,
                         vs(S1, S2, XR, range(60, 64), [5, 7, 8], TV)),
    "dpp_row_sum": (lambda: A.dpp_row_sum(S1 + S2), 64, vs(S1, S2)),
    "dz_xhat_finish": (lambda: A.dz_xhat_finish(S1, S2, range(60, 68), range(68, 76), TV), 24, vs(S1, S2, range(60, 76), TV)),
    "exec_lane15": (A.exec_lane15, 2, set()),
    "bn_relu_bits16": (lambda: A.bn_relu_bits16(50, 20, 60, 68, 9, 5, 6, 7), 36,
                       regs("v", 50, 4) | regs("v", 20, 8) | regs("v", 60, 16) | {("s", 9), ("v", 5), ("v", 6), ("v", 7)}),
    "desc_tail": (lambda: A.desc_tail(12, "4096"), 2, regs("s", 14, 2)),
    "desc_tail flags only": (lambda: A.desc_tail(12), 1, {("s", 15)}),
    "desc pointer": (lambda: A.desc(12, 20, 21, records="s30", minus="s31"), 4, regs("s", 12, 4) | regs("s", 20, 2) | regs("s", 30, 2)),
    "desc pointer + offset": (lambda: A.desc(12, 20, 21, "s8", "s9", "64"), 5, regs("s", 12, 4) | regs("s", 20, 2) | regs("s", 8, 2)),
    "desc 32-bit offset": (lambda: A.desc(12, 20, 21, "128"), 4, regs("s", 12, 4) | regs("s", 20, 2)),
    "desc_addr pointer": (lambda: A.desc_addr(12, 20, 23), 2, regs("s", 12, 2) | {("s", 20), ("s", 23)}),
    "desc_addr pointer + offset": (lambda: A.desc_addr(12, 20, 23, "s8", "s9", comment="window"), 3, regs("s", 12, 2) | {("s", 20), ("s", 23)} | regs("s", 8, 2)),
    "desc_adv": (lambda: A.desc_adv(12, 40), 3, regs("s", 12, 3) | {("s", 40)}),
}


@pytest.mark.parametrize("name", sorted(SNIPPETS))
def test_snippet_count_and_registers(name):
    call, count, allowed = SNIPPETS[name]
    insts = call()
    assert isinstance(insts, list) and all(isinstance(i, str) for i in insts)
    assert len(insts) == count
    assert named(insts) <= allowed, named(insts) - allowed
    if allowed:
        assert named(insts), "the check sees no register at all"


def test_snippet_texts_that_every_kernel_depends_on():
    assert A.mfma(8, 20, 30) == "v_mfma_f32_16x16x32_bf16 a[8:11], v[20:23], v[30:33], a[8:11]"
    assert A.mfma(8, 20, 30, zero=True, afile="a") == "v_mfma_f32_16x16x32_bf16 a[8:11], a[20:23], v[30:33], 0"
    assert A.mfma(8, 24, 32, f8=True) == "v_mfma_f32_16x16x128_f8f6f4 a[8:11], v[24:31], v[32:39], a[8:11]"
    assert A.exec_lane15() == ["s_mov_b32 exec_lo, 0x80008000", "s_mov_b32 exec_hi, 0x80008000"]
    assert A.desc(12, 20, 21, "s8", None, "64") == ["s_add_u32 s12, s20, s8", "s_addc_u32 s13, s21, 0", "s_and_b32 s13, s13, 0xffff", "s_mov_b32 s14, 64",
                                                    "s_mov_b32 s15, 0x00020000"]
    assert A.desc(12, 20, 21, records="s30", minus="s31")[:3] == ["s_mov_b32 s12, s20", "s_and_b32 s13, s21, 0xffff", "s_sub_u32 s14, s30, s31"]
    assert A.desc_addr(12, 20, 23, "s8", "s9", comment="window") == ["s_add_u32 s12, s20, s8\t; window", "s_addc_u32 s13, s23, s9", "s_and_b32 s13, s13, 0xffff"]
    assert A.desc(12, 20, 21, records="64") == A.desc_addr(12, 20, 21) + A.desc_tail(12, "64")
    assert A.dpp_row_sum([3])[0] == "v_add_f32_dpp v3, v3, v3 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
    leaky = A.bn_bwd_acc(S1, S2, XR, 60, 5, TV, (7, 8), leaky=TV[1:] + TV[:1])
    assert leaky[:3] == ["v_bfe_i32 v10, v5, 0, 1\t; 0 / -1: ReLU mask bit of element 0", "v_mul_f32 v11, 0x%08x, v20" % A.LEAKY_BITS, "v_bfi_b32 v20, v10, v20, v11\t; dz"]
