#!/usr/bin/env python3
"""asm_common.py — what the gfx950 assembly generators of this directory share.
  What no kernel decides: register allocation (Alloc, R), the instruction emitter (Emitter), the code-object wrapper (header, kernel descriptor,
  metadata: code_object) and the command line (generate, main).
  The scheduling vocabulary, which several kernels decide identically:
    placement      merge (one group list spread evenly through another) and spread (groups placed between MFMAs, the four placement rules as arguments);
    counted waits  resolve_waits and its one protocol on Emitter: trip_open, vm()-tagged operations emitted with put, wait_vm(tags), trip_close;
    snippets       plain functions from register numbers to a flat list of instructions, one per shared sequence: mfma, acc_pair_read, pack4, unpack8,
                   stats_acc, bn_bwd_acc, dpp_row_sum, dz_xhat_finish, exec_lane15, bn_relu_bits16, desc (= desc_addr + desc_tail), desc_adv.
  Loop orders, grouping (dconv_gen chops in twos, pw_gen keeps tagged stores in its groups, po_gen emits straight through) and what goes between which
  MFMAs stay in the generators: they are the schedule.  A helper exists only where at least two sites emit the same sequence."""
import argparse
import os
import struct

LEAKY_BITS = 0x3c23d70a   # 0.01f: the slope of the stats == 3 epilogues


class Alloc:
    def __init__(self, prefix, first, limit):
        self.p, self.n, self.limit = prefix, first, limit

    def get(self, n=1, align=1):
        self.n = (self.n + align - 1) // align * align
        r = self.n
        self.n += n
        assert self.n <= self.limit, "out of %s registers" % self.p
        return r


def R(p, i, n=1):
    return "%s%d" % (p, i) if n == 1 else "%s[%d:%d]" % (p, i, i + n - 1)


def merge(a, b):
    """the group list b spread evenly through the group list a (a new list)"""
    out = []
    na, nb = len(a), len(b)
    ib = 0
    for i, g in enumerate(a):
        out.append(g)
        while ib < nb and (ib + 1) * na <= (i + 1) * nb:
            out.append(b[ib])
            ib += 1
    out.extend(b[ib:])
    return out


def resolve_waits(events):
    """events of ONE loop trip in program order: ("op", tag, conditional) for a vector-memory instruction, ("wait", key, [tags]) for a
    counted wait.  Returns {key: count}: the unconditional operations issued after the youngest one carrying one of the wait's tags,
    searching back cyclically through the trip (steady state; the first trip only has MORE younger operations in flight, from the
    prologue, and a conditional operation only makes the real count larger: both make a counted wait stronger, never weaker)."""
    n = len(events)
    counts = {}
    for i, (kind, key, tags) in enumerate(events):
        if kind != "wait":
            continue
        assert tags, "a counted wait must name the operations it waits for"
        best = None
        for tag in tags:
            cnt = 0
            for back in range(1, n + 1):
                k2, t2, cond = events[(i - back) % n]
                if k2 != "op":
                    continue
                if t2 == tag:
                    break
                cnt += 0 if cond else 1
            else:
                raise AssertionError("no operation tagged %r in the trip" % (tag,))
            best = cnt if best is None else min(best, cnt)
        counts[key] = best
    return counts


def spread(mf, groups, first=1, tail=1, percent=100, clamp=False, skip=()):
    """the MFMA list `mf` with the instruction groups `groups` placed between its members (a new flat list): group j of k goes behind
    MFMA first + (j * span) // k.  The four rules in use, each as its kernel decided it:
      dconv_gen / pk_gen   span = n - first - 1                            (the defaults; fp8 columns with first = 0)
      po_gen               span = max(1, n - first - 1), position <= n - 1 (clamp)
      wg_gen / wg1_gen     span = int((n - first) * rspan / 100)           (tail = 0, percent = Cfg.rspan)
      pw_gen               position (j * n) // k                           (first = 0, tail = 0), and the groups of `skip` (by identity) are
                           left out WITHOUT moving the others: the two copies of a substep issue their common instructions in the same order
    More groups than MFMAs share positions (every position stays below first + span).  A group whose position is no MFMA's index (n <= first
    without clamp) is dropped, as the generators always did; k = 0 returns the MFMAs alone."""
    n, k = len(mf), len(groups)
    span = n - first - tail
    if percent != 100:
        span = int(span * percent / 100)
    if clamp:
        span = max(1, span)
    slots = {}
    for j, grp in enumerate(groups):
        pos = first + (j * span) // k
        slots.setdefault(min(n - 1, pos) if clamp else pos, []).append(grp)
    skipped = {id(g) for g in skip}
    out = []
    for i, m in enumerate(mf):
        out.append(m)
        for grp in slots.get(i, ()):
            if id(grp) not in skipped:
                out.extend(grp)
    return out


# ---- instruction sequences several kernels emit identically: plain functions of register numbers, each returns a flat list of instructions
# (an instruction may carry its comment behind "\t; ").  Grouping and placement stay with the caller.
def mfma(acc, a, b, zero=False, f8=False, afile="v"):
    """ONE instruction: a[acc:acc+3] = <afile>[a..] x v[b..] + (0 if zero else a[acc:acc+3]); v_mfma_f32_16x16x32_bf16 on 4-register operands,
    f8: v_mfma_f32_16x16x128_f8f6f4 on 8-register operands"""
    w = 8 if f8 else 4
    return "%s %s, %s, %s, %s" % ("v_mfma_f32_16x16x128_f8f6f4" if f8 else "v_mfma_f32_16x16x32_bf16", R("a", acc, 4), R(afile, a, w), R("v", b, w),
                                  "0" if zero else R("a", acc, 4))


def acc_pair_read(tv, a0, a1):
    """8 instructions: tv[0:4] / tv[4:8] = accumulator tiles a0 / a1, interleaved"""
    return [ins for i in range(4) for ins in ("v_accvgpr_read_b32 %s, a%d" % (R("v", tv[i]), a0 + i), "v_accvgpr_read_b32 %s, a%d" % (R("v", tv[4 + i]), a1 + i))]


def pack4(d, tv):
    """4 instructions: v[d:d+3] = the 8 floats tv as bf16 pairs"""
    return ["v_cvt_pk_bf16_f32 %s, %s, %s" % (R("v", d + i), R("v", tv[2 * i]), R("v", tv[2 * i + 1])) for i in range(4)]


def unpack8(xr, d):
    """8 instructions: xr[0:8] = the 8 bf16 values of v[d:d+3] as floats"""
    return [ins for i in range(4) for ins in ("v_lshlrev_b32 %s, 16, %s" % (R("v", xr[2 * i]), R("v", d + i)), "v_and_b32 %s, 0xffff0000, %s" % (R("v", xr[2 * i + 1]), R("v", d + i)))]


def stats_acc(s1, s2, xr):
    """16 instructions: BN statistics, s1 += x, s2 += x * x"""
    return [ins for i in range(8) for ins in ("v_add_f32 %s, %s, %s" % (R("v", s1[i]), R("v", s1[i]), R("v", xr[i])),
                                              "v_fma_f32 %s, %s, %s, %s" % (R("v", s2[i]), R("v", xr[i]), R("v", xr[i]), R("v", s2[i])))]


def bn_bwd_acc(s1, s2, xr, y, bits, mask, yv, leaky=None, what="ReLU mask bit"):
    """40 instructions (48 with `leaky`): the BN-backward sums of 8 elements under a ReLU mask, s1 += dz, s2 += dz * y with dz = xr where bit i of
    v[bits] is set, else 0 — or, leaky (8 temporaries), xr * 0.01: the fp32 product of the rounded value, as bn_reduce_kernel<MASK = 3>.  xr becomes
    dz; v[y:y+3] holds y as bf16 pairs; mask[i] takes the 0 / -1 of element i, yv[0:2] the unpacked y."""
    out = []
    for i in range(8):
        out.append("v_bfe_i32 %s, %s, %d, 1\t; 0 / -1: %s of element %d" % (R("v", mask[i]), R("v", bits), i, what, i))
        if leaky:
            out.append("v_mul_f32 %s, 0x%08x, %s" % (R("v", leaky[i]), LEAKY_BITS, R("v", xr[i])))
            out.append("v_bfi_b32 %s, %s, %s, %s\t; dz" % (R("v", xr[i]), R("v", mask[i]), R("v", xr[i]), R("v", leaky[i])))
        else:
            out.append("v_and_b32 %s, %s, %s\t; dz" % (R("v", xr[i]), R("v", xr[i]), R("v", mask[i])))
        if i & 1:
            out.append("v_and_b32 %s, 0xffff0000, %s" % (R("v", yv[1]), R("v", y + i // 2)))
        else:
            out.append("v_lshlrev_b32 %s, 16, %s" % (R("v", yv[0]), R("v", y + i // 2)))
        out.append("v_add_f32 %s, %s, %s" % (R("v", s1[i]), R("v", s1[i]), R("v", xr[i])))
        out.append("v_fma_f32 %s, %s, %s, %s\t; sum dz*y" % (R("v", s2[i]), R("v", xr[i]), R("v", yv[i & 1]), R("v", s2[i])))
    return out


def dpp_row_sum(regs):
    """4 * len(regs) instructions: lane 15 of every row of 16 lanes ends with the row's sum of each register"""
    return ["v_add_f32_dpp %s, %s, %s row_shr:%d row_mask:0xf bank_mask:0xf bound_ctrl:1" % (R("v", r), R("v", r), R("v", r), sh) for sh in (1, 2, 4, 8) for r in regs]


def dz_xhat_finish(s1, s2, mu, isd, t):
    """24 instructions: s2 = sum dz*xhat = invstd * (sum dz*y - mean * sum dz) of 8 channels (t: 8 temporaries)"""
    return (["v_mul_f32 %s, %s, %s" % (R("v", t[i]), R("v", mu[i]), R("v", s1[i])) for i in range(8)]
            + ["v_sub_f32 %s, %s, %s" % (R("v", s2[i]), R("v", s2[i]), R("v", t[i])) for i in range(8)]
            + ["v_mul_f32 %s, %s, %s" % (R("v", s2[i]), R("v", isd[i]), R("v", s2[i])) for i in range(8)])


def exec_lane15():
    """2 instructions: EXEC = lane 15 of every row of 16, where a DPP row sum ends"""
    return ["s_mov_b32 exec_lo, 0x80008000", "s_mov_b32 exec_hi, 0x80008000"]


def bn_relu_bits16(d, f, sc, sh, k1, bits, o, o2):
    """36 instructions: v[f:f+3] = a = relu(y * scale + shift) as bf16 of the 8 raw bf16 values y in v[d:d+3] (scale / shift: v[sc:sc+7] / v[sh:sh+7]);
    v[bits] = the byte of ReLU bits (a != 0, bit 2j + half of pair j); v[o2] = v[o] >> 4 (the byte offset of the bits from that of a).  Rounded to bf16
    first, ReLU on the packed pairs as signed 16-bit integers (a negative bf16, -0 included, is a negative int16): the same values as ReLU in fp32
    followed by the rounding.  The bit is that of the STORED value (bn_apply_kernel tests the fp32 value: the same unless a positive value rounds to a
    bf16 zero, below 2^-134).  s[k1] = 0x00010001; v[f+4:f+7] are temporaries."""
    t = f + 4
    return (unpack8(range(f, f + 8), d)
            + ["v_fma_f32 %s, %s, %s, %s" % (R("v", f + q), R("v", f + q), R("v", sc + q), R("v", sh + q)) for q in range(8)]
            + pack4(f, range(f, f + 8))
            + ["v_pk_max_i16 %s, %s, 0" % (R("v", f + q), R("v", f + q)) for q in range(4)]
            + ["v_pk_min_u16 %s, %s, %s" % (R("v", t + q), R("v", f + q), R("s", k1)) for q in range(4)]
            + ["v_lshl_or_b32 %s, %s, 2, %s" % (R("v", t), R("v", t + 1), R("v", t)), "v_lshl_or_b32 %s, %s, 2, %s" % (R("v", t + 2), R("v", t + 3), R("v", t + 2)),
               "v_lshl_or_b32 %s, %s, 4, %s" % (R("v", t), R("v", t + 2), R("v", t)), "v_lshrrev_b32 %s, 4, %s" % (R("v", o2), R("v", o)),
               "v_lshrrev_b32 %s, 15, %s" % (R("v", t + 1), R("v", t)), "v_and_b32 %s, 0x55, %s" % (R("v", t), R("v", t)),
               "v_and_b32 %s, 0xaa, %s" % (R("v", t + 1), R("v", t + 1)), "v_or_b32 %s, %s, %s" % (R("v", bits), R("v", t + 1), R("v", t))])


def desc_tail(srd, records=None, minus=None):
    """the tail of the raw-buffer descriptor s[srd:srd+3]: num_records = `records` (an operand; - `minus` when given; None: set by the caller), then the
    flags word.  1 or 2 instructions."""
    out = []
    if records is not None:
        out.append("s_sub_u32 %s, %s, %s" % (R("s", srd + 2), records, minus) if minus is not None else "s_mov_b32 %s, %s" % (R("s", srd + 2), records))
    return out + ["s_mov_b32 %s, 0x00020000" % R("s", srd + 3)]


def desc_addr(srd, lo, hi, off_lo=None, off_hi=None, comment=None):
    """the address words of the raw-buffer descriptor s[srd:srd+3]: the pointer s[lo], s[hi] (2 instructions), or pointer + offset (3: off_lo an
    operand, off_hi an operand or None for a 32-bit offset), the upper 16 bits of the second word cleared.  comment: on the first instruction."""
    if off_lo is None:
        out = ["s_mov_b32 %s, %s" % (R("s", srd), R("s", lo)), "s_and_b32 %s, %s, 0xffff" % (R("s", srd + 1), R("s", hi))]
    else:
        out = ["s_add_u32 %s, %s, %s" % (R("s", srd), R("s", lo), off_lo), "s_addc_u32 %s, %s, %s" % (R("s", srd + 1), R("s", hi), off_hi if off_hi is not None else "0"),
               "s_and_b32 %s, %s, 0xffff" % (R("s", srd + 1), R("s", srd + 1))]
    if comment:
        out[0] += "\t; " + comment
    return out


def desc(srd, lo, hi, off_lo=None, off_hi=None, records=None, minus=None, comment=None):
    """a whole raw-buffer descriptor: desc_addr() + desc_tail().  A site that puts a line of its own between the two calls them itself."""
    return desc_addr(srd, lo, hi, off_lo, off_hi, comment) + desc_tail(srd, records, minus)


def desc_adv(srd, inc):
    """3 instructions: the window of s[srd:srd+3] moves on by s[inc] bytes, num_records shrinks by as much"""
    return ["s_add_u32 %s, %s, %s" % (R("s", srd), R("s", srd), R("s", inc)),
            "s_addc_u32 %s, %s, 0" % (R("s", srd + 1), R("s", srd + 1)),
            "s_sub_u32 %s, %s, %s" % (R("s", srd + 2), R("s", srd + 2), R("s", inc))]


def vm(tag, text, cond=False):
    """a vector-memory instruction tagged for the counted waits of its loop trip (Emitter.put); cond: issued on one path only.  No tag (the
    copies outside a loop): the plain instruction."""
    return ("vm", tag, text, cond) if tag else text


def code_object(name, body, lds, kernarg, ptrs, args, agprs, accum_offset, sgprs, wg_id_y):
    """the complete .s text of one kernel: `body` (lines) behind the symbol, the kernel descriptor and the code-object metadata.
    Kernel arguments: `ptrs` global pointers of 8 bytes, then by-value arguments of the sizes in `args`."""
    total_v = accum_offset + agprs
    assert lds <= 160 * 1024 and total_v <= 512 and 8 * ptrs + sum(args) == kernarg
    hdr = ['\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"', "\t.amdhsa_code_object_version 6", "\t.text", "\t.protected\t%s" % name,
           "\t.globl\t%s" % name, "\t.p2align\t8", "\t.type\t%s,@function" % name, "%s:" % name]
    tail = ["\t.section\t.rodata,\"a\",@progbits", "\t.p2align\t6, 0x0", "\t.amdhsa_kernel %s" % name]
    kd = dict(group_segment_fixed_size=lds, private_segment_fixed_size=0, kernarg_size=kernarg,
              user_sgpr_count=2, user_sgpr_dispatch_ptr=0, user_sgpr_queue_ptr=0, user_sgpr_kernarg_segment_ptr=1,
              user_sgpr_dispatch_id=0, user_sgpr_kernarg_preload_length=0, user_sgpr_kernarg_preload_offset=0,
              user_sgpr_private_segment_size=0, uses_dynamic_stack=0, enable_private_segment=0,
              system_sgpr_workgroup_id_x=1, system_sgpr_workgroup_id_y=wg_id_y, system_sgpr_workgroup_id_z=0,
              system_sgpr_workgroup_info=0, system_vgpr_workitem_id=0, next_free_vgpr=total_v,
              next_free_sgpr=sgprs, accum_offset=accum_offset, reserve_vcc=1, float_round_mode_32=0,
              float_round_mode_16_64=0, float_denorm_mode_32=3, float_denorm_mode_16_64=3, dx10_clamp=1, ieee_mode=1,
              fp16_overflow=0, tg_split=0)
    for k, v in kd.items():
        tail.append("\t\t.amdhsa_%s %d" % (k, v))
    tail += ["\t.end_amdhsa_kernel", "\t.text", "\t.amdgpu_metadata", "---", "amdhsa.kernels:", "  - .agpr_count:     %d" % agprs, "    .args:"]
    for i in range(ptrs):
        tail.append("      - .address_space:  global\n        .offset:         %d\n        .size:           8\n        .value_kind:     global_buffer" % (8 * i))
    off = 8 * ptrs
    for size in args:
        tail.append("      - .offset:         %d\n        .size:           %d\n        .value_kind:     by_value" % (off, size))
        off += size
    tail += ["    .group_segment_fixed_size: %d" % lds, "    .kernarg_segment_align: 8", "    .kernarg_segment_size: %d" % kernarg,
             "    .max_flat_workgroup_size: 256", "    .name:           %s" % name, "    .private_segment_fixed_size: 0",
             "    .sgpr_count:     %d" % (sgprs + 6), "    .sgpr_spill_count: 0", "    .symbol:         %s.kd" % name,
             "    .uniform_work_group_size: 1", "    .uses_dynamic_stack: false", "    .vgpr_count:     %d" % total_v,
             "    .vgpr_spill_count: 0", "    .wavefront_size: 64", "amdhsa.target:   amdgcn-amd-amdhsa--gfx950",
             "amdhsa.version:\n  - 1\n  - 2", "...", "\t.end_amdgpu_metadata"]
    body = body + ["\t.p2align 8", ".Lend_%s:" % name, "\t.size\t%s, .Lend_%s-%s" % (name, name, name)]
    return "\n".join(hdr + body + tail) + "\n"


class Emitter:
    """the instruction text of one kernel (self.out) and its register allocators; a generator's gen() allocates, emits and ends with
    finish().  label_prefix: po_gen.py puts the kernel name into its labels."""

    def __init__(self, c, sgpr_limit=100, label_prefix="L_"):
        self.c = c
        self.out = []
        self.nlabel = 0
        self.label_prefix = label_prefix
        self.S = Alloc("s", 4, sgpr_limit)
        self.V = Alloc("v", 1, 256)
        self.trip, self.trip_start, self.trip_tagged = None, 0, set()   # the events of the open loop trip (resolve_waits), its first line, its tagged lines

    def e(self, s, comment=None):
        self.out.append("\t" + s + ("\t; " + comment if comment else ""))

    def label(self, name):
        self.out.append(name + ":")

    def newlabel(self, stem):
        self.nlabel += 1
        return "%s%s_%d" % (self.label_prefix, stem, self.nlabel)

    def comment(self, s):
        self.out.append("\t; " + s)

    # ---- counted waits of one loop trip: trip_open(); vm()-tagged operations (put) and wait_vm(tags) in program order; trip_close() writes the counts
    def put(self, insts, count=True):
        """emit a flat list of instructions; a vm() entry of an open trip is recorded as one of its operations (count=False: emitted and tagged, not
        counted: the second copy of a stretch whose first copy was counted)"""
        for ins in insts:
            if isinstance(ins, tuple):
                _, tag, ins, cond = ins
                if self.trip is not None:
                    self.trip_tagged.add(len(self.out))
                    if count:
                        self.trip.append(("op", tag, cond))
            self.e(ins)

    def trip_open(self):
        assert self.trip is None, "a trip is open already"
        self.trip, self.trip_start, self.trip_tagged = [], len(self.out), set()

    def wait_vm(self, tags, comment=None):
        """s_waitcnt vmcnt(n), n = the most that leaves every operation of the trip tagged with one of `tags` complete"""
        assert self.trip is not None, "a counted wait stands inside a trip"
        self.trip.append(("wait", len(self.out), list(tags)))
        self.e("s_waitcnt vmcnt(?)", comment)

    def trip_close(self, clamp=False):
        """every buffer_ instruction of the trip must have been tagged; clamp: a count above the counter's range waits for 63"""
        assert self.trip is not None, "no trip is open"
        for i in range(self.trip_start, len(self.out)):
            assert i in self.trip_tagged or not self.out[i].startswith("\tbuffer_"), "untagged vector-memory operation in the loop trip: " + self.out[i]
        for i, cnt in resolve_waits(self.trip).items():
            assert 0 <= cnt and (clamp or cnt <= 63)
            self.out[i] = self.out[i].replace("vmcnt(?)", "vmcnt(%d)" % min(cnt, 63))
        self.trip = None

    def finish(self, lds, kernarg, ptrs, args, wg_id_y=0):
        """the code object around self.out (self.accum_offset, self.nagpr and the SGPR allocator are final by now)"""
        self.lds_bytes = lds
        return code_object(self.c.name, self.out, lds, kernarg, ptrs, args, self.nagpr, self.accum_offset, self.S.n, wg_id_y)


def generate(variants, Gen, base, /, **over):
    """(config, generator, .s text) of variant `base`, its config fields replaced by `over` (over["name"] renames the kernel)"""
    c = variants[base]
    if over:
        c = type(c)(**{**c.__dict__, **over})
    g = Gen(c)
    return c, g, g.gen()


def main(variants, generate, table=None):
    """python <gen>.py [--out DIR] [--set key=int ...] [--suffix SFX] [names ...]: writes <name>.s for the named (default: every shipped)
    variant.  --set overrides config fields (tuning); --suffix renames the kernels and, for a generator with a `table` hook (config ->
    words), also writes <name>.tbl, the raw per-wave table tools/micro/dconv_bench.cpp passes as kernel arguments."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="build")
    ap.add_argument("--set", action="append", default=[], help="tuning: override a config field (key=int), with --suffix names the kernel")
    ap.add_argument("--suffix", default="")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    over = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in a.set}
    for name in (a.names or variants):
        if a.suffix:
            over["name"] = name + a.suffix
        c, g, text = generate(name, **over)
        if a.suffix and table:
            words = table(c)
            with open(os.path.join(a.out, c.name + ".tbl"), "wb") as f:
                f.write(struct.pack("<%dI" % len(words), *words))
        with open(os.path.join(a.out, c.name + ".s"), "w") as f:
            f.write(text)
        print("%s: %d lines, %d VGPR + %d AGPR, %d SGPR, LDS %d" % (c.name, text.count("\n"), g.accum_offset, g.nagpr, g.S.n, g.lds_bytes))
