#!/usr/bin/env python3
"""asm_common.py — what the gfx950 assembly generators of this directory share and no kernel decides: register allocation, the
instruction emitter, the even merge of two instruction-group lists, the counted-wait resolver, the code-object wrapper (header,
kernel descriptor, metadata) and the command line."""
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

    def e(self, s, comment=None):
        self.out.append("\t" + s + ("\t; " + comment if comment else ""))

    def label(self, name):
        self.out.append(name + ":")

    def newlabel(self, stem):
        self.nlabel += 1
        return "%s%s_%d" % (self.label_prefix, stem, self.nlabel)

    def comment(self, s):
        self.out.append("\t; " + s)

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
