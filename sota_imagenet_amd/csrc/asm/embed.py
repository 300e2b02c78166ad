#!/usr/bin/env python3
"""embed.py — the files gen_kernels.cpp embeds.
  embed.py kernels <out dir>           every shipped kernel of the six generators as <name>.s (each variant generated once) and one
                                       initialiser per kernel: dconv_meta.inc (direct 3x3 kernels), dconv_tt.inc (their transform tables,
                                       Cfg.bnin), pw_meta.inc (pointwise), wg_meta.inc / wg1_meta.inc (3x3 / 1x1 weight gradient),
                                       pk_meta.inc (long-reduction pointwise), po_meta.inc (output-heavy pointwise with resident weights)
  embed.py blob <linked .hsaco> <out>  the linked code object as a byte array (dconv_blob.inc)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dconv_gen  # noqa: E402
import pk_gen  # noqa: E402
import po_gen  # noqa: E402
import pw_gen  # noqa: E402
import wg1_gen  # noqa: E402
import wg_gen  # noqa: E402

INCLUDES = ("dconv_meta.inc", "dconv_tt.inc", "pw_meta.inc", "wg_meta.inc", "wg1_meta.inc", "pk_meta.inc", "po_meta.inc")


def initialisers(mod, c, g):
    """(include file, initialiser) of one generated kernel: the fields of its variant struct in gen_kernels.cpp"""
    ka = mod.Gen.KA["size"]
    if mod is dconv_gen:
        words = ",".join("%du" % w for par in dconv_gen.tables(c) for row in par for w in row)
        yield "dconv_meta.inc", '{"%s", %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, {%s}},' % (
            c.name, c.H, c.W, c.IPT, c.TPI, c.BN, c.Cin, c.NCOLS, c.stats, c.s2d, c.bnin, c.fp8, g.lds_bytes, g.ka_size, words)
        if c.bnin:   # the transform tables of the kernels with the input's BatchNorm in their operand path
            words = ",".join("%du" % w for par in dconv_gen.ttables(c) for row in par for w in row)
            yield "dconv_tt.inc", '{"%s", {%s}},' % (c.name, words)
    elif mod is pw_gen:
        words = ",".join("%du" % w for row in pw_gen.tables(c) for w in row)
        yield "pw_meta.inc", '{"%s", %d, %d, %d, %d, %d, %d, {%s}},' % (c.name, c.K, c.N, c.stats, c.ROWS, g.lds_bytes, ka, words)
    elif mod is wg_gen:
        tn, ti = c.TPI_NUM
        yield "wg_meta.inc", '{"%s", %d, %d, %d, %d, %d, %d, %d, %d},' % (c.name, c.H, c.W, c.C, c.CO, tn, ti, g.lds_bytes, ka)
    elif mod is wg1_gen:
        yield "wg1_meta.inc", '{"%s", %d, %d, %d, %d, %d, %d},' % (c.name, c.C, c.CO, c.XP, c.DP, g.lds_bytes, ka)
    elif mod is pk_gen:
        yield "pk_meta.inc", '{"%s", %d, %d, %d, %d, %d, %d, %d},' % (c.name, c.W, c.Cin, c.NCOLS, c.BN, c.stats, g.lds_bytes, ka)
    else:
        yield "po_meta.inc", '{"%s", %d, %d, %d, %d, %d, %d, %d, %d, %d},' % (
            c.name, c.K, c.BN, c.stats, c.add, c.TP, c.WM, c.bnin, g.lds_bytes, ka)


def kernels(out_dir):
    rows = {inc: [] for inc in INCLUDES}
    for mod in (dconv_gen, pw_gen, wg_gen, wg1_gen, pk_gen, po_gen):
        for name in mod.VARIANTS:
            c, g, text = mod.generate(name)
            with open(os.path.join(out_dir, name + ".s"), "w") as f:
                f.write(text)
            for inc, row in initialisers(mod, c, g):
                rows[inc].append(row + "\n")
    for inc, lines in rows.items():
        with open(os.path.join(out_dir, inc), "w") as f:
            f.write("".join(lines))


def blob(hsaco, out):
    data = open(hsaco, "rb").read()
    with open(out, "w") as f:
        for i in range(0, len(data), 32):
            f.write(",".join(str(b) for b in data[i:i + 32]) + ",\n")


if __name__ == "__main__":
    {"kernels": kernels, "blob": blob}[sys.argv[1]](*sys.argv[2:])
