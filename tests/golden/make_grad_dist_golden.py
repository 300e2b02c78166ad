#!/usr/bin/env python3
"""Records tests/golden/grad_dist_ref.npz by running the REFERENCE's own GradDistributionTB callback (sota_imagenet/callbacks.py of a reference
checkout, loaded by path through make_sam_golden.load_reference with its stub modules; none of its text is here) on the CPU, with a tb_logger
that captures what add_histogram is handed.

    python tests/golden/make_grad_dist_golden.py --reference <checkout of the reference>

Inputs (float32, drawn from numpy generators seeded below): per tag a list of tensors — () and (1,), one of 7 elements (shorter than subsample 10),
an all-equal one, one that is mostly exact zeros, several with |x| = 10^u, u uniform over [-20, 3], signs mixed, and one large tensor ((300, 257)
among the parameters only, to keep the file under 1 MB; (41, 13, 3, 3) in the states, more than one 4096-element work item).  exp_avg_sq is
non-negative.  The callback reads optimizer.state.values() and model.parameters(): a namespace with a dict of dicts and a ParameterList do.

The reference takes log10 in float32 and the tests bin the recorded values against log10 of the bin edges, so a value next to an edge could fall on
either side: every input whose |x| lies within a relative 1e-3 of an edge of the bins (tests/grad_dist_common.py) is moved to the centre of its
bin, and every recorded value is asserted to be at least 1e-5 away from every log10 edge.

Arrays of the file: meta (json: shapes per tag, global_sample_step), in/<tag>/<i> the inputs (flat), out/<subsample>/<tag> the recorded float32
array for subsample in {1, 3, 10}."""
import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import grad_dist_common as G  # noqa: E402

STEP = 19200
STATE_SHAPES = [(), (1,), (7,), (64,), (50, 20), (33, 17), (41, 13, 3, 3), (129,)]
PARAM_SHAPES = [(1,), (), (7,), (64,), (50, 20), (33, 17), (300, 257), (129,)]


def _tensor(rng, shape, kind, nonneg):
    n = int(np.prod(shape)) if len(shape) else 1
    if kind == "equal":
        x = np.full(n, 3.7e-4, dtype=np.float32)
    else:
        x = (10.0 ** rng.uniform(-20.0, 3.0, n)).astype(np.float32)
        if not nonneg:
            x *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
        if kind == "zeros":
            x[rng.uniform(size=n) < 0.7] = 0.0
        else:
            x[rng.uniform(size=n) < 0.02] = 0.0
    return x.reshape(shape)


def off_the_edges(x):
    """every element within a relative 1e-3 of a bin edge moves to the centre of its bin (bin 0: half its upper edge), sign kept"""
    e = G.edges().astype(np.float64)
    a = np.abs(x.astype(np.float64)).ravel()
    near = (np.abs(a[:, None] - e[None, :]) <= 1e-3 * e[None, :]).any(axis=1) if a.size * e.size < 5e7 else None
    if near is None:  # the large tensor: by nearest edge
        i = np.clip(np.searchsorted(e, a), 1, len(e) - 1)
        near = np.minimum(np.abs(a - e[i - 1]) / e[i - 1], np.abs(a - e[i]) / e[i]) <= 1e-3
    b = G.bin_of(x)
    lo = np.concatenate([[0.0], e])[b]
    hi = np.concatenate([e, [2 * e[-1]]])[b]
    centre = (0.5 * (lo + hi)).astype(np.float32)
    flat = x.ravel().copy()
    sign = np.where(np.signbit(flat), np.float32(-1), np.float32(1))
    flat[near] = (sign * centre)[near]
    assert (G.bin_of(flat) == b).all()
    return flat.reshape(x.shape)


def inputs():
    rng = np.random.default_rng(4601)
    kinds = ["plain", "plain", "plain", "plain", "equal", "zeros", "plain", "plain"]
    out = {}
    for tag, shapes, nonneg in ((G.TAGS[0], STATE_SHAPES, False), (G.TAGS[1], STATE_SHAPES, True), (G.TAGS[2], PARAM_SHAPES, False)):
        out[tag] = [off_the_edges(_tensor(rng, s, k, nonneg)) for s, k in zip(shapes, kinds)]
    return out


class Capture:
    def __init__(self):
        self.seen = {}

    def add_histogram(self, tag, values, global_step=None, **kw):
        assert tag not in self.seen
        self.seen[tag] = (values.detach().clone().numpy(), global_step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "grad_dist_ref.npz"))
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("make_sam_golden", os.path.join(HERE, "make_sam_golden.py"))
    sam = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sam)
    clb_mod, _ = sam.load_reference(a.reference)
    torch.set_num_threads(1)
    ins = inputs()
    arrays = {"meta": np.frombuffer(json.dumps(dict(shapes={t: [list(x.shape) for x in xs] for t, xs in ins.items()},
                                                    global_sample_step=STEP)).encode(), dtype=np.uint8)}
    for tag, xs in ins.items():
        for i, x in enumerate(xs):
            arrays[f"in/{tag}/{i}"] = x.ravel()
    model = torch.nn.Module()
    model.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(x.copy())) for x in ins[G.TAGS[2]]])
    states = {i: {"exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
              for i, (m, v) in enumerate(zip(ins[G.TAGS[0]], ins[G.TAGS[1]]))}
    log_edges = np.log10(G.edges().astype(np.float64))
    for s in G.SUBSAMPLES:
        clb = clb_mod.GradDistributionTB(log_every=50, subsample=s)
        cap = Capture()
        clb.state = types.SimpleNamespace(step=100, optimizer=types.SimpleNamespace(state=states), model=model, tb_logger=cap,
                                          global_sample_step=STEP)
        with torch.no_grad():
            clb.on_batch_end()
        assert sorted(cap.seen) == sorted(G.TAGS)
        for tag, (v, step) in cap.seen.items():
            assert step == STEP and v.dtype == np.float32 and len(v) == G.kept_total([x.size for x in ins[tag]], s)
            gap = np.abs(v.astype(np.float64)[:, None] - log_edges[None, :]).min() if len(v) * len(log_edges) < 5e7 else min(
                np.abs(c.astype(np.float64)[:, None] - log_edges[None, :]).min() for c in np.array_split(v, 64))
            assert gap >= 1e-5, (tag, s, gap)
            assert (np.bincount(G.bin_of_log(v), minlength=G.NB) == G.formula_of(ins[tag], s)).all(), (tag, s)
            arrays[f"out/{s}/{tag}"] = v
    np.savez_compressed(a.out, **arrays)
    size = os.path.getsize(a.out)
    assert size < 1_000_000, size
    print(f"wrote {a.out}: {size} bytes")


if __name__ == "__main__":
    main()
