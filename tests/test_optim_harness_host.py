"""tests/optim_harness.py held to its own statements on the CPU: the yardstick rule at its edge and on the values that must never pass, the two
definitions of the reported ratio, the 64-element layout of the flat test buffers, and the model-scale helpers on a stub of a flat model."""
import math

import pytest
import torch

import optim_harness as H
from optim_harness import NAN


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------
def _with_error(err):
    """(got, ref) with max |ref| = 1 and max |got - ref| = err exactly"""
    return torch.tensor([1.0, err], dtype=torch.float64), torch.tensor([1.0, 0.0], dtype=torch.float64)


def test_the_rule_passes_at_its_bound_and_fails_above_it_and_on_nan_and_inf():
    yard = 1e-6
    edge = 1.5 * yard + 4 * 2.0 ** -24  # in figures: the constants are held too
    assert H.bound(yard, 1.0) == edge
    H.within_yardstick(*_with_error(edge), yard, "at the bound")
    for err in (math.nextafter(edge, math.inf), NAN, math.inf):
        with pytest.raises(AssertionError):
            H.within_yardstick(*_with_error(err), yard, f"error {err!r}")


def test_both_ratios_are_what_their_formulas_say():
    """err = 2^-21 against a reference of magnitude 2, so the floor is 4 * 2^-24 * 2 = 2^-21 as well"""
    got, ref = torch.tensor([2.0 + 2.0 ** -21, 0.5]), torch.tensor([2.0, 0.5], dtype=torch.float64)
    assert H.within_yardstick(got, ref, 2.0 ** -20, "yard above the floor") == 0.5
    assert H.within_yardstick(got, ref, 2.0 ** -20, "yard above the floor", floor_in_ratio=True) == 0.5
    assert H.within_yardstick(got, ref, 2.0 ** -23, "yard below the floor") == 4.0  # err / yard
    assert H.within_yardstick(got, ref, 2.0 ** -23, "yard below the floor", floor_in_ratio=True) == 1.0  # err / max(yard, floor)
    assert H.within_yardstick(got, ref, 0.0, "no yardstick", floor_in_ratio=True) == 1.0


# ---- the layout ----------------------------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65]


def _flat(**kw):
    vals = [torch.full((s,), float(i + 1)) for i, s in enumerate(SIZES)]
    return H.flat_params(SIZES, [(s,) for s in SIZES], vals, "cpu", **kw)


def test_flat_params_layout_and_gaps():
    ps, fp, fg, offs = _flat()
    assert offs == [0, 64, 128, 192] and fp.numel() == fg.numel() == 384
    gaps = H.gaps(ps, fp)
    assert int(gaps.sum()) == 191 and (fp[gaps] == 0).all() and torch.isnan(fg[gaps]).all()
    for i, (p, o, s) in enumerate(zip(ps, offs, SIZES)):
        assert p.data_ptr() == fp.data_ptr() + 4 * o and p.grad.data_ptr() == fg.data_ptr() + 4 * o
        assert (p == i + 1).all() and not gaps[o:o + s].any()
    assert torch.equal(H.gather(ps), torch.cat([torch.full((s,), float(i + 1)) for i, s in enumerate(SIZES)]))
    H.set_grads(ps, [torch.full((s,), 3.0) for s in SIZES], mult=0.5)
    assert (fg[~gaps] == 1.5).all() and torch.isnan(fg[gaps]).all()
    _, fp0, fg0, _ = _flat(grad_fill=0.0)
    assert (fg0[gaps] == 0).all() and torch.equal(fp0, fp)
    assert _flat(order=[3, 0, 1, 2])[3] == [128, 192, 256, 0]


def test_separate_storages_do_not_alias():
    ps, fp, fg, _ = _flat(separate=True)
    spans = sorted((t.data_ptr(), t.data_ptr() + 4 * t.numel()) for p in ps for t in (p, p.grad))
    assert len(spans) == 8 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    lo, hi = fp.data_ptr(), fp.data_ptr() + 4 * fp.numel()
    assert all(b <= lo or a >= hi for a, b in spans) and (fp == 0).all()
    assert all((p == i + 1).all() and (p.grad == 0).all() for i, p in enumerate(ps))


# ---- model scale ---------------------------------------------------------------------------------------------------------------------------
class _FlatStub:
    """two parameters as views of a flat array with a gap between them and padding behind: what the model-scale helpers read of a flat model"""

    def __init__(self):
        self.flat_params, self.flat_grads = torch.zeros(192), torch.zeros(192)
        self.views = [("a", self.flat_params[0:5].view(5)), ("b", self.flat_params[64:64 + 70].view(7, 10))]

    def parameters(self):
        return [p for _, p in self.views]

    def named_parameters(self):
        return list(self.views)


def test_padding_mask_and_grads_for_on_a_stub():
    m = _FlatStub()
    mask = H.padding_mask(m)
    want = torch.ones(192, dtype=torch.bool)
    want[0:5], want[64:134] = False, False
    assert torch.equal(mask, want)
    g = H.grads_for(m, 7)
    assert torch.isnan(g[mask]).all() and torch.isfinite(g[~mask]).all() and g[~mask].abs().max() < 0.1 and (g[~mask] != 0).all()
    assert torch.equal(g[~mask].view(torch.int32), H.grads_for(m, 7)[~mask].view(torch.int32))
    g0 = H.grads_for(m, 7, pad=0.0)
    assert (g0[mask] == 0).all() and torch.equal(g0[~mask], g[~mask])
    assert not torch.equal(H.grads_for(m, 8, pad=0.0), g0)
    gen = torch.Generator().manual_seed(7 * 1000 + 1)  # the draw of parameter 1 under seed 7
    assert torch.equal(g0[64:134], torch.randn((70,), generator=gen) * 1e-2)
