"""tests/upwgrad_x3_refs.py on the CPU: the transform-domain form of the upsampler weight gradient against torch in float64, the
emulated split-bf16 pair loop against float64, the float32 replay of the bias partials against the plain sum, and the two sides of
the crafted case's bar (the emulated correct form; every single mistake) for the split counts tests/test_upwgrad_x3_gpu.py runs."""
import pytest
import torch

import upwgrad_x3_refs as R


def _random(B, H, W, Ci, Co, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, Ci, generator=g), torch.randn(B, 2 * H, 2 * W, Co, generator=g)


@pytest.mark.parametrize("B,H,W", [(1, 1, 8), (2, 3, 8), (1, 2, 16)])
def test_transform_domain_is_the_weight_gradient(B, H, W):
    x, dy = _random(B, H, W, 5, 6)
    M, _ = R.reference(*R.transforms(x, dy, torch.float64))
    gw, _ = R.dw_f64(x, dy)
    assert float((R.output(M) - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


def test_unit_ranges():
    assert R.unit_ranges(2, 4) == [(0, 1), (1, 1), (2, 0), (3, 0)]
    assert R.unit_ranges(10, 4) == [(0, 3), (3, 3), (6, 3), (9, 1)]
    assert R.unit_ranges(5, 2) == [(0, 3), (3, 2)]


@pytest.mark.parametrize("ns", [1, 2, 4])
def test_emulated_loop_against_float64(ns):
    """random operands, 5 units: six of the nine plane products and fp32 accumulation stay within a few 2^-24 of sum |V| |D|"""
    x, dy = _random(1, 5, 8, 8, 8)
    V, D = R.transforms(x, dy)
    ref, S = R.reference(V, D)
    e = R.rel_err(R.emulate(V, D, ns).sum(dim=0), ref, S)
    assert e < 8 * 2.0 ** -24, e


@pytest.mark.parametrize("ns", [1, 2, 4])
def test_bias_replay(ns):
    _, dy = _random(2, 3, 16, 4, 8)
    got = R.bias_partials_f32(dy, 16, ns)
    n = dy.shape[0] * dy.shape[1] * dy.shape[2]
    assert got.shape == (ns, 8)
    assert bool(((got.double().sum(dim=0) - dy.double().sum(dim=(0, 1, 2))).abs() <= n * 2.0 ** -24 * dy.double().abs().sum(dim=(0, 1, 2))).all())


@pytest.mark.parametrize("ns", [1, 2])
def test_crafted_sides_are_apart(ns):
    """the crafted case of the GPU test: every single mistake lands at least 4 x beyond the emulated correct form (bar_between
    asserts it), the stale partner among them; all nine positions receive products"""
    x, dy = R.crafted_xy(1, 3, 8, 32, 128, 24)
    V, D = R.transforms(x, dy)
    ref, S = R.reference(V, D)
    assert all(bool((S[p] > 0).any()) for p in range(9))
    e_ok = R.rel_err(R.emulate(V, D, ns).sum(dim=0), ref, S)
    errs = {k: R.rel_err(M, ref, S) for k, M in R.mistakes(V, D, ns).items()}
    assert "odd unit paired with stale data" in errs
    bar = R.bar_between(e_ok, min(errs.values()))
    print(f"nsplit {ns}: emulated {e_ok:.3e}, mistakes {min(errs.values()):.3e} .. {max(errs.values()):.3e}, bar {bar:.3e}")
    assert e_ok < bar < min(errs.values())
