"""The fp32 Winograd weight gradient on split-bf16 products (csrc/wgrad3_wino.hip): a step takes TWO units (the K = 16 of
v_mfma_f32_32x32x16_bf16), an odd last unit is paired with a unit of zeros, and the two units of a pair may belong to two images
(each then needs its own GroupNorm rows).  vae_wgrad_wino + vae_wgrad_wino_reduce are called as in
tests/test_wgrad_stagger_gpu.py (whose launch and check helpers are used here), at the smallest shapes at which the pairing can
go wrong, against torch's conv2d weight gradient in float64 on the host.

Bars, those of that file: dW within 3e-5 of max |dW|; |db - ref| <= n * 2^-24 * sum |dy|.  Every launch is made twice
(bit-identical slabs); a split without units leaves zeros.  The crafted case compares the slab itself with float64 on the
scale sum |V| |D'| under the bar tests/test_wgrad_x3_host.py derives (tests/wgrad_x3_refs.py): between the emulated correct
form's error and the smallest single mistake's (a dropped or doubled term, swapped planes, a stale partner unit)."""
import pytest
import torch

import wgrad_x3_refs as R
from guarded import GuardedPool
from test_wgrad_stagger_gpu import _case, _check, _launch, _nan, _operands
from vaehip import ops

pytestmark = pytest.mark.gpu


# W = 16: H / 2 units.  In 2 splits 3 and 5 units start the second range on unit 2 and 3 (odd); 3 units in 4 splits: ranges of one
# unit starting on odd units and an empty split; 5 in 4: 2 + 2 + 1 + 0
@pytest.mark.parametrize("ns", [1, 2, 4])
@pytest.mark.parametrize("units", [1, 2, 3, 4, 5])
def test_units_per_split(cuda, units, ns):
    _case(cuda, 1, 2 * units, 16, 32, 128, ns)


@pytest.mark.parametrize("xf", [ops.XF_AFFINE_SILU, ops.XF_AFFINE])
@pytest.mark.parametrize("B,H,W,Ci,ns", [(3, 2, 16, 32, 1), (2, 2, 16, 64, 2), (3, 2, 32, 64, 1)])
def test_pairs_across_images(cuda, xf, B, H, W, Ci, ns):
    """one unit per image (pairs (0, 1) and (2, zeros): both units of the first pair need their own GroupNorm rows); one unit per
    split and image; two units per image at W = 32"""
    _case(cuda, B, H, W, Ci, 128, ns, xf)


@pytest.mark.parametrize("ns", [1, 2])
def test_crafted_operands(cuda, ns):
    """3 units (24 tiles) of operands every term has a known share of: the slab, summed over the splits, against float64"""
    B, H, W, Ci, Co = 1, 6, 16, 32, 128
    x, dy = R.crafted_xy(B, H, W, Ci, Co, 24)
    V, D = R.transforms(x, dy)
    ref, S = R.reference(V, D)
    e_ok = R.rel_err(R.emulate(V, D), ref, S)
    e_bad = min(R.rel_err(M, ref, S) for M in R.mistakes(V, D).values())
    bar = R.bar_between(e_ok, e_bad)
    r = dict(x=x.to(cuda), dy=dy.to(cuda))
    one = _launch(r, B, H, W, Ci, Co, ns, ops.XF_NONE, False, _nan(cuda))
    two = _launch(r, B, H, W, Ci, Co, ns, ops.XF_NONE, False, _nan(cuda))
    assert torch.equal(one[0], two[0]), "two launches differ in the slab"
    M = one[0].double().sum(dim=0).reshape(16, Ci, Co).cpu()
    live = S > 0
    assert not bool(M[~live].any()), "a position without products is not exactly zero"
    e = float(((M - ref).abs()[live] / S[live]).max())
    print(f"nsplit {ns}: device {e:.3e}, emulated {e_ok:.3e}, smallest single mistake {e_bad:.3e}, bar {bar:.3e} of sum|V||D'|")
    assert e < bar


def test_in_guarded_memory(cuda):
    """3 units in 2 splits behind GroupNorm + SiLU, operands and outputs between poisoned guards: every element written,
    nothing outside touched, no operand changed"""
    B, H, W, Ci, Co, ns, xf = 3, 2, 16, 32, 128, 2, ops.XF_AFFINE_SILU
    r = _operands(cuda, B, H, W, Ci, Co, xf)
    pool = GuardedPool(cuda)
    x, dy = pool.put(r["x"], "x"), pool.put(r["dy"], "dy")
    rg = dict(r, scale=pool.put(r["scale"], "scale"), shift=pool.put(r["shift"], "shift"))
    pool.snapshot()
    _, _, dW, db = _launch(rg, B, H, W, Ci, Co, ns, xf, True, lambda shape, label: pool.alloc(shape, label=label), x=x, dy=dy)
    torch.cuda.synchronize()
    assert pool.violations() == [] and pool.changed() == [] and pool.unwritten_report() == []
    _check(r, dW, db, "guarded")
