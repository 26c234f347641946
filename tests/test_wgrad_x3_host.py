"""The arithmetic of the Winograd weight gradient's split-bf16 products (csrc/wgrad3_wino.hip), emulated in torch on the CPU
(tests/wgrad_x3_refs.py): F(3x3,2x2) transforms in fp32, every V and D' value split into three bf16 planes, a step of 16 tiles
(two units) adds the six plane products, smallest first, to an fp32 accumulator.  This file pins the error model the crafted
case of tests/test_wgrad_x3_gpu.py rests on; it launches nothing.

Crafted operands pass the transforms unsummed, so every term has its known share of a product: hi.lo = lo.hi = 5.72e-6,
mid.mid = 8.58e-6, hi.mid = mid.hi = 2.93e-3 of hi.hi.  Per K the correct form's error against float64 and the error of every
single mistake (a term dropped, a term doubled, two planes swapped, an odd last unit paired with stale data instead of zeros)
are measured on the scale sum |V| |D'|; the bar is NOT a number written here but the geometric mean of the two measured sides,
and it only counts as a bar if the smallest mistake is at least 4 x the correct form's error.  Measured (printed by the test):
K = 8: 8.9e-8 against 5.71e-6;  K = 24: 1.6e-7 against 5.79e-6;  K = 4096: 1.0e-6 against 6.27e-6 (fp32 accumulation over 256
steps is what grows).  K = 4096 is 512 units, an even count: the stale-partner mistake exists at K = 8 and 24 only."""
import pytest
import torch

import wgrad_x3_refs as R

# K (tiles) -> B, H, W of the map: K = B * H/2 * W/2
MAPS = {8: (1, 2, 16), 24: (1, 6, 16), 4096: (1, 128, 128)}


@pytest.mark.parametrize("K", [8, 24, 4096])
def test_crafted_operands_pass_the_transforms_unsummed(K):
    B, H, W = MAPS[K]
    x, dy = R.crafted_xy(B, H, W, 8, 8, K)
    V, D = R.transforms(x, dy)
    assert V.shape[0] == K
    V64, D64 = R.transforms(x, dy, torch.float64)
    assert torch.equal(V.double(), V64) and torch.equal(D.double(), D64), "a transform rounded: a value is a sum of operands"
    for t, src in ((V, x), (D, dy)):
        vals = set(t.abs().unique().tolist())
        assert vals <= set(src.abs().unique().tolist()), "a transformed value is not plus or minus one operand"
    hi, mid, lo = R.split(V)
    nz = V != 0
    assert torch.equal(mid[nz], hi[nz] * (0.75 * 2.0 ** -8)) and torch.equal(lo[nz], hi[nz] * (0.375 * 2.0 ** -16))


@pytest.mark.parametrize("K", [8, 24, 4096])
def test_six_terms_reach_float64_and_every_single_mistake_shows(K):
    B, H, W = MAPS[K]
    x, dy = R.crafted_xy(B, H, W, 8, 8, K)
    V, D = R.transforms(x, dy)
    ref, S = R.reference(V, D)
    e_ok = R.rel_err(R.emulate(V, D), ref, S)
    bad = {name: R.rel_err(M, ref, S) for name, M in R.mistakes(V, D).items()}
    worst = min(bad, key=bad.get)
    print(f"K={K}: correct form {e_ok:.3e} of sum|V||D'|; smallest single mistake: {worst} {bad[worst]:.3e}")
    for name, e in sorted(bad.items(), key=lambda kv: kv[1]):
        print(f"K={K}:   {name}: {e:.3e}")
    assert ((K // 8) % 2 == 1) == ("odd unit paired with stale data" in bad)
    bar = R.bar_between(e_ok, bad[worst])
    print(f"K={K}: bar {bar:.3e}")
    assert e_ok < bar
    for name, e in bad.items():
        assert e > bar, f"K={K}: {name} stays inside the bar ({e:.3e} <= {bar:.3e})"


@pytest.mark.parametrize("K", [8, 24, 4096])
def test_random_operands_stay_at_fp32_accumulation_accuracy(K):
    """N(0,1) operands, error on the scale of the result's max, printed beside an fp32 matmul's over the same V and D'.
    The bound is that of the accumulation, not of the split: an accumulator receives n = 6 K / 16 fp32 additions, each rounding
    by at most 2^-24 of a partial sum that stays within the result's scale; independent roundings add up as sqrt(n).  One more
    2^-24 covers the split itself (six terms leave <= 2^-25 of a product out) and the fp32 transforms: (sqrt(6 K / 16) + 1) 2^-24,
    i.e. 1.6e-7, 2.4e-7 and 2.4e-6 -- at K = 4096 a twelfth of the dW bar (3e-5) of the kernel's tests."""
    B, H, W = MAPS[K]
    g = torch.Generator().manual_seed(K)
    x, dy = torch.randn(B, H, W, 8, generator=g), torch.randn(B, H, W, 8, generator=g)
    V, D = R.transforms(x, dy)
    V64, D64 = R.transforms(x, dy, torch.float64)
    ref, _ = R.reference(V64, D64)
    e = float((R.emulate(V, D).double() - ref).abs().max() / ref.abs().max())
    e32 = float(((V.permute(1, 2, 0) @ D.permute(1, 0, 2)).double() - ref).abs().max() / ref.abs().max())
    bound = ((6 * K / 16) ** 0.5 + 1) * 2.0 ** -24
    print(f"K={K}: split {e:.3e}, fp32 matmul {e32:.3e} of the result's max; bound {bound:.3e}")
    assert e <= bound
