"""ops.image_metrics (csrc/image_metrics.hip): the fused device kernel behind evaluate.py's Average MSE / PSNR / SSIM, held to
the project's CPU definition (evaluate.to_unit / psnr_sums / ssim_per_image in float64) and to closed forms independent of it.

Bars.  The kernel's operands are the same fp32 values the CPU reference widens to float64 (u(x) is evaluated in fp32 on both
sides), and everything after them is float64 on both sides, so the two differ by summation order only: over the <= 2e5 terms
of these shapes that is at most N * 2^-53 ~ 2e-11 relative.  Hence SSIM within 1e-10 absolute, both squared-error sums within
1e-10 relative, and exactly 0.0 for identical inputs.  An fp32 window statistic is off by 1e-4 on flat regions
(evaluate.ssim_per_image's docstring) and cannot meet this; that is the point of the bar."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from evaluate import ssim_per_image, to_unit

pytestmark = pytest.mark.gpu

C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE_H, TILE_W = 22, 32  # window positions per workgroup (csrc/image_metrics.hip); test_tile_shape holds this to the library
SHAPES = [(1, 3, 11, 11), (2, 3, 12, 37), (3, 1, 40, 48), (2, 3, 64, 64), (1, 3, 70, 33),
          (1, 3, TILE_H + 10, TILE_W + 10), (1, 3, TILE_H + 11, TILE_W + 11)]
_CACHE = {}


def _inputs(shape, variant):
    """target uniform in [-1.2, 1.2] (the clamp acts); prediction noisy, or nearly flat: 1e-3 on every third column"""
    g = torch.Generator().manual_seed(1000 + sum(s * 7 ** i for i, s in enumerate(shape)))
    t = torch.rand(shape, generator=g) * 2.4 - 1.2
    if variant == "noisy":
        p = t + 0.2 * torch.randn(shape, generator=g)
    else:
        p = t.clone()
        p[..., ::3] += 1e-3
    return p, t


def _reference(p, t):
    """[B, 3] float64 on the CPU, from the project's own definition"""
    up, ut = to_unit(p).double(), to_unit(t).double()
    B = p.shape[0]
    return torch.stack([((p.double() - t.double()) ** 2).reshape(B, -1).sum(-1), ((up - ut) ** 2).reshape(B, -1).sum(-1),
                        ssim_per_image(up, ut)], dim=1)


def _case(shape, variant):
    key = (tuple(shape), variant)
    if key not in _CACHE:
        p, t = _inputs(shape, variant)
        _CACHE[key] = (p, t, _reference(p, t))
    return _CACHE[key]


def _check(got, ref, what=""):
    got = got.cpu()
    assert got.dtype == torch.float64 and got.shape == ref.shape
    sse_rel = ((got[:, :2] - ref[:, :2]).abs() / ref[:, :2].abs().clamp_min(1e-300)).max().item()
    ssim_abs = (got[:, 2] - ref[:, 2]).abs().max().item()
    print(f"{what}: SSE relative error {sse_rel:.2e}, SSIM absolute error {ssim_abs:.2e} (bars 1e-10)")
    assert bool(torch.isfinite(got).all()), got
    assert sse_rel <= 1e-10, (what, got, ref)
    assert ssim_abs <= 1e-10, (what, got, ref)


def test_tile_shape(cuda):
    """the two tile-edge shapes of SHAPES really are one tile, and one more in both directions"""
    from vaehip.lib import lib
    n = C.c_int64(0)
    lib.call("vae_image_metrics_workspace", 1, 1, TILE_H + 10, TILE_W + 10, C.byref(n))
    assert n.value == 3
    lib.call("vae_image_metrics_workspace", 1, 1, TILE_H + 11, TILE_W + 11, C.byref(n))
    assert n.value == 4 * 3


@pytest.mark.parametrize("variant", ["noisy", "flat"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_cpu_definition(cuda, shape, variant):
    from vaehip import ops
    p, t, ref = _case(shape, variant)
    _check(ops.image_metrics(p.to(cuda), t.to(cuda)), ref, f"{shape} {variant}")


@pytest.mark.parametrize("shape", [(2, 3, 12, 37), (1, 3, 70, 33)], ids=lambda s: "x".join(map(str, s)))
def test_identical_inputs(cuda, shape):
    from vaehip import ops
    _, t, _ = _case(shape, "noisy")
    x = t.to(cuda)
    got = ops.image_metrics(x, x.clone()).cpu()
    assert got[:, 0].tolist() == [0.0] * shape[0] and got[:, 1].tolist() == [0.0] * shape[0]
    assert float((got[:, 2] - 1.0).abs().max()) <= 1e-10


def test_layouts_agree_bitwise(cuda):
    """channels-last view (what the engine returns), contiguous NCHW and a [1::2] batch slice of a larger tensor"""
    from vaehip import ops
    shape = (2, 3, 70, 33)
    p, t, ref = _case(shape, "noisy")
    pd, td = p.to(cuda), t.to(cuda)
    base = ops.image_metrics(pd, td)
    _check(base, ref, "contiguous")
    p_cl = pd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert p_cl.stride() != pd.stride() and p_cl.stride(1) == 1
    assert torch.equal(ops.image_metrics(p_cl, td), base)
    big_p = torch.zeros((5,) + shape[1:], device=cuda)
    big_t = torch.zeros((5,) + shape[1:], device=cuda)
    big_p[1::2], big_t[1::2] = pd, td
    assert torch.equal(ops.image_metrics(big_p[1::2], big_t[1::2]), base)
    assert torch.equal(ops.image_metrics(p_cl, big_t[1::2]), base)


def _window():
    ax = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-(ax / 1.5) ** 2 / 2)
    return g / g.sum()


@pytest.mark.parametrize("a,delta", [(0.25, 0.1), (0.6, -0.05), (0.0, 0.3)])
def test_constant_offset_closed_forms(cuda, a, delta):
    """constant target, constant prediction: variances and covariance vanish, SSIM is the luminance term.  The kernel takes
    images in [-1, 1]; the expected values come from the fp32 operands it sees, not from the decimal literals."""
    from vaehip import ops
    shape = (2, 3, 40, 45)
    t = torch.full(shape, 2 * a - 1)
    p = torch.full(shape, 2 * (a + delta) - 1)
    ua, up = float(to_unit(t)[0, 0, 0, 0].double()), float(to_unit(p)[0, 0, 0, 0].double())
    numel = shape[1] * shape[2] * shape[3]
    got = ops.image_metrics(p.to(cuda), t.to(cuda)).cpu()
    want_ssim = (2 * ua * up + C1) / (ua * ua + up * up + C1)
    raw = float(p[0, 0, 0, 0].double() - t[0, 0, 0, 0].double())
    for b in range(shape[0]):
        assert float(got[b, 0]) == pytest.approx(numel * raw * raw, rel=1e-10)
        assert float(got[b, 1]) == pytest.approx(numel * (up - ua) ** 2, rel=1e-10)
        # the window weights sum to 1 within a few ulp, and mu^2 cancels against E[x^2] to about 1e-16 of c2 = 9e-4
        assert float(got[b, 2]) == pytest.approx(want_ssim, abs=1e-10)


def test_two_level_image_against_flat_image(cuda):
    """target: left half a, right half b (constant along y); prediction flat c: 1-D window sums, independent of ssim_per_image"""
    from vaehip import ops
    H, W = 32, 40
    t = torch.empty(1, 1, H, W)
    t[..., : W // 2] = 2 * 0.2 - 1
    t[..., W // 2:] = 2 * 0.8 - 1
    p = torch.full_like(t, 2 * 0.5 - 1)
    row = to_unit(t)[0, 0, 0].double().numpy()
    c = float(to_unit(p)[0, 0, 0, 0].double())
    g = _window()
    vals = []
    for x in range(W - 10):  # window positions wholly inside the image
        seg = row[x:x + 11]
        mu = float((seg * g).sum())
        var = float((seg * seg * g).sum()) - mu * mu
        vals.append(((2 * mu * c + C1) * C2) / ((mu * mu + c * c + C1) * (var + C2)))
    want = float(np.mean(vals))
    got = ops.image_metrics(p.to(cuda), t.to(cuda)).cpu()
    assert 0 < want < 1 and float(got[0, 2]) == pytest.approx(want, abs=1e-10)
    assert float(got[0, 1]) == pytest.approx(float(((row - c) ** 2).sum()) * H, rel=1e-10)


def test_repeatable(cuda):
    from vaehip import ops
    p, t, _ = _case((2, 3, 64, 64), "noisy")
    pd, td = p.to(cuda), t.to(cuda)
    assert torch.equal(ops.image_metrics(pd, td), ops.image_metrics(pd, td))


@pytest.mark.parametrize("offset_bytes", [0, 4])
def test_guarded_memory(cuda, offset_bytes):
    """operands between poisoned guards, once 256-byte aligned and once 4 bytes off; result and workspace from the guarded pool:
    no store outside them, no element of either left unwritten, and a load outside an operand would meet NaN and fail the bars"""
    from guarded import GuardedPool, guarded
    from vaehip import ops
    shape = (1, 3, 70, 33)
    p, t, ref = _case(shape, "noisy")
    pool = GuardedPool(cuda)
    pg = pool.put(p, "pred", offset_bytes=offset_bytes)
    tg = pool.put(t, "target", offset_bytes=offset_bytes)
    pool.snapshot()
    n0 = len(pool.blocks)
    with guarded(pool, ops):
        got = ops.image_metrics(pg, tg)
    torch.cuda.synchronize()
    assert len(pool.blocks) == n0 + 2, [b.label for b in pool.blocks]  # the workspace and the result
    assert pool.violations() == []
    assert pool.unwritten_report() == []
    assert pool.changed() == []
    _check(got, ref, f"guarded, offset {offset_bytes}")


def test_offsets_past_2_gib(cuda):
    """two images of one tensor whose batch stride puts image 1 more than 2^31 bytes behind image 0"""
    from vaehip import ops
    n = int(2.25 * 2 ** 30) // 4
    buf = torch.empty(n, device=cuda, dtype=torch.float32)
    stride_b = 2 ** 29 + 1024 + 4  # elements: 2^31 + 4112 bytes
    g = torch.Generator().manual_seed(7)
    t = torch.rand((2, 3, 16, 16), generator=g) * 2.4 - 1.2
    p = t + 0.2 * torch.randn((2, 3, 16, 16), generator=g)
    view = torch.as_strided(buf, (2, 3, 16, 16), (stride_b, 256, 16, 1), storage_offset=12)
    assert (view[1].data_ptr() - view[0].data_ptr()) > 2 ** 31 and 12 + stride_b + 768 <= n
    view.copy_(p.to(cuda))
    _check(ops.image_metrics(view, t.to(cuda)), _reference(p, t), "batch stride > 2 GiB (pred)")
    view.copy_(t.to(cuda))
    _check(ops.image_metrics(p.to(cuda), view), _reference(p, t), "batch stride > 2 GiB (target)")


def test_refusals_touch_nothing(cuda):
    from vaehip import ops
    ok = torch.zeros((1, 3, 64, 64), device=cuda)
    cases = [(torch.zeros((1, 3, 10, 64), device=cuda),) * 2, (torch.zeros((1, 3, 64, 10), device=cuda),) * 2,
             (ok, torch.zeros((1, 3, 64, 65), device=cuda)), (ok, ok.bfloat16()), (ok.bfloat16(), ok), (ok[0], ok[0])]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(cuda)
    stats0 = torch.cuda.memory_stats(cuda)["allocation.all.allocated"]
    for a, b in cases:
        with pytest.raises(ValueError, match="image_metrics"):
            ops.image_metrics(a, b)
    assert torch.cuda.memory_allocated(cuda) == before
    assert torch.cuda.memory_stats(cuda)["allocation.all.allocated"] == stats0  # no allocation was even attempted
    assert math.isfinite(float(ops.image_metrics(ok, ok)[0, 2]))  # the operator still serves a valid call afterwards
