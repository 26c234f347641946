"""csrc/recon_loss.hip through vaehip.ops (ops.recon_loss, ops.ssim_index): the pixel losses with their gradient seed, the
unclamped SSIM term and its gradient, the final pass.  References, inputs and bars: tests/recon_loss_refs.py (the bars are
derived there, and tests/test_recon_loss_host.py shows what they accept and reject)."""
import ctypes as C

import pytest
import torch

import recon_loss_refs as rr

pytestmark = pytest.mark.gpu

DELTA = 0.5
PIXEL_N = [1, 3, 255, 256, 257, 4 * 4096 + 1]
_CACHE = {}


def _spec(kind="mse", weight=0.0, delta=DELTA):
    from vaehip.losses import ReconLoss
    return ReconLoss(kind, delta, weight)


def _klp(cuda, B=1):
    """KL partials as sample_kl leaves them: [B][blocks]; their mean over B is scalars[1]"""
    return torch.arange(1, 2 * B + 1, device=cuda, dtype=torch.float32).reshape(B, 2)


def _tile():
    from vaehip import ops
    return ops.ssim_tile()


# ---------------------------------------------------------------------------------------------------------- pixel
def _check_pixel(got, r, x, kind, scale, klp, klw, what):
    sc, terms, d = got
    ref = rr.reference(r, x, kind, DELTA, 0.0, scale)
    want = rr.pixel_seed_fp32(r, x, kind, DELTA, scale)
    sc, terms, d = sc.cpu(), terms.cpu(), d.cpu()
    rel = abs(float(sc[0]) - ref["pixel"]) / max(abs(ref["pixel"]), 1e-300)
    print(f"{what}: loss {float(sc[0]):.9g} against {ref['pixel']:.9g} (relative {rel:.2e}, bar {rr.LOSS_REL:.2e}), "
          f"seed bitwise {torch.equal(d, want)}")
    assert torch.equal(d, want), (what, int((d != want).sum()))
    assert rr.seed_ok(d, ref)   # the fp32 expression itself sits inside the float64 bar, so this adds nothing but a cross-check
    assert rr.loss_ok(float(sc[0]), ref["pixel"]), (what, float(sc[0]), ref["pixel"])
    assert float(terms[0]) == float(sc[0]) and bool(torch.isnan(terms[1]))
    kl = float(klp.double().sum() / klp.shape[0])
    assert float(sc[1]) == pytest.approx(kl, rel=1e-6)
    assert float(sc[2]) == pytest.approx(ref["pixel"] + klw * kl, rel=1e-6)


@pytest.mark.parametrize("scale", [1.0, 0.25])
@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("n", PIXEL_N)
def test_pixel_loss_and_seed(cuda, n, kind, scale):
    from vaehip import ops
    r, x = rr.pixel_inputs(n)
    klp = _klp(cuda)
    got = ops.recon_loss(r.to(cuda), x.to(cuda), klp, 1e-3, _spec(kind), scale)
    _check_pixel(got, r, x, kind, scale, klp.cpu(), 1e-3, f"n={n} {kind} scale={scale}")


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("which", ["all", "recon", "target"])
def test_pixel_off_16_byte_alignment(cuda, kind, which):
    """operands 4 bytes behind a 16-byte boundary, both or one alone: scalar accesses throughout"""
    from vaehip import ops
    n = 4 * 4096 + 1
    r, x = rr.pixel_inputs(n, seed=1)

    def place(t, off):
        buf = torch.zeros(n + 8, device=cuda)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + n]
        v.copy_(t)
        return v
    rd = place(r, 1 if which in ("all", "recon") else 0)
    xd = place(x, 1 if which in ("all", "target") else 0)
    assert rd.data_ptr() % 16 == (4 if which in ("all", "recon") else 0)
    klp = _klp(cuda)
    _check_pixel(ops.recon_loss(rd, xd, klp, 1e-3, _spec(kind), 0.25), r, x, kind, 0.25, klp.cpu(), 1e-3, f"offset {which} {kind}")


def test_loss_only(cuda):
    from vaehip import ops
    r, x = rr.pixel_inputs(257)
    sc, terms, d = ops.recon_loss(r.to(cuda), x.to(cuda), _klp(cuda), 0.0, _spec("huber"), want_grad=False)
    assert d is None and rr.loss_ok(float(sc[0]), rr.reference(r, x, "huber", DELTA)["pixel"])


# ---------------------------------------------------------------------------------------------------------- SSIM
def _shapes():
    th, tw = 22, 32   # test_tile_shape holds these to the library
    return [(1, 3, 11, 11), (2, 3, 12, 37), (1, 3, 70, 33), (1, 3, th + 10, tw + 10), (1, 3, th + 11, tw + 11)]


SHAPES = _shapes()
VARIANTS = ["noisy", "flat", "range"]
WEIGHT = 0.2


def _case(shape, variant, kind="huber", scale=0.25):
    key = (tuple(shape), variant, kind, scale)
    if key not in _CACHE:
        p, t = rr.ssim_inputs(shape, variant)
        _CACHE[key] = (p, t, rr.reference(p, t, kind, DELTA, WEIGHT, scale), rr.ssim_index(p, t))
    return _CACHE[key]


def test_tile_shape(cuda):
    """the tile-edge shapes of SHAPES are one forward tile and one position more each way; the backward tiles are pixels"""
    from vaehip.lib import lib
    th, tw = _tile()
    assert (th + 10, tw + 10) == SHAPES[3][2:] and (th + 11, tw + 11) == SHAPES[4][2:]
    npart, nmaps = C.c_int64(0), C.c_int64(0)
    lib.call("vae_ssim_workspace", 1, 1, th + 10, tw + 10, C.byref(npart), C.byref(nmaps))
    assert (npart.value, nmaps.value) == (1, 3 * th * tw)
    lib.call("vae_ssim_workspace", 1, 1, th + 11, tw + 11, C.byref(npart), C.byref(nmaps))
    assert (npart.value, nmaps.value) == (4, 3 * (th + 1) * (tw + 1))
    lib.call("vae_ssim_workspace", 2, 3, 70, 33, C.byref(npart), C.byref(nmaps))
    assert (npart.value, nmaps.value) == (2 * 3 * 3 * 1, 3 * 2 * 3 * 60 * 23)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_index(cuda, shape, variant):
    from vaehip import ops
    p, t, _, want = _case(shape, variant)
    got = ops.ssim_index(p.to(cuda), t.to(cuda)).cpu()
    assert got.dtype == torch.float64 and got.shape == want.shape
    print(f"{shape} {variant}: SSIM index absolute error {float((got - want).abs().max()):.2e} (bar {rr.INDEX_ABS:.0e})")
    assert rr.index_ok(got, want)


@pytest.mark.parametrize("shape", [(2, 3, 12, 37), (1, 3, 70, 33)], ids=lambda s: "x".join(map(str, s)))
def test_identical_inputs_give_exactly_one(cuda, shape):
    from vaehip import ops
    for variant in ("noisy", "range"):
        p = _case(shape, variant)[0].to(cuda)
        assert ops.ssim_index(p, p.clone()).tolist() == [1.0] * shape[0]


def _check_seed(got, ref, what):
    sc, terms, d = (v.cpu() for v in got)
    ex = rr.seed_excess(d, ref)
    print(f"{what}: seed error / bound {ex:.3f}; rec {float(sc[0]):.9g} against {ref['rec']:.9g}, ssim {float(terms[1]):.9g} "
          f"against {ref['ssim']:.9g}")
    assert ex <= 1.0, (what, ex)
    assert rr.loss_ok(float(terms[0]), ref["pixel"]) and rr.loss_ok(float(terms[1]), ref["ssim"]) and rr.loss_ok(float(sc[0]), ref["rec"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_combined_seed(cuda, shape, variant):
    """huber + 0.2 (1 - ssim) at grad_scale 0.25, (B, C, H, W) tensors read in place"""
    from vaehip import ops
    p, t, ref, _ = _case(shape, variant)
    got = ops.recon_loss(p.to(cuda), t.to(cuda), _klp(cuda, shape[0]), 1e-3, _spec("huber", WEIGHT), 0.25, layout="nchw")
    _check_seed(got, ref, f"{shape} {variant}")


def test_layouts(cuda):
    """the engine's NHWC tensors against contiguous NCHW: index bitwise equal, seed bitwise equal after the permutation"""
    from vaehip import ops
    shape = (2, 3, 33, 43)   # two backward pixel tiles each way: 22 + 11 rows, 32 + 11 columns
    p, t, ref, want = _case(shape, "noisy", "l1", 1.0)
    pd, td = p.to(cuda), t.to(cuda)
    pl, tl = pd.permute(0, 2, 3, 1).contiguous(), td.permute(0, 2, 3, 1).contiguous()
    base = ops.ssim_index(pd, td)
    assert rr.index_ok(base, want)
    assert torch.equal(ops.ssim_index(pl.permute(0, 3, 1, 2), tl.permute(0, 3, 1, 2)), base)
    assert torch.equal(ops.ssim_index(pl.permute(0, 3, 1, 2), td), base)
    klp = _klp(cuda, 2)
    a = ops.recon_loss(pd, td, klp, 1e-3, _spec("l1", WEIGHT), 1.0, layout="nchw")
    b = ops.recon_loss(pl, tl, klp, 1e-3, _spec("l1", WEIGHT), 1.0)
    _check_seed(a, ref, "nchw")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[2].permute(0, 3, 1, 2), a[2])


def test_offsets_past_2_gib(cuda):
    """two images of one tensor whose batch stride puts image 1 more than 2^31 bytes behind image 0 (every offset is 64-bit)"""
    from vaehip import ops
    n = int(2.25 * 2 ** 30) // 4
    buf = torch.empty(n, device=cuda, dtype=torch.float32)
    stride_b = 2 ** 29 + 1024 + 4  # elements: 2^31 + 4112 bytes
    p, t = rr.ssim_inputs((2, 3, 16, 16), "noisy")
    want = rr.ssim_index(p, t)
    view = torch.as_strided(buf, (2, 3, 16, 16), (stride_b, 256, 16, 1), storage_offset=12)
    assert (view[1].data_ptr() - view[0].data_ptr()) > 2 ** 31 and 12 + stride_b + 768 <= n
    view.copy_(p.to(cuda))
    assert rr.index_ok(ops.ssim_index(view, t.to(cuda)), want)
    view.copy_(t.to(cuda))
    assert rr.index_ok(ops.ssim_index(p.to(cuda), view), want)


# ---------------------------------------------------------------------------------------------------------- both
def test_repeatable(cuda):
    from vaehip import ops
    p, t, _, _ = _case((1, 3, 70, 33), "noisy")
    pd, td, klp = p.to(cuda), t.to(cuda), _klp(cuda)
    a = ops.recon_loss(pd, td, klp, 1e-3, _spec("huber", WEIGHT), 0.25, layout="nchw")
    b = ops.recon_loss(pd, td, klp, 1e-3, _spec("huber", WEIGHT), 0.25, layout="nchw")
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(ops.ssim_index(pd, td), ops.ssim_index(pd, td))
    r, x = rr.pixel_inputs(4 * 4096 + 1)
    a = ops.recon_loss(r.to(cuda), x.to(cuda), klp, 1e-3, _spec("l1"), 1.0)
    b = ops.recon_loss(r.to(cuda), x.to(cuda), klp, 1e-3, _spec("l1"), 1.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_bad_arguments_launch_nothing(cuda):
    """every refusal is VAE_EINVAL with a message, before a launch: the buffers handed in keep their fill"""
    from vaehip.lib import lib, VaeHipError
    from vaehip import ops
    f = torch.full((64 * 64 * 3,), 7.0, device=cuda)
    dbl = torch.full((4096,), 7.0, device=cuda, dtype=torch.float64)
    out = torch.full((64 * 64 * 3,), 7.0, device=cuda)
    s, P = ops._stream(), ops._p
    st = (64 * 64 * 3, 64 * 64, 64, 1)
    n = f.numel()
    bad = [
        ("vae_pixel_loss", (None, P(f), n, 0, 1.0, 1.0, P(dbl), P(out), s), "null"),
        ("vae_pixel_loss", (P(f), None, n, 0, 1.0, 1.0, P(dbl), P(out), s), "null"),
        ("vae_pixel_loss", (P(f), P(f), n, 0, 1.0, 1.0, None, P(out), s), "null"),
        ("vae_pixel_loss", (P(f), P(f), 0, 0, 1.0, 1.0, P(dbl), P(out), s), "n=0"),
        ("vae_pixel_loss", (P(f), P(f), n, 3, 1.0, 1.0, P(dbl), P(out), s), "unknown kind"),
        ("vae_pixel_loss", (P(f), P(f), n, -1, 1.0, 1.0, P(dbl), P(out), s), "unknown kind"),
        ("vae_pixel_loss", (P(f), P(f), n, 2, 0.0, 1.0, P(dbl), P(out), s), "delta"),
        ("vae_pixel_loss", (P(f), P(f), n, 2, -0.5, 1.0, P(dbl), P(out), s), "delta"),
        ("vae_ssim_fwd", (None, *st, P(f), *st, 1, 3, 64, 64, P(dbl), None, s), "null"),
        ("vae_ssim_fwd", (P(f), *st, P(f), *st, 1, 3, 64, 64, None, None, s), "null"),
        ("vae_ssim_fwd", (P(f), *st, P(f), *st, 1, 3, 10, 64, P(dbl), None, s), "smaller than"),
        ("vae_ssim_fwd", (P(f), *st, P(f), *st, 1, 3, 64, 10, P(dbl), None, s), "smaller than"),
        ("vae_ssim_bwd", (P(f), *st, P(f), *st, None, 1, 3, 64, 64, 1.0, P(out), *st, s), "null"),
        ("vae_ssim_bwd", (P(f), *st, P(f), *st, P(dbl), 1, 3, 64, 64, 1.0, None, *st, s), "null"),
        ("vae_ssim_bwd", (P(f), *st, P(f), *st, P(dbl), 1, 3, 10, 64, 1.0, P(out), *st, s), "smaller than"),
        ("vae_ssim_index", (P(dbl), 1, 3, 10, 64, P(dbl), s), "smaller than"),
        ("vae_ssim_index", (None, 1, 3, 64, 64, P(dbl), s), "null"),
        ("vae_recon_loss_final", (None, n, None, 1, 3, 64, 64, 0.0, P(f), 1, 0.0, P(out), P(out), s), "null"),
        ("vae_recon_loss_final", (P(dbl), n, P(dbl), 1, 3, 10, 64, 0.1, P(f), 1, 0.0, P(out), P(out), s), "smaller than"),
        ("vae_recon_loss_final", (P(dbl), n, None, 1, 3, 64, 64, -0.1, P(f), 1, 0.0, P(out), P(out), s), "ssim_weight"),
    ]
    for name, args, match in bad:
        with pytest.raises(VaeHipError, match=match):
            lib.call(name, *args)
    npart, nmaps = C.c_int64(0), C.c_int64(0)
    for H, W in ((10, 64), (64, 10)):
        with pytest.raises(VaeHipError, match="smaller than"):
            lib.call("vae_ssim_workspace", 1, 3, H, W, C.byref(npart), C.byref(nmaps))
    assert lib.query("vae_pixel_loss_blocks", 0) == -1 and lib.query("vae_ssim_tile", 2) == -1
    torch.cuda.synchronize()
    assert bool((f == 7).all()) and bool((dbl == 7).all()) and bool((out == 7).all())
    # the Python layer refuses before it allocates
    ok = torch.zeros((1, 3, 64, 64), device=cuda)
    small = torch.zeros((1, 3, 10, 64), device=cuda)
    half = ok.bfloat16()
    klp = _klp(cuda)
    before = torch.cuda.memory_stats(cuda)["allocation.all.allocated"]
    with pytest.raises(ValueError, match="ssim_index"):
        ops.ssim_index(small, small)
    with pytest.raises(ValueError, match="recon_loss"):
        ops.recon_loss(small, small, klp, 0.0, _spec("l1", WEIGHT), layout="nchw")
    with pytest.raises(ValueError, match="recon_loss"):
        ops.recon_loss(ok, small, klp, 0.0, _spec("l1"))
    with pytest.raises(ValueError, match="recon_loss"):
        ops.recon_loss(ok, half, klp, 0.0, _spec("l1"))
    assert torch.cuda.memory_stats(cuda)["allocation.all.allocated"] == before


@pytest.mark.parametrize("case", ["pixel", "ssim"])
def test_guarded_memory(cuda, case):
    """operands 4 bytes off alignment between poisoned guards, results and workspaces from the guarded pool: no store outside
    them, no element of drecon, scalars, terms or a workspace left unwritten, and the values still meet their bars"""
    from guarded import GuardedPool, guarded
    from vaehip import ops
    pool = GuardedPool(cuda)
    if case == "pixel":
        r, x = rr.pixel_inputs(4 * 4096 + 1)
        spec, layout, scale, extra = _spec("huber"), "nhwc", 0.25, 4   # partials, drecon, scalars, terms
    else:
        r, x, ref, _ = _case((1, 3, 70, 33), "noisy")
        spec, layout, scale, extra = _spec("huber", WEIGHT), "nchw", 0.25, 6   # ... and the SSIM partials and maps
    rg, xg = pool.put(r, "recon", offset_bytes=4), pool.put(x, "target", offset_bytes=4)
    klp = pool.put(_klp(cuda).cpu(), "kl_partial")
    pool.snapshot()
    n0 = len(pool.blocks)
    with guarded(pool, ops):
        got = ops.recon_loss(rg, xg, klp, 1e-3, spec, scale, layout=layout)
    torch.cuda.synchronize()
    assert len(pool.blocks) == n0 + extra, [b.label for b in pool.blocks]
    assert pool.violations() == []
    assert pool.unwritten_report() == []
    assert pool.changed() == []
    if case == "pixel":
        _check_pixel(got, r, x, "huber", scale, klp.cpu(), 1e-3, "guarded pixel")
    else:
        _check_seed(got, ref, "guarded ssim")
