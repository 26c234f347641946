"""The GroupNorm, tracker and dead-weight kernels (csrc/norm.hip: nine entry points; vae_dead_scan / vae_dead_scan_adaptive of
csrc/elementwise.hip) against the float64 references of tests/norm_refs.py, at the shapes and values where such kernels go
wrong: fewer pixels than the workgroup has rows, ragged and empty chunks, the clamped tail of the backward apply, grid-stride
trips, both grids of the statistics' final pass, constant groups, a large mean, an outlier as a thread's pivot, SiLU where exp
overflows, gamma == 0, one-hot gradients, bf16 storage; segment ends, chunk boundaries, unaligned starts and the strict `<` of
the scan.  tests/test_norm_edges_host.py proves every shape's and builder's property without a GPU.

The entry points are called through the C ABI with every workspace and output pre-filled with NaN (k_* below; one test holds
them to vaehip.ops bit for bit).  Bars: mean 1e-6 and rstd 2e-5 as test_groupnorm_statistics_with_large_mean has them; the
tensors max(4 x the error of torch's fp32 CPU arithmetic against float64, the bar of the plain-input test in
tests/test_kernels_gpu.py); never anything the kernel returned.  Every figure is printed and recorded next to its bar
(profiles/norm_edges_measured.json).

Two readings that the numbers forced, both measured on the CPU before a GPU saw the test:
  * constant group: the kernels apply y = x * scale + shift with shift = beta - mean * scale rounded to fp32, so the normalised
    value of a constant group is beta to within an ulp of mean * scale (rstd = 1000 there: 3e-5 for x = 0.7,
    gamma = 1.3), as it is in torch's fp32 CPU kernel, which has the same form.  mean, rstd and xhat == 0 are exact and are
    asserted bit for bit; y is held to beta by that format bound, element by element, and by the common bar as a tensor.
  * the large-mean apply keeps the absolute bar of the existing test, 3e-4 * max(1, ratio / 30): fp32 x itself carries
    ratio * 6e-8.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import norm_refs as nr

pytestmark = pytest.mark.gpu
K = nr.KIND
TARGET = (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.Linear, torch.nn.GroupNorm)
XF_AFFINE, XF_AFFINE_SILU = 1, 2


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), device=dev, dtype=dtype)


# ---------------------------------------------------------------------------------------------------- the ABI, poisoned
def k_stats(x, gamma, beta, eps=nr.EPS):
    """vae_gn_stats_partial + vae_gn_stats_final as ops.gn_stats calls them; every chunk, empty ones included, must have written
    its partial before the final pass reads it"""
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    nch = ops._gn_nchunk(B, H * W, Cc)
    ws = _nan((B, nch, nr.G, 2), x.device)
    lib.call("vae_gn_stats_partial", ops._p(x), ops._b16(x), B, H * W, Cc, nr.G, nch, ops._p(ws), ops._stream())
    assert not bool(ws.isnan().any()), "a chunk left its statistics partial unwritten"
    mean, rstd, scale, shift = _nan((B, nr.G), x.device), _nan((B, nr.G), x.device), _nan((B, Cc), x.device), _nan((B, Cc), x.device)
    lib.call("vae_gn_stats_final", ops._p(ws), B, H * W, Cc, nr.G, nch, ops._p(gamma), ops._p(beta), eps, ops._p(mean), ops._p(rstd),
             ops._p(scale), ops._p(shift), ops._stream())
    return ops.Stats(mean, rstd, scale, shift)


def k_apply(x, st, xf):
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    y = _nan(x.shape, x.device)
    lib.call("vae_gn_apply", ops._p(x), ops._b16(x), ops._p(st.scale), ops._p(st.shift), B, H * W, Cc, xf, ops._p(y), ops._stream())
    return y


def k_apply16(x, st, xf):
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    y = _nan(x.shape, x.device, torch.bfloat16)
    lib.call("vae_gn_apply_bf16", ops._p(x), ops._b16(x), ops._p(st.scale), ops._p(st.shift), B, H * W, Cc, xf, ops._p(y), ops._stream())
    return y


def k_track(x, st):
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    nch = ops._gn_nchunk(B, H * W, Cc)
    ws, out = _nan((B * nch, Cc), x.device), _nan((Cc,), x.device)
    lib.call("vae_gn_track_partial", ops._p(x), ops._b16(x), ops._p(st.scale), ops._p(st.shift), B, H * W, Cc, nch, ops._p(ws), ops._stream())
    assert not bool(ws.isnan().any()), "a chunk left its tracker partial unwritten"
    lib.call("vae_track_final", ops._p(ws), B * nch, Cc, 1.0 / float(B * H * W), ops._p(out), ops._stream())
    return out


def k_bwd(x, g, st, gamma, beta, silu, add, want32=True, want16=False):
    """the three launches of ops.gn_bwd -> dx (fp32 or None), dx16 (bf16 or None), dgamma, dbeta; add is stored like x"""
    from vaehip import ops
    from vaehip.lib import lib
    B, H, W, Cc = x.shape
    assert add is None or add.dtype == x.dtype
    nch = ops._gn_nchunk(B, H * W, Cc)
    ws, coef = _nan((B, nch, Cc, 2), x.device), _nan((B, nr.G, 2), x.device)
    dgamma, dbeta = _nan((Cc,), x.device), _nan((Cc,), x.device)
    dx = _nan(x.shape, x.device) if want32 else None
    dx16 = _nan(x.shape, x.device, torch.bfloat16) if want16 else None
    s = ops._stream()
    lib.call("vae_gn_bwd_partial", ops._p(x), ops._b16(x), ops._p(g), ops._p(st.mean), ops._p(st.rstd), ops._p(gamma), ops._p(beta),
             B, H * W, Cc, nr.G, nch, int(silu), ops._b16(g), ops._p(ws), s)
    assert not bool(ws.isnan().any()), "a chunk left its backward partial unwritten"
    lib.call("vae_gn_bwd_final", ops._p(ws), ops._p(st.rstd), ops._p(gamma), B, H * W, Cc, nr.G, nch, ops._p(dgamma), ops._p(dbeta),
             ops._p(coef), s)
    lib.call("vae_gn_bwd_apply", ops._p(x), ops._b16(x), ops._p(g), ops._p(st.mean), ops._p(st.rstd), ops._p(gamma), ops._p(beta),
             ops._p(coef), ops._p(add), B, H * W, Cc, nr.G, int(silu), ops._b16(g), ops._p(dx), ops._p(dx16), s)
    return dx, dx16, dgamma, dbeta


def k_track_final(ws, count, out):
    from vaehip import ops
    from vaehip.lib import lib
    lib.call("vae_track_final", ops._p(ws), ws.shape[0], ws.shape[1], 1.0 / float(count), ops._p(out), ops._stream())
    return out


def k_dead_scan(flat, segs, thr, athr=None, use_fixed=0):
    """vae_dead_scan (athr None) -> counts, abssum; vae_dead_scan_adaptive -> counts; chunk partials pre-filled with garbage"""
    from vaehip import ops
    from vaehip.lib import lib
    dev = flat.device
    seg = torch.tensor([[b, e] for b, e in segs], dtype=torch.int64).view(-1).to(dev)
    c0 = nr.dead_chunk0(segs)
    chunk0, nchunk, n = torch.from_numpy(c0).to(dev), int(c0[-1]), len(segs)
    counts = torch.full((n,), -7, dtype=torch.int64, device=dev)
    pcnt = torch.full((nchunk,), -1, dtype=torch.int64, device=dev)
    if athr is None:
        abssum, psum = _nan((n,), dev, torch.float64), _nan((nchunk,), dev, torch.float64)
        lib.call("vae_dead_scan", ops._p(flat), ops._p(seg), ops._p(chunk0), n, nchunk, float(np.float32(thr)), ops._p(pcnt), ops._p(psum),
                 ops._p(counts), ops._p(abssum), ops._stream())
        return counts.cpu().tolist(), abssum.cpu().tolist()
    at = torch.tensor([float(np.float32(a)) for a in athr], dtype=torch.float32, device=dev)
    lib.call("vae_dead_scan_adaptive", ops._p(flat), ops._p(seg), ops._p(chunk0), n, nchunk, float(np.float32(thr)), int(use_fixed),
             ops._p(at), ops._p(pcnt), ops._p(counts), ops._stream())
    return counts.cpu().tolist(), None


# ---------------------------------------------------------------------------------------------------- GroupNorm cases
def _same(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                                                           b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32)))


def _track_err(tr, ref) -> float:
    """largest relative error of a channel; a channel whose reference is zero (gamma == 0, beta == 0) has to be zero"""
    tr, ref = tr.detach().double().cpu(), ref.detach().double().cpu()
    z = ref == 0
    if bool(z.any()) and not bool((tr[z] == 0).all()):
        return math.inf
    return float(((tr[~z] - ref[~z]).abs() / ref[~z]).max()) if bool((~z).any()) else 0.0


def _abs_err(a, b) -> float:
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _forward(key, c, st, x, silu, ref, t32, per_channel=False):
    """statistics, both apply passes (fp32 and bf16 output), tracker; -> the kernel's y"""
    y32, act32, track32 = t32[:3]
    ratio = c.info.get("ratio")
    nr.check(K + "mean", key, nr.rel(st.mean, ref.mean), 1e-6)
    nr.check(K + "rstd", key, nr.elem_rel(st.rstd, ref.rstd), 2e-5)
    y = k_apply(x, st, XF_AFFINE)
    assert bool(y.isfinite().all())
    if ratio is not None:   # fp32 x itself carries ratio * 6e-8: the bar of test_groupnorm_statistics_with_large_mean, absolute
        lim = 3e-4 * max(1.0, ratio / 30)
        nr.check(K + "apply_abs", key, _abs_err(y, ref.y), lim, _abs_err(y32, ref.y))
    else:
        cpu = nr.rel(y32, ref.y)
        nr.check(K + "apply", key, nr.rel(y, ref.y), nr.bar(4, cpu, 1e-5), cpu)
    assert _same(k_apply16(x, st, XF_AFFINE), y.bfloat16())
    if silu:
        act = k_apply(x, st, XF_AFFINE_SILU)
        assert bool(act.isfinite().all())
        if ratio is not None:   # |silu'| <= 1.1
            nr.check(K + "apply_silu_abs", key, _abs_err(act, ref.act), 1.1 * lim, _abs_err(act32, ref.act))
        else:
            cpu = nr.rel(act32, ref.act)
            nr.check(K + "apply_silu", key, nr.rel(act, ref.act), nr.bar(4, cpu, 1e-5), cpu)
        if per_channel:   # every channel on its own scale: the planted channels are not hidden behind the largest
            cpu = nr.scaled_rel(act32, ref.act, nr.chan_max(ref.act))
            nr.check(K + "apply_silu_per_channel", key, nr.scaled_rel(act, ref.act, nr.chan_max(ref.act)), nr.bar(4, cpu, 1e-5), cpu)
        assert _same(k_apply16(x, st, XF_AFFINE_SILU), act.bfloat16())
    tr = k_track(x, st)
    live = torch.ones(ref.track.shape, dtype=torch.bool)
    const = c.info.get("const")
    if const:   # a channel that is constant in every image: its |y| is |beta + rounding of shift|, and |beta| may be tiny -- the
        # format bound of the module doc string instead of a ratio (absolute, one ulp of the largest mean * scale)
        B, cpg = x.shape[0], x.shape[-1] // nr.G
        for grp in range(nr.G):
            if all((b, grp) in const for b in range(B)):
                live[grp * cpg:(grp + 1) * cpg] = False
        if not bool(live.all()):
            ulp = float(np.spacing(np.float32(float((st.scale.abs().cpu() * nr.CONST_VALUE).max()))))
            nr.check(K + "track_constant_channels_abs", key, _abs_err(tr.cpu()[~live], ref.track[~live]), ulp, strict=False)
    cpu = _track_err(track32[live], ref.track[live])
    nr.check(K + "track", key, _track_err(tr.cpu()[live], ref.track[live]), nr.bar(4, cpu, 1e-5), cpu)
    assert _same(k_track(x, st), tr), "gn_track is not repeatable bit for bit"
    return y


def _backward(key, c, st, x, g, add, gamma, beta, silu, bref, t32, per_channel=False):
    dx32, dgamma32, dbeta32 = t32[3:]
    dx, _, dgamma, dbeta = k_bwd(x, g, st, gamma, beta, silu, add)
    for t in (dx, dgamma, dbeta):
        assert bool(t.isfinite().all())
    for name, got, want, torch32 in (("dx", dx, bref.dx, dx32), ("dgamma", dgamma, bref.dgamma, dgamma32), ("dbeta", dbeta, bref.dbeta, dbeta32)):
        cpu = nr.rel(torch32, want)
        nr.check(K + name, key, nr.rel(got, want), nr.bar(4, cpu, 2e-5), cpu)
    if per_channel:   # each channel's sums on the scale of what they add up: the planted channels are not hidden behind the plain ones
        for name, got, want, torch32, den in (("dgamma", dgamma, bref.dgamma, dgamma32, bref.dgamma_abs),
                                              ("dbeta", dbeta, bref.dbeta, dbeta32, bref.dbeta_abs)):
            cpu = nr.scaled_rel(torch32, want, den)
            nr.check(K + name + "_per_channel", key, nr.scaled_rel(got, want, den), nr.bar(4, cpu, 2e-5), cpu)
    again = k_bwd(x, g, st, gamma, beta, silu, add)
    assert _same(again[0], dx) and _same(again[2], dgamma) and _same(again[3], dbeta), "gn_bwd is not repeatable bit for bit"
    return dx, dgamma, dbeta


def _run(cuda, name, values, silu, backward=True, use_add=True):
    c = nr.build_case(name, values)
    key = f"{name},{values},silu={int(silu)}"
    x, gamma, beta = c.x.to(cuda), c.gamma.to(cuda), c.beta.to(cuda)
    add = c.add if (backward and use_add) else None
    ref = nr.gn_ref64(c.x, c.gamma, c.beta, silu=silu)
    t32 = nr.gn_torch(c.x, c.gamma, c.beta, silu, c.g if backward else None, add)
    st = k_stats(x, gamma, beta)
    assert all(_same(a, b) for a, b in zip(k_stats(x, gamma, beta), st)), "gn_stats is not repeatable bit for bit"
    y = _forward(key, c, st, x, silu, ref, t32, per_channel=values == "silu_range")
    out = None
    if backward:
        bref = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, silu, add, ref=ref)
        out = _backward(key, c, st, x, c.g.to(cuda), None if add is None else add.to(cuda), gamma, beta, silu, bref, t32,
                        per_channel=values == "silu_range")
    return c, st, y, ref, out


PLAIN = [("one_pixel", True), ("seven_pixels", False), ("tail_c256", True), ("tail_c512", False), ("one_chunk", True),
         ("one_chunk_plus1", False), ("ragged_two", True), ("last_empty", True), ("many_chunks", False), ("b65", True), ("capped", True)]


@pytest.mark.parametrize("name,silu", PLAIN)
def test_plain_values_at_every_shape(cuda, name, silu):
    _run(cuda, name, "plain", silu)


def test_grid_stride_trips_of_the_apply_passes(cuda):
    """more quads (and more octets) than the capped grid has threads: forward apply passes and the tracker only"""
    _run(cuda, "grid_stride", "plain", True, backward=False)


def test_direct_calls_are_what_ops_runs(cuda):
    """the poisoned ABI calls of this file and vaehip.ops launch the same kernels on the same plans: identical bits"""
    from vaehip import ops
    c = nr.plain_case("last_empty")
    x, g, add, gamma, beta = (t.to(cuda) for t in (c.x, c.g, c.add, c.gamma, c.beta))
    st, st_ops = k_stats(x, gamma, beta), ops.gn_stats(x, gamma, beta)
    assert all(_same(a, b) for a, b in zip(st, st_ops))
    assert _same(k_apply(x, st, XF_AFFINE_SILU), ops.gn_apply(x, st, ops.XF_AFFINE_SILU)) and ops.XF_AFFINE == XF_AFFINE
    assert _same(k_apply16(x, st, XF_AFFINE_SILU), ops.gn_apply_bf16(x, st, ops.XF_AFFINE_SILU))
    assert _same(k_track(x, st), ops.gn_track(x, st))
    dga, dbe = _nan((x.shape[-1],), cuda), _nan((x.shape[-1],), cuda)
    dx = ops.gn_bwd(x, g, st, gamma, beta, True, add, dga, dbe)
    mine = k_bwd(x, g, st, gamma, beta, True, add)
    assert _same(mine[0], dx) and _same(mine[2], dga) and _same(mine[3], dbe)


@pytest.mark.parametrize("name,ratio,silu", [("ragged_two", 30.0, True), ("tail_c256", 30.0, False), ("last_empty", 30.0, True),
                                             ("ragged_two", 1000.0, False), ("tail_c256", 1000.0, True), ("last_empty", 1000.0, False)])
def test_large_mean_forward_and_backward(cuda, name, ratio, silu):
    _run(cuda, name, f"large_mean_{ratio:g}", silu)


@pytest.mark.parametrize("name", ["seven_pixels", "one_chunk_plus1", "tail_c256", "last_empty"])
def test_constant_group_and_constant_image(cuda, name):
    c, st, y, ref, (dx, dgamma, dbeta) = _run(cuda, name, "constant", True)
    B, H, W, Cc = c.x.shape
    cpg = Cc // nr.G
    mean, rstd, scale = st.mean.cpu(), st.rstd.cpu(), st.scale.cpu()
    for b, grp in c.info["const"]:
        sl = slice(grp * cpg, (grp + 1) * cpg)
        assert float(mean[b, grp]) == float(np.float32(nr.CONST_VALUE)), "the mean of a constant group is its value"
        assert float(rstd[b, grp]) == float(np.float32(1.0 / math.sqrt(float(np.float32(nr.EPS))))), "var == 0: rstd = 1 / sqrt(eps)"
        # y = x * scale + shift, shift = beta - mean * scale rounded to fp32 at the size of mean * scale: beta within one ulp of that
        ulp = float(np.spacing(np.float32(float((scale[b, sl].abs() * nr.CONST_VALUE).max()))))
        err = float((y[b, :, :, sl].cpu().double() - c.beta.double()[sl]).abs().max())
        nr.check(K + "constant_is_beta_abs", f"{name},b={b},g={grp}", err, ulp, strict=False)
    if B > 1:   # the image that is constant throughout, alone: its tracker vector is |beta|, to the same format bound
        x0, gamma, beta = c.x[:1].to(cuda), c.gamma.to(cuda), c.beta.to(cuda)
        st0 = k_stats(x0, gamma, beta)
        ulp = float(np.spacing(np.float32(float((st0.scale.abs() * nr.CONST_VALUE).max()))))
        err = float((k_track(x0, st0).cpu().double() - c.beta.double().abs()).abs().max())
        nr.check(K + "constant_track_is_abs_beta_abs", name, err, ulp, strict=False)


@pytest.mark.parametrize("name", ["ragged_two", "tail_c256", "last_empty"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_outlier_as_pivot_and_as_last_value(cuda, name, where):
    _run(cuda, name, f"outlier_{where}", False)


@pytest.mark.parametrize("name", ["seven_pixels", "one_chunk", "tail_c256", "last_empty"])
def test_silu_where_exp_overflows_and_gamma_zero_or_negative(cuda, name):
    c, st, y, ref, _ = _run(cuda, name, "silu_range", True)
    zero = c.info["kind"] == 2
    # gamma == 0: scale is 0, shift is beta, the pre-activation is beta bit for bit
    assert bool((y.cpu()[..., zero] == c.beta[zero]).all())


@pytest.mark.parametrize("name", ["tail_c512", "ragged_two", "tail_c256", "b65"])
def test_one_hot_gradient_reaches_its_group_and_no_other(cuda, name):
    c, st, y, ref, (dx, dgamma, dbeta) = _run(cuda, name, "one_hot", False, use_add=False)
    B, H, W, Cc = c.x.shape
    cpg = Cc // nr.G
    dxc = dx.cpu()
    for b, pix, ch in c.info["hot"]:
        mask = torch.zeros(Cc, dtype=torch.bool)
        mask[(ch // cpg) * cpg:(ch // cpg + 1) * cpg] = True
        assert bool((dxc[b][..., ~mask] == 0).all()), "a group without gradient received one"
        assert bool((dxc[b][..., mask] != 0).all()), "a pixel of the group was left out"


@pytest.mark.parametrize("name,values,silu", [("one_pixel", "plain", True), ("tail_c256", "plain", False), ("tail_c512", "plain", True),
                                              ("last_empty", "plain", True), ("tail_c256", "silu_range", True),
                                              ("last_empty", "silu_range", True)])
def test_bf16_storage(cuda, name, values, silu):
    """x, g and add stored as bf16, bf16 outputs wanted: against float64 on the rounded values, and bit for bit against the
    fp32-storage run on x.float(), g.float(), add.float()"""
    c = nr.build_case(name, values)
    key = f"{name},{values},silu={int(silu)},bf16"
    c = c._replace(x=nr.r16(c.x), g=nr.r16(c.g), add=nr.r16(c.add))
    gamma, beta = c.gamma.to(cuda), c.beta.to(cuda)
    xf, gf, af = c.x.to(cuda), c.g.to(cuda), c.add.to(cuda)
    xh, gh, ah = xf.bfloat16(), gf.bfloat16(), af.bfloat16()
    assert torch.equal(xh.float(), xf) and torch.equal(gh.float(), gf) and torch.equal(ah.float(), af)
    ref = nr.gn_ref64(c.x, c.gamma, c.beta, silu=silu)
    bref = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, silu, c.add, ref=ref)
    t32 = nr.gn_torch(c.x, c.gamma, c.beta, silu, c.g, c.add)
    st = k_stats(xh, gamma, beta)
    assert all(_same(a, b) for a, b in zip(st, k_stats(xf, gamma, beta)))
    _forward(key, c, st, xh, silu, ref, t32, per_channel=values == "silu_range")
    for xfm in (XF_AFFINE, XF_AFFINE_SILU):
        assert _same(k_apply(xh, st, xfm), k_apply(xf, st, xfm)) and _same(k_apply16(xh, st, xfm), k_apply16(xf, st, xfm))
    assert _same(k_track(xh, st), k_track(xf, st))
    dx, dgamma, dbeta = _backward(key, c, st, xh, gh, ah, gamma, beta, silu, bref, t32, per_channel=values == "silu_range")
    fdx, _, fdg, fdb = k_bwd(xf, gf, st, gamma, beta, silu, af)
    assert _same(dx, fdx) and _same(dgamma, fdg) and _same(dbeta, fdb)
    both = k_bwd(xh, gh, st, gamma, beta, silu, ah, want32=True, want16=True)
    only = k_bwd(xh, gh, st, gamma, beta, silu, ah, want32=False, want16=True)
    assert _same(both[0], dx) and _same(both[1], dx.bfloat16()) and only[0] is None and _same(only[1], dx.bfloat16())
    assert _same(both[2], dgamma) and _same(only[2], dgamma) and _same(both[3], dbeta) and _same(only[3], dbeta)


# ---------------------------------------------------------------------------------------------------- vae_track_final
@pytest.mark.parametrize("Cc", nr.TRACK_C)
@pytest.mark.parametrize("rows", nr.TRACK_ROWS)
def test_track_final_rows_and_channel_tails(cuda, rows, Cc):
    """the kernel sums in float64 and rounds once; inv_count is itself the fp32 rounding of 1 / count: two roundings of half an
    ulp, 2^-23 relative against the exact quotient (derived, not measured).  Elements of `out` past C keep their NaN."""
    ws = nr.track_ws(rows, Cc)
    count = 7 * rows + 3   # 1 / count is not a power of two
    out = _nan(((Cc + 3) // 4 * 4 + 4,), cuda)
    k_track_final(ws.to(cuda), count, out)
    ref = nr.track_final_ref64(ws, count)
    got = out.cpu()
    assert bool(got[Cc:].isnan().all()), "vae_track_final wrote past its C channels"
    nr.check(K + "track_final", f"rows={rows},C={Cc}", nr.elem_rel(got[:Cc], ref), 2.0 ** -23, strict=False)
    again = _nan(out.shape, cuda)
    assert _same(k_track_final(ws.to(cuda), count, again)[:Cc], out[:Cc])


# ---------------------------------------------------------------------------------------------------- loud refusals
def test_unsupported_channel_counts_are_refused_loudly(cuda):
    """each returns an error with a message in vae_last_error() and launches nothing: the NaN-filled outputs stay untouched"""
    from vaehip import ops, VaeHipError
    from vaehip.lib import lib
    s = ops._stream()
    buf = [_nan((4096,), cuda) for _ in range(9)]
    p = [ops._p(b) for b in buf]
    b16 = _nan((4096,), cuda, torch.bfloat16)
    with pytest.raises(VaeHipError, match="channels per group unsupported"):   # 32 channels per group: GN_GPW * 32 > 64
        lib.call("vae_gn_bwd_final", p[0], p[1], p[2], 1, 4, 1024, 32, 1, p[3], p[4], p[5], s)
    with pytest.raises(VaeHipError, match="C=96 must be"):                     # 256 % (96 / 4) != 0
        lib.call("vae_gn_stats_partial", p[0], 0, 1, 4, 96, 32, 1, p[1], s)
    with pytest.raises(VaeHipError, match="C=96 must be"):
        lib.call("vae_gn_bwd_apply", p[0], 0, p[1], p[2], p[3], p[4], p[5], p[6], None, 1, 4, 96, 32, 0, 0, p[7], None, s)
    with pytest.raises(VaeHipError, match="gn_stats_final: C=132"):            # C = 132, G = 33
        lib.call("vae_gn_stats_final", p[0], 1, 4, 132, 33, 1, p[1], p[2], 1e-6, p[3], p[4], p[5], p[6], s)
    with pytest.raises(VaeHipError, match="gn_apply_bf16: bad args"):          # C % 8 != 0
        lib.call("vae_gn_apply_bf16", p[0], 0, p[1], p[2], 1, 4, 132, XF_AFFINE, ops._p(b16), s)
    torch.cuda.synchronize()
    assert all(bool(b.isnan().all()) for b in buf) and bool(b16.isnan().all())


# ---------------------------------------------------------------------------------------------------- dead-weight scan
def _check_scan(key, got_counts, got_sums, ref_counts, ref_sums, info):
    assert got_counts == ref_counts, (key, [(s, g, r) for s, (g, r) in enumerate(zip(got_counts, ref_counts)) if g != r])
    if got_sums is None:
        return
    worst = 0.0
    for s, (g, r) in enumerate(zip(got_sums, ref_sums)):
        if s == info["nan"]:
            assert math.isnan(g) and math.isnan(r), (key, s, g)      # the NaN poisons its own segment's sum ...
        elif s in info["inf"]:
            assert g == math.inf and r == math.inf, (key, s, g)
        else:
            assert math.isfinite(g), (key, s, g)                     # ... and no other; nor does a gap's
            worst = max(worst, abs(g - r) / r)                       # a float64 sum in another order
    nr.check(K + "dead_abssum", key, worst, 1e-12)


@pytest.mark.parametrize("gaps", ["zeros", "nan"])
def test_dead_scan_segments_gaps_and_strictness(cuda, gaps):
    """16 segments (every length of DEAD_LENGTHS on a 16-byte boundary and one element past one) with gaps of zeros (counted by
    a bound that is off by one) or NaN (poisoning a sum that reaches into them); values exactly at, just below and at minus the
    threshold, -0.0, a denormal, +inf and one NaN at segment ends and on both sides of chunk boundaries"""
    flat, segs, info = nr.dead_layout(0.0 if gaps == "zeros" else float("nan"))
    dev = flat.to(cuda)
    assert dev.data_ptr() % 16 == 0
    ref_counts, ref_sums = nr.dead_counts(flat, segs, nr.DEAD_THR)
    counts, sums = k_dead_scan(dev, segs, nr.DEAD_THR)
    _check_scan(f"gaps={gaps}", counts, sums, ref_counts, ref_sums, info)
    assert ref_counts[info["nan"]] == nr.dead_counts(torch.nan_to_num(flat, nan=1.0), segs, nr.DEAD_THR)[0][info["nan"]]   # NaN: not counted
    counts2, sums2 = k_dead_scan(dev, segs, nr.DEAD_THR)            # fixed chunk order: the same bits again
    assert counts2 == counts and all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(sums2, sums))
    # adaptive thresholds per segment; segment 5's threshold lies exactly on one of its values, which the strict `<` leaves out
    athr = [0.005 * (1 + s / 16) for s in range(len(segs))]
    on = next(s for s, (b, e) in enumerate(segs) if e - b > 32768 and s not in info["inf"] and s != info["nan"])
    athr[on] = abs(float(flat[segs[on][0] + 7]))
    athr[1] = 0.5 * nr.DEAD_THR    # below the fixed threshold: decides with use_fixed too
    for use_fixed in (0, 1):
        ref, _ = nr.dead_counts(flat, segs, nr.DEAD_THR, athr, use_fixed=bool(use_fixed))
        got, _ = k_dead_scan(dev, segs, nr.DEAD_THR, athr, use_fixed)
        _check_scan(f"gaps={gaps},adaptive,use_fixed={use_fixed}", got, None, ref, None, info)
    loose = nr.dead_counts(flat, segs, nr.DEAD_THR, [float(np.nextafter(np.float32(a), np.float32(1))) for a in athr], use_fixed=False)[0]
    assert loose[on] == nr.dead_counts(flat, segs, nr.DEAD_THR, athr, use_fixed=False)[0][on] + 1   # a `<=` would count one more


@pytest.fixture(scope="module")
def planted_arena_model(cuda):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), nr.TRACKER_SEED))
    w.to(cuda)
    nr.plant_tracker_params(dict(w.vae.named_parameters()))
    assert w.vae.arena.owns(w.vae)
    return w


@pytest.mark.parametrize("mode", ["threshold", "percent_of_mean", "both"])
def test_tracker_on_the_arena_matches_its_own_formulas(cuda, planted_arena_model, mode):
    """DeadNeuronTracker.track_dead_neurons (one scan over the arena) against the same tracker's per-parameter formulas on CPU
    copies; the seed and the plants are the ones tests/test_norm_edges_host.py vetted for threshold ambiguity"""
    from tracking.deadneuron import DeadNeuronTracker
    w = planted_arena_model
    t = DeadNeuronTracker(TARGET, [], threshold=nr.TRACKER_THR, mean_percentage=nr.TRACKER_MEAN_PCT, dead_type=mode)
    t.track_dead_neurons(w, 3)
    got = {k: v[0][1] for k, v in t.percent_history.items()}
    params = dict(w.vae.named_parameters())
    assert len(got) == 248 and {nr.PLANT_ZERO_BIAS, nr.PLANT_TINY_BIAS, nr.PLANT_ONE_VALUE, nr.PLANT_LARGE_CONV, nr.PLANT_BETWEEN} <= set(got)
    for name, pct in got.items():
        want = t.get_percentage(params[name].detach().cpu().contiguous())
        assert pct == pytest.approx(want, rel=1e-9, abs=0.0), (mode, name, pct, want)
    assert got[nr.PLANT_ZERO_BIAS] == 100.0
    assert got[nr.PLANT_TINY_BIAS] == 100.0
    n_one = params[nr.PLANT_ONE_VALUE].numel()
    assert got[nr.PLANT_ONE_VALUE] == pytest.approx((n_one - 1) / n_one * 100.0, rel=1e-12)
    assert got[nr.PLANT_LARGE_CONV] >= 200 / params[nr.PLANT_LARGE_CONV].numel() * 100.0
    assert got[nr.PLANT_BETWEEN] >= 50.0
