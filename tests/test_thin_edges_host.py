"""tests/thin_refs.py without a GPU: every case's argument block selects the kernel instantiation its label names and passes the
storage-flag query (through the library's own selection, which needs no device), no instantiation of the six kernels is left
without a case, the hand-written geometry equals torch's conv2d and autograd in float64, the cases have the tile / split / pass
structure they are in the table for, and the criteria accept a correct implementation with another summation order (torch
float32 on the CPU, r16 at the kernel's rounding points) and reject each single mistake on the case built for it."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import bf16_refs as br
import thin_refs as T
from vaehip import ops
from vaehip.lib import lib

ALL_ROWS = T.ROWS_CASES + (T.THIN_LARGE,)


_passes, rows_figures, wg_figures = T.passes, T.rows_figures, T.wg_figures


def _track32(c, stored):
    """per-tile sums of |stored| in float32, rows past M left out"""
    M, N = stored.shape
    nt = (M + T.TP - 1) // T.TP
    return torch.cat([stored.float().abs(), torch.zeros(nt * T.TP - M, N)]).reshape(nt, T.TP, N).sum(dim=1)


# ---------------------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("c", ALL_ROWS, ids=lambda c: c.id)
def test_rows_case_selects_its_kernel(c):
    a = T.rows_block(c, ops)
    with ops.option("no_thin_mfma", int(c.no_thin)):
        assert T.kernel_name(lib, "vae_igemm_kernel_name", a) == c.kernel
        assert (c.out16 or c.a16) == bool(a.out_bf16 or a.a_bf16)
        assert lib.query("vae_conv_io16_ok", C.byref(a)) == 1
    if T.matrix_pipe(c.kernel):   # the option sends the same block to the VALU kernel of the pair
        with ops.option("no_thin_mfma", 1):
            other = T.kernel_name(lib, "vae_igemm_kernel_name", a)
            assert other == c.kernel.replace("conv_thinn_bf16", "conv_smalln").replace("conv_thin_bf16", "conv_smallk")
            assert lib.query("vae_conv_io16_ok", C.byref(a)) == 1


@pytest.mark.parametrize("c", T.WG_CASES, ids=lambda c: c.id)
def test_wgrad_case_selects_its_kernel(c):
    a = T.wg_block(c, ops)
    assert a.nsplit == c.ns and a.M == c.Co and a.N == c.Ci
    with ops.option("no_thin_mfma", int(c.no_thin)):
        assert T.kernel_name(lib, "vae_wgrad_kernel_name", a) == c.kernel
        assert lib.query("vae_wgrad_io16_ok", C.byref(a)) == 1
    if T.matrix_pipe(c.kernel):
        with ops.option("no_thin_mfma", 1):
            assert T.kernel_name(lib, "vae_wgrad_kernel_name", a) == c.kernel.replace("wgrad_thin_bf16", "wgrad_smallk")
            assert lib.query("vae_wgrad_io16_ok", C.byref(a)) == 1


def test_the_planned_split_count_is_the_tile_count():
    """vae_wgrad_plan gives these kernels min(1024, tiles): nsplit 12 on map A is the planned value, and no smaller test shape
    ever gets more than one tile per split from the plan"""
    for c in T.WG_CASES:
        a = T.wg_block(c, ops)
        ns, fus = C.c_int32(0), C.c_int32(0)
        with ops.option("no_thin_mfma", int(c.no_thin)):
            lib.call("vae_wgrad_plan", C.byref(a), C.byref(ns), C.byref(fus))
        assert ns.value == T.wg_tiles(c) and fus.value == 1, c.id


def test_every_instantiation_has_a_case():
    named = {c.kernel for c in ALL_ROWS} | {c.kernel for c in T.WG_CASES}
    assert named == set(T.INSTANTIATIONS) and len(T.INSTANTIATIONS) == 16
    ids = [c.id for c in ALL_ROWS] + [c.id for c in T.WG_CASES]
    assert len(ids) == len(set(ids))
    # the arms the suite is for, each by the case that takes it
    wg = {(c.kernel, c.ns) for c in T.WG_CASES if c.shape == T.MAP_A}
    for k in ("wgrad_thin_bf16_kernel<false,0>", "wgrad_thin_bf16_kernel<false,1>", "wgrad_thin_bf16_kernel<false,2>",
              "wgrad_thin_bf16_kernel<true,0>", "wgrad_smallk_kernel<true,0>", "wgrad_smallk_kernel<false,2>"):
        assert {(k, 1), (k, 5), (k, 12)} <= wg, k
    has = lambda cases, **kw: any(all(getattr(c, f) == v for f, v in kw.items()) for c in cases)   # noqa: E731
    for K in (32, 96, 128):
        assert has(T.SMALLN_CASES, Ci=K)
    for K in (32, 64, 128):
        assert has(T.THINN_CASES, Ci=K)
    for N in (1, 2, 3, 4):
        assert has(T.SMALLN_CASES, Co=N)
    for N in (1, 3, 4):
        assert has(T.THINN_CASES, Co=N)
    for xf in (0, 1, 2):
        assert has(T.SMALLN_CASES, xf=xf) and has(T.THINN_CASES, xf=xf)
    assert has(T.SMALLN_CASES, bias=False) and has(T.SMALLN_CASES, Ci=32, Cs=64) and has(T.THINN_CASES, Ci=32, Cs=64)
    assert has(T.SMALLN_CASES, a16=True, Ci=96) and has(T.SMALLN_CASES, a16=True, no_thin=True)
    for K in (1, 2, 3, 4):
        assert has(T.SMALLK_CASES, Ci=K, form="fwd") and has(T.THIN_CASES, Ci=K, form="fwd")
    for N in (96, 160):
        assert has(T.SMALLK_CASES, Co=N)
    assert has(T.THIN_CASES, Co=256) and has(T.THIN_CASES, track=False) and has(T.THIN_CASES, track=True)
    for kind in ("c3", "c3s2", "c3up", "c1"):
        assert has(T.SMALLK_CASES, kind=kind, form="fwd") and has(T.WG_CASES, kind=kind, side=1)
    assert has(T.SMALLK_CASES, form="dgrad", kind="c3") and has(T.SMALLK_CASES, form="dgrad", kind="c3s2") and has(T.THIN_CASES, form="dgrad")
    assert has(T.SMALLK_CASES, out16=True, bf16=True)
    assert has(T.WG_CASES, side=1, Co=160) and has(T.WG_CASES, side=1, Co=256) and has(T.WG_CASES, side=2, Ci=256)
    assert has(T.WG_CASES, side=1, no_thin=True, wide16=True) and has(T.WG_CASES, side=2, no_thin=True, wide16=True)
    assert has(T.WG_CASES, side=1, bias=False) and has(T.WG_CASES, side=1, Ci=1, Cs=1) and has(T.WG_CASES, side=2, Co=1) and has(T.WG_CASES, side=2, Co=4)


# ---------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("kind,H,W", [("c3", 5, 7), ("c3s2", 10, 14), ("c3s2", 9, 11), ("c3up", 5, 6), ("c1", 5, 7)])
def test_hand_written_geometry_equals_torch(kind, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    B, Ci, Co = 2, 3, 5
    taps = T.taps_of(kind)
    x = torch.randn(B, H, W, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Co, taps, Ci, generator=g, dtype=torch.float64)
    Ho, Wo = T.out_hw(kind, H, W)
    assert (Ho, Wo) == ops.out_hw(kind, H, W)
    dy = torch.randn(B, Ho, Wo, Co, generator=g, dtype=torch.float64)
    # torch, spelled out here: stride 2 pads (0, 1, 0, 1), an upsampler interpolates nearest first
    xn = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wn = T._oihw(w, kind).clone().requires_grad_(True)
    if kind == "c3s2":
        y = F.conv2d(F.pad(xn, (0, 1, 0, 1)), wn, None, 2, 0)
    elif kind == "c3up":
        y = F.conv2d(F.interpolate(xn, scale_factor=2.0, mode="nearest"), wn, None, 1, 1)
    else:
        y = F.conv2d(xn, wn, None, 1, 0 if kind == "c1" else 1)
    gx, gw = torch.autograd.grad(y, (xn, wn), dy.permute(0, 3, 1, 2))
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())   # noqa: E731
    assert close(T.fwd_by_hand(x, w, kind), y.detach().permute(0, 2, 3, 1))
    assert close(br.conv_nchw(x.permute(0, 3, 1, 2), T._oihw(w, kind), kind), y.detach())
    assert close(T.wgrad_by_hand(dy, x, kind), gw.permute(0, 2, 3, 1).reshape(Co, taps, Ci))
    assert close(T.dgrad_by_hand(dy, w, kind, H, W), gx.permute(0, 2, 3, 1))


@pytest.mark.parametrize("cid", ["smallk-c3s2", "smallk-c3up", "smallk-c1", "smallk-c3-ragged", "smallk-dgrad", "smallk-c3s2-dgrad"])
def test_rows_reference_equals_the_hand_written_form(cid):
    c, o = T.rows_case(cid), T.rows_operands(T.rows_case(cid))
    B, H, W = c.shape
    if c.form == "fwd":
        want = T.fwd_by_hand(o.src.double()[..., :c.Ci], o.w.double(), c.kind)
    else:
        want = T.dgrad_by_hand(o.src.double(), o.w.double(), c.kind, H, W)
    want = want.reshape(-1, want.shape[-1]) + (o.bias.double() if o.bias is not None else 0.0)
    assert float((T.rows_ref(c) - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("cid", ["smallk-c3s2-k1-3of4-m128-ns1", "smallk-c3up-k1-4of4-m128-ns2", "smallk-c1-k1-4of4-m128-ns1",
                                 "smallk-mapB-k2-m3-n128-xf2-ns2"])
def test_wgrad_reference_equals_the_hand_written_form(cid):
    c = T.wg_case(cid)
    o = T.wg_operands(c)
    a = T._transform(o.x.double(), o.scale, o.shift, c.xf)[..., :c.Ci]
    want = T.wgrad_by_hand(o.dy.double(), a, c.kind)
    ref = T.wg_ref(c)
    assert float((ref.gw - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert torch.equal(ref.gb, o.dy.double().sum(dim=(0, 1, 2)))


# ---------------------------------------------------------------------------------------------------- case properties
def _straddles(tile, hw, npix):
    lo, hi = tile * T.TP, min(npix, tile * T.TP + T.TP) - 1
    return lo // hw != hi // hw


def test_weight_gradient_maps_have_their_tile_structure():
    a = {c.ns: c for c in T.WG_CASES if c.id.startswith("thin-k2-m3-n128-xf2")}
    assert set(a) == {1, 5, 12}
    B, H, W = T.MAP_A
    assert T.wg_pixels(a[1]) == 1536 and T.wg_tiles(a[1]) == 12 and (H * W) // T.TP == 4 and (H * W) % T.TP == 0
    assert T.wg_ranges(a[1]) == [(0, 12)]                                     # per = 12: across both image boundaries (tiles 4, 8)
    assert T.wg_ranges(a[5]) == [(0, 3), (3, 6), (6, 9), (9, 12), (12, 12)]   # per = 3, the last split empty
    assert [r for r in T.wg_ranges(a[5]) if r[0] < 4 < r[1] or r[0] < 8 < r[1]] == [(3, 6), (6, 9)]   # ranges that enter the next image
    assert T.wg_ranges(a[12]) == [(t, t + 1) for t in range(12)]
    b = [c for c in T.WG_CASES if c.shape == T.MAP_B]
    assert {c.ns for c in b} == {1, 2, 3} and all(not T.matrix_pipe(c.kernel) for c in b)
    for c in b:
        assert T.wg_pixels(c) == 300 and T.wg_tiles(c) == 3 and 300 - 2 * T.TP == 44
        assert _straddles(0, 100, 300) and _straddles(1, 100, 300) and not _straddles(2, 100, 300)   # xb changes inside tiles 0 and 1
    assert T.wg_ranges(T.wg_case("smallk-mapB-k1-3of4-m160-ns2")) == [(0, 2), (2, 3)]
    assert T.wg_ranges(T.wg_case("smallk-c3up-k1-4of4-m128-ns2")) == [(0, 1), (1, 1)]
    assert T.wg_pixels(T.wg_case("smallk-c3s2-k1-3of4-m128-ns1")) == 35 and T.wg_pixels(T.wg_case("smallk-c3up-k1-4of4-m128-ns2")) == 120
    for c in T.WG_CASES:
        assert T.wg_pixels(c) <= T.MAX_WGRAD_PIXELS, c.id
        if T.matrix_pipe(c.kernel):   # whole tiles, each inside one image (wgrad_thin_bf16_eligible)
            assert (c.shape[1] * c.shape[2]) % T.TP == 0 and (c.Co if c.side == 1 else c.Ci) % 128 == 0


def test_rows_maps_have_their_tile_structure():
    M = T.rows_dims(T.rows_case("smallk-c3-ragged"))[0]
    assert M == 300 and M % T.TP == 44 and _straddles(0, 100, 300)
    assert T.rows_dims(T.rows_case("smallk-out16"))[0] % T.TP != 0            # why the thin kernel does not take it
    M = T.rows_dims(T.rows_case("thin-straddle"))[0]
    assert M == 384 and M % T.TP == 0 and all(_straddles(t, 96, M) for t in range(3))
    for c in T.THIN_CASES + (T.THIN_LARGE,):
        assert T.rows_dims(c)[0] % T.TP == 0 and T.rows_dims(c)[1] % 128 == 0, c.id
    # the large case: launch_conv_thin_bf16 takes min(8, tiles / 1024) tiles per workgroup
    M = T.rows_dims(T.THIN_LARGE)[0]
    tiles = M // T.TP
    per = max(1, min(8, tiles // 1024))
    wgs = (tiles + per - 1) // per
    assert (M, tiles, per, wgs) == (263040, 2055, 2, 1028) and min(tiles, (wgs - 1) * per + per) - (wgs - 1) * per == 1
    assert all(max(1, min(8, (T.rows_dims(c)[0] // T.TP) // 1024)) == 1 for c in T.THIN_CASES)
    assert M * 128 * 2 == 67338240                                            # the output, bytes
    # narrow output: 2 x 2 tiles per image; chunks of 32 channels (VALU), passes of 1024 (pixel, octet) chunks over the 204 halo pixels
    B, H, W = T.MAP_N
    assert (H // T.SN_TH, W // T.SN_TW, B) == (2, 2, 2) and H % T.SN_TH == 0 and W % T.SN_TW == 0
    assert {c.Ci // 32 for c in T.SMALLN_CASES} == {1, 3, 4}
    halo = (T.SN_TH + 2) * (T.SN_TW + 2)
    assert {c.Ci: -(-halo * (c.Ci // 8) // 1024) for c in T.THINN_CASES} == {32: 1, 64: 2, 128: 4}
    assert all(256 % (c.Ci // 8) == 0 for c in T.THINN_CASES) and 256 % (96 // 8) != 0


def test_unused_channels_are_far_and_shifts_are_not_zero():
    for c in ALL_ROWS:
        o = T.rows_operands(c)
        if c.form == "fwd" and c.Cs > c.Ci:
            assert bool((o.src[..., c.Ci:].float() > 0.99 * T.FAR).all()), c.id
        if c.xf != T.XF_NONE:
            assert float(o.shift.abs().min()) > 0 and o.scale.shape == (c.shape[0], c.Cs)
    for c in T.WG_CASES:
        o = T.wg_operands(c)
        if c.Cs > c.Ci:
            assert bool((o.x[..., c.Ci:].float() > 0.99 * T.FAR).all()), c.id
        assert o.x.dtype == (torch.bfloat16 if c.wide16 and c.side == 2 else torch.float32)
        assert o.dy.dtype == (torch.bfloat16 if c.wide16 and c.side == 1 else torch.float32)


# ---------------------------------------------------------------------------------------------------- the criteria accept ...
@pytest.mark.parametrize("c", ALL_ROWS, ids=lambda c: c.id)
def test_rows_criteria_accept_float32_on_the_cpu(c):
    v = T.rows_ref(c)
    v32 = T.rows_value(c, acc=torch.float32, xfdt=torch.float32)
    out = T.rows_store(c, v32)
    figs = rows_figures(c, out, _track32(c, out) if c.track else None, v=v)
    assert _passes(figs), (c.id, figs)
    bar, fp = T.rows_bar(c)
    assert (fp is not None) == (T.matrix_pipe(c.kernel) and c.xf != T.XF_NONE) and bar >= br.BAR_DIRECT
    assert fp is None or fp < 1e-2, (c.id, fp)   # (a bar of 4 x that still separates every mistake below)


@pytest.mark.parametrize("c", T.WG_CASES, ids=lambda c: c.id)
def test_wgrad_criteria_accept_float32_on_the_cpu(c):
    o = T.wg_operands(c)
    got = T.wg_value(c, acc=torch.float32, xfdt=torch.float32)
    db = o.dy.float().sum(dim=(0, 1, 2)) if c.bias else None
    figs = wg_figures(c, got.gw.float(), db)
    assert _passes(figs), (c.id, figs)
    bar, fp = T.wg_bar(c)
    assert (fp is not None) == (T.matrix_pipe(c.kernel) and c.xf != T.XF_NONE)
    assert bar >= (br.BAR_WGRAD_GN if c.xf else br.BAR_WGRAD) and (fp is None or fp < 1e-3), (c.id, fp)


# ---------------------------------------------------------------------------------------------------- ... and reject
LONGEST = ("smallk-k1-3of4-m128-ns1", "thin-k1-3of4-m128-ns1", "smallk-k2-m3-n128-xf2-ns1", "thin-k2-m3-n128-xf2-ns1", "thin-k2-m3-n128-xf0-ns1")


@pytest.mark.parametrize("cid", LONGEST)
def test_a_dropped_pixel_is_seen_at_the_longest_contraction(cid):
    c = T.wg_case(cid)
    n = T.wg_pixels(c)
    assert n == max(T.wg_pixels(x) for x in T.WG_CASES)
    for k in (0, 5 * T.TP + 77, n - 1):
        pw = torch.ones(n)
        pw[k] = 0.0
        got = T.wg_value(c, acc=torch.float32, xfdt=torch.float32, pw=pw)
        figs = wg_figures(c, got.gw.float())
        assert figs["dW"][0] > 10 * figs["dW"][1], (cid, k, figs)   # by far more than the bar


@pytest.mark.parametrize("cid", ["smallk-k1-3of4-m128-ns5", "thin-k1-3of4-m128-ns5", "smallk-k2-m3-n128-xf1-ns5", "thin-k2-m3-n128-xf1-ns5",
                                 "smallk-mapB-k1-3of4-m160-ns2", "smallk-mapB-k2-m3-n128-xf2-ns2"])
@pytest.mark.parametrize("times", [0.0, 2.0])
def test_a_tile_dropped_from_a_split_or_counted_in_two_is_seen(cid, times):
    c = T.wg_case(cid)
    n = T.wg_pixels(c)
    t = T.wg_ranges(c)[1][0]   # the first tile of the second split: at the seam of two ranges
    pw = torch.ones(n)
    pw[t * T.TP:(t + 1) * T.TP] = times
    got = T.wg_value(c, acc=torch.float32, xfdt=torch.float32, pw=pw)
    figs = wg_figures(c, got.gw.float(), got.gb.float())
    assert figs["dW"][0] > 10 * figs["dW"][1] and figs["db"][0] > 10, (cid, figs)


@pytest.mark.parametrize("cid,where", [("smallk-k2-m3-n128-xf1-ns1", "image"), ("thin-k2-m3-n128-xf1-ns1", "image"),
                                       ("smallk-k2-m3-n128-xf2-ns1", "image"), ("thin-k2-m3-n128-xf2-ns1", "image"),
                                       ("smallk-k2-m3-n128-xf2-ns5", "image"), ("smallk-mapB-k2-m3-n128-xf2-ns1", "tile")])
def test_a_stale_scale_row_after_an_image_boundary_is_seen(cid, where):
    c = T.wg_case(cid)
    bidx = T.own_image(c)
    if where == "image":
        bidx[1] = 0                             # image 1 transformed with image 0's row: the reload skipped inside a range
    else:
        bidx.view(-1)[100:T.TP] = 0             # ... inside tile 0, whose rows 100..127 belong to image 1
    got = T.wg_value(c, acc=torch.float32, xfdt=torch.float32, bidx=bidx)
    figs = wg_figures(c, got.gw.float())
    assert figs["dW"][0] > 10 * figs["dW"][1], (cid, figs)


@pytest.mark.parametrize("cid", ["smallk-mapB-k1-3of4-m160-ns1", "thin-k1-4of4-m256-ns5", "smallk-k2-m4-n256-xf2-ns5", "thin-k2-m4-n256-xf1-ns1"])
def test_a_missing_last_channel_block_of_the_weight_gradient_is_seen(cid):
    c = T.wg_case(cid)
    got = T.wg_value(c, acc=torch.float32, xfdt=torch.float32)
    gw, gb = got.gw.float().clone(), got.gb.float().clone()
    if c.side == 1:
        gw[128 * ((c.Co - 1) // 128):] = 0.0
        gb[128 * ((c.Co - 1) // 128):] = 0.0
    else:
        gw[:, :, 128:] = 0.0
    figs = wg_figures(c, gw, gb)
    assert figs["dW"][0] > 10 * figs["dW"][1] and (c.side == 2 or figs["db"][0] > 10), (cid, figs)


@pytest.mark.parametrize("cid,mut", [
    ("smallk-c3-ragged", "tap"), ("smallk-dgrad", "tap"), ("smallk-c3s2", "tap"), ("thin-straddle", "tap"), ("thin-dgrad", "tap"),
    ("smalln-4-k128of128-n3-xf2", "tap"), ("thinn-4-k128of128-n3-xf2", "tap"),
    ("smallk-c3-ragged", "unused"), ("thin-straddle", "unused"), ("smalln-6-k32of64-n3-xf2", "unused"), ("thinn-7-k32of64-n3-xf2", "unused"),
    ("smallk-n160", "lastblock"), ("thin-n256", "lastblock"),
    ("smalln-4-k128of128-n3-xf2", "pad"), ("smalln-2-k96of96-n2-xf1", "pad"), ("thinn-4-k128of128-n3-xf2", "pad"), ("thinn-2-k64of64-n4-xf1", "pad"),
])
def test_one_mistake_in_a_rows_kernel_is_seen(cid, mut):
    c = T.rows_case(cid)
    assert mut in T.ROWS_MUTANTS
    out = T.rows_store(c, T.rows_value(c, acc=torch.float32, xfdt=torch.float32, mut=mut))
    figs = rows_figures(c, out)
    assert figs["out"][0] > 10 * figs["out"][1], (cid, mut, figs)


@pytest.mark.parametrize("cid", ["smallk-c3-ragged", "smallk-out16", "smallk-n96"])
def test_rows_past_the_end_in_the_tracker_are_seen(cid):
    c = T.rows_case(cid)
    assert c.track and c.bias and T.rows_dims(c)[0] % T.TP != 0
    v = T.rows_ref(c)
    bar, _ = T.rows_bar(c)
    ref, allow = T.track_ref(c, v, bar)
    wrong, _ = T.track_ref(c, v, bar, ragged_included=True)
    assert T.track_ratio(ref.float(), ref, allow) <= 1.0
    assert T.track_ratio(wrong.float(), ref, allow) > 10
    assert torch.equal(wrong[:-1], ref[:-1])   # (only the ragged tile differs)


@pytest.mark.parametrize("cid", ["thin-straddle", "smallk-out16"])
def test_the_bias_added_after_the_rounding_is_seen(cid):
    c = T.rows_case(cid)
    figs = rows_figures(c, T.rows_bias_early(c))
    assert figs["out"][0] > figs["out"][1], (cid, figs)
    assert _passes(rows_figures(c, T.rows_store(c, T.rows_ref(c))))


def test_an_unwritten_element_fails_every_criterion():
    c = T.rows_case("smallk-c3-ragged")
    out = T.rows_store(c, T.rows_ref(c)).clone()
    trk = _track32(c, out)
    out[17, 3] = float("nan")
    trk[2, 5] = float("nan")
    figs = rows_figures(c, out, trk)
    assert not figs["out"][0] <= figs["out"][1] and not figs["track"][0] <= 1.0
    w = T.wg_case("smallk-k1-3of4-m128-ns5")
    got = T.wg_value(w, acc=torch.float32)
    gw, gb = got.gw.float().clone(), got.gb.float().clone()
    gw[5, 4, 1] = float("nan")
    gb[7] = float("nan")
    figs = wg_figures(w, gw, gb)
    assert not figs["dW"][0] <= figs["dW"][1] and not figs["db"][0] <= 1.0
