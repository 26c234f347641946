"""tests/bf16_tile_refs.py held to the library and to torch without a GPU: what tests/test_bf16_tile_edges_gpu.py rests on.

  * every case's argument block, with placeholder pointers, is named by the library (vae_igemm_kernel_name) as the instantiation
    the case states;
  * the restated plan agrees with the library where the library answers: vae_conv_gstat_chunks, and the eligibility seen through
    the name on both sides of each threshold (191 / 192 tiles, M below 32768);
  * every regime is claimed by a case whose plan has the property (bf16_tile_refs.HOLDS);
  * the float64 reference agrees with torch's fp32 CPU arithmetic in another formulation (autograd for the dgrads, an explicit
    repeat for the upsample) on the same rounded operands;
  * the criterion can fail: five planted mistakes, applied to the float64 result on the CPU, each far above ratio 1."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import bf16_tile_refs as R

P = 4096   # a placeholder pointer: non-null, 16-byte aligned, never dereferenced (no launch here)


@pytest.fixture(scope="module")
def ops():
    from vaehip import ops as o
    from vaehip.lib import lib
    lib.load()
    return o


def _block(ops, c, **over):
    a = R.args(c._replace(**over) if over else c, ops)
    for f in R.pointer_fields(c):
        setattr(a, f, C.c_void_p(P))
    return a


def _name(ops, a):
    return ops._kernel_name("vae_igemm_kernel_name", a)


def test_the_library_names_every_case(ops):
    for c in R.CASES:
        a = _block(ops, c)
        if c.form != "phase":
            assert _name(ops, a) == c.kernel, (c.name, _name(ops, a))
            continue
        for pa, pb in R.PHASES:
            a.tapmask = R.tapmask(pa, pb)
            assert a.tapmask == ops._phase_tapmask(pa, pb)
            assert _name(ops, a) == c.kernel, (c.name, pa, pb, _name(ops, a))
            assert ops.lib.query("vae_conv_phase_ok", C.byref(a)) == 1, c.name
        print(f"{c.name:20s} {c.kernel}")
    assert {c.fam for c in R.CASES} == {"tile", "wide", "conv1"}
    # the storage flags each block carries are the ones its kernel honours
    for c in R.CASES:
        assert ops.lib.query("vae_conv_io16_ok", C.byref(_block(ops, c))) == 1, c.name


def test_the_plan_agrees_with_the_library(ops):
    from vaehip.lib import lib
    for c in R.CASES:
        p, a = R.plan(c), _block(ops, c)
        if c.fam != "conv1":
            assert p["whole_tiles"], c.name
            assert a.N == c.N and a.K == c.K and a.M == math.prod(R.out_shape(c)[:3]) // (4 if c.form == "phase" and not c.dgrad else 1)
        if "s" in c.epi:
            assert lib.query("vae_conv_gstat_chunks", C.byref(a)) == p["gstat_chunks"] > 0, c.name
        if c.fam == "wide":
            assert p["eligible"] and p["kchunks"] % 2 == 0, c.name   # (the 6-stage loop takes chunks in pairs)
            # one image fewer: below 192 tiles (or, where it is not, still wide) -- the plan and the name agree
            B, H, W = c.bhw
            for b in range(1, B):
                d = c._replace(bhw=(b, H, W))
                wide = _name(ops, _block(ops, d)).startswith("conv3_wide_bf16_kernel")
                assert wide == R.plan(d)["eligible"] == (R.plan(d)["ntiles"] >= R.WIDE_MIN_TILES), (c.name, b)
            if c.form == "plain":  # without the image, and under no_wide, the 128-pixel kernel
                with ops.option("no_wide"):
                    assert _name(ops, a).startswith("conv3_tile_bf16_kernel<"), c.name
        if c.fam == "tile" and c.a == "a16":
            assert not R.plan(c._replace(fam="wide"))["eligible"], c.name   # nothing the wide kernel would take
        if c.fam == "conv1":
            assert p["eligible"], c.name
            B, H, W = c.bhw
            small = c._replace(bhw=(1, H // 2 if B == 2 else 99, W))   # M = 16384 / 32472
            assert not R.plan(small)["eligible"] and _name(ops, _block(ops, small)).startswith("igemm_rows_bf16_kernel"), c.name
            assert (p["grid"], p["stride"]) == (p["slices"] * p["wpn"], 4 * p["wpn"])
    # a 512-row dgrad slice does not fit LDS: the plan and the library refuse it alike
    big = R.BY_NAME["c_dg_k256_n512"]._replace(Co=512, kernel="")
    assert not R.plan(big)["eligible"] and _name(ops, _block(ops, big)).startswith("igemm_rows_bf16_kernel")


def test_first_tile_is_a_permutation_and_every_tile_has_one_owner():
    for c in R.CASES:
        if c.fam == "conv1":
            continue
        p = R.plan(c)
        firsts = sorted(R.first_tile(p["grid"], w) for w in range(p["grid"]))
        assert firsts == list(range(p["grid"])), c.name
        owned = sorted(t for w in range(p["grid"]) for t in R.tiles_of(c, p, w))
        assert owned == list(range(p["ntiles"])), c.name
        counts = {len(R.tiles_of(c, p, w)) for w in range(p["grid"])}
        assert (max(counts), min(counts)) == (p["max_tiles"], p["min_tiles"]), c.name


def test_every_regime_is_claimed_and_held():
    for r in R.REGIMES:
        holders = [c for c in R.CASES if r in c.regimes]
        assert holders, f"no case claims: {r}"
        for c in holders:
            assert R.HOLDS[r](c, R.plan(c)), (c.name, r, R.plan(c))
    for c in R.CASES:
        assert c.regimes and c.why and R.route(c).startswith("direct launch"), c.name
    # both fused transforms, both directions of every family, both tap-block kernels
    assert {c.a for c in R.CASES if R.T_XF in c.regimes} == {"xf1", "xf2"}
    assert {(c.fam, c.dgrad) for c in R.CASES} == {(f, d) for f in ("tile", "wide", "conv1") for d in (False, True)}
    assert {c.kernel for c in R.CASES if c.fam == "wide"} == {f"conv3_wide_bf16_kernel<{d},{k}>" for d in ("false", "true") for k in (2, 3)}
    assert {(c.K, c.N) for c in R.CASES if c.fam == "conv1" and not c.dgrad} == {(k, n) for k in (128, 256, 512) for n in (128, 512)}
    assert {(c.K, c.N) for c in R.CASES if c.fam == "conv1" and c.dgrad} == {(k, n) for k in (128, 256) for n in (128, 512)}
    two3 = R.plan(R.BY_NAME["c_k128_n512"])
    assert two3["blocks_per_wave"] == [2, 3] and two3["nblocks"] == 2 * two3["stride"] + 1
    for name in R.OPS + R.LDC_PAD + R.GUARDED + R.REPEAT + R.OPTIONS:
        assert name in R.BY_NAME
    for name in R.GUARDED + R.REPEAT:
        p = R.plan(R.BY_NAME[name])
        assert p.get("max_tiles", 0) >= 2 or max(p.get("blocks_per_wave", [0])) >= 2, name


def _macs(c):
    return math.prod(R.out_shape(c)) * c.K * (1 if c.fam == "conv1" else 9)


def _torch32(c, act, w):
    """the case's contraction by torch in fp32, formulated another way than bf16_tile_refs.contraction"""
    a = act.float().permute(0, 3, 1, 2)
    w = w.float()
    pad = 0 if c.fam == "conv1" else 1
    if c.form == "phase" and not c.dgrad:   # tap by tap on the padded map
        B, _, H, W = a.shape
        ap = F.pad(a, (1, 1, 1, 1))
        y = torch.zeros(B, c.Co, 2 * H, 2 * W)
        for pa, pb in R.PHASES:
            for kh in R._PHASE_ROWS[pa]:
                for kw in R._PHASE_ROWS[pb]:
                    y[:, :, pa::2, pb::2] += torch.einsum("bchw,oc->bohw", ap[:, :, kh:kh + H, kw:kw + W], w[:, :, kh, kw])
        return y.permute(0, 2, 3, 1)
    if c.dgrad:   # the gradient of the forward convolution by autograd
        B, H, W = c.bhw
        if c.form == "phase":
            out = 0
            for pa, pb in R.PHASES:
                xg = torch.zeros(B, c.Ci, H, W, requires_grad=True)
                (g,) = torch.autograd.grad(F.conv2d(xg, R._masked(w, pa, pb), None, 1, 1), xg, a[:, :, pa::2, pb::2].contiguous())
                out = out + g
            return out.permute(0, 2, 3, 1)
        xg = torch.zeros(B, c.Ci, H, W, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv2d(xg, w, None, 1, pad), xg, a.contiguous())
        return g.permute(0, 2, 3, 1)
    if c.form == "up":
        a = a.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return F.conv2d(a, w, None, 1, pad).permute(0, 2, 3, 1)


def test_the_reference_agrees_with_torch_fp32():
    """fp32 sums of n <= 4608 products of exactly representable bf16 x bf16 terms: blocked sums stay near sqrt(n) 2^-24 of the
    sum of magnitudes, a few 1e-6 of max|v|; 1e-5 separates that from any wrong tap, channel or pixel (1e-2 and more)."""
    n = 0
    for c in R.CASES:
        if _macs(c) > 1e10:  # (every case of the table is below it: the whole table is checked)
            continue
        inp = R.inputs(c.name)
        act, w16 = R.operand_read(c, inp), R.r16(inp["w"]).double()
        v = R.reference(c)
        assert tuple(v.shape) == R.out_shape(c) and v.dtype == torch.float64
        t32 = R.epilogue64(c, inp, _torch32(c, act, w16).double())
        err = float((t32 - v).abs().max() / v.abs().max())
        print(f"{c.name:20s} fp32 CPU vs float64 reference {err:.2e}")
        assert err < 1e-5, (c.name, err)
        # and a correct kernel's stored result passes the criterion
        assert R.ratio(R.stage(c, R.store(c, v))) <= 1.0, c.name
        n += 1
    assert n == len(R.CASES), n


# ---------------------------------------------------------------------------------------------------- the criterion can fail
def _mut_last_chunk_dropped(c):
    inp = R.inputs(c.name)
    act = R.operand_read(c, inp).clone()
    assert c.K % R.BK != 0
    act[..., c.K - c.K % R.BK:] = 0.0   # (the contraction's channels are the operand's last dimension, forward and dgrad)
    return R.store(c, R.epilogue64(c, inp, R.contraction(c, act, R.r16(inp["w"]).double())))


def _mut_tail_tile_zero(c):
    got = R.store(c, R.reference(c)).clone()
    got[..., (c.N // R.BN) * R.BN:] = 0.0
    return got


def _mut_halo_column_of_the_neighbour(c):
    """the tile at x0 = 32 of image 0, rows 0..3, reads its left halo column (x = 31) from the tile before it (x = -1 + 32 k)"""
    inp = R.inputs(c.name)
    act = R.operand_read(c, inp).clone()
    act[:, :, 31, :] = act[:, :, 63, :]
    v2 = R.epilogue64(c, inp, R.contraction(c, act, R.r16(inp["w"]).double()))
    got = R.store(c, R.reference(c)).clone()
    got[0, 0:R.TH[c.fam], 32, :] = R.store(c, v2)[0, 0:R.TH[c.fam], 32, :]
    return got


def _mut_first_chunk_with_previous_n0(c):
    """a workgroup's second tile multiplies its first 32-channel chunk with the weight rows of the tile before it (a weight stage
    that was not replaced): rows n0p .. of the weight image, zeros beyond N"""
    p, inp = R.plan(c), R.inputs(c.name)
    th = R.TH[c.fam]
    for w in range(p["grid"]):
        ts = R.tiles_of(c, p, w)
        if len(ts) >= 2 and R.decode(c, ts[0], p)[3] != R.decode(c, ts[1], p)[3]:
            break
    else:
        raise AssertionError("no workgroup changes n0")
    (_, _, _, n0p), (b, y0, x0, n0) = R.decode(c, ts[0], p), R.decode(c, ts[1], p)
    assert not c.dgrad and c.form == "plain"
    w16 = R.r16(inp["w"]).double()
    wpad = torch.cat([w16, torch.zeros(R.BN, *w16.shape[1:], dtype=w16.dtype)])
    nn = min(R.BN, c.N - n0)
    dw = (wpad[n0p:n0p + nn] - w16[n0:n0 + nn])[:, :R.BK]
    act = F.pad(R.operand_read(c, inp)[b].permute(2, 0, 1)[None, :R.BK], (1, 1, 1, 1))[:, :, y0:y0 + th + 2, x0:x0 + R.TW + 2]
    delta = F.conv2d(act, dw)[0].permute(1, 2, 0)
    v = R.reference(c).clone()
    v[b, y0:y0 + th, x0:x0 + R.TW, n0:n0 + nn] += delta
    return R.store(c, v)


def _mut_block_unwritten(c):
    p = R.plan(c)
    got = R.store(c, R.reference(c)).clone().reshape(-1, c.N)
    blk = p["nblocks"] - 1   # the block only the 3-block wave reaches
    got[blk * 32:(blk + 1) * 32, c.N - R.C1_BN:] = 0.0   # a lucky zero, not the prefill
    return got.reshape(R.out_shape(c))


PLANTED = [("the last partial chunk dropped", _mut_last_chunk_dropped, ("t_k40_n264", "t_dg_k72_n40_o16", "t_k72_n40_o16")),
           ("the tail channel tile zero", _mut_tail_tile_zero, ("t_k40_n264_o16", "t_k8_n40", "w_576_tn3", "w_k64_n136_260")),
           ("one halo column taken from the neighbouring tile", _mut_halo_column_of_the_neighbour, ("t_track_n136", "w_k64_n136_260")),
           ("a tile's first chunk with the previous tile's n0 weights", _mut_first_chunk_with_previous_n0, ("t_576_k32_o16", "w_576_tn3")),
           ("one 32-row block unwritten", _mut_block_unwritten, ("c_k128_n512",))]


def test_the_criterion_rejects_planted_mistakes():
    smallest = math.inf
    for what, mut, names in PLANTED:
        for name in names:
            c = R.BY_NAME[name]
            good = R.ratio(R.stage(c, R.store(c, R.reference(c))))
            bad = R.ratio(R.stage(c, mut(c)))
            print(f"{what:58s} {name:18s} ratio {bad:10.1f}   (unharmed: {good:.2f})")
            assert good <= 1.0 and bad > 50.0, (what, name, good, bad)
            smallest = min(smallest, bad)
    print(f"smallest ratio of a planted mistake: {smallest:.1f}")
