"""tests/norm_refs.py without a GPU: the float64 GroupNorm references against torch's float64 group_norm and autograd, every
named shape against the property it is in the table for (through the host plans, not arithmetic done by hand), every value
builder for what it claims, and the dead-weight reference against DeadNeuronTracker's per-parameter formulas."""
import math

import numpy as np
import pytest
import torch

import norm_refs as nr

TARGET = (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.Linear, torch.nn.GroupNorm)


# ---------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("name", ["tail_c256", "seven_pixels"])
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("with_add", [False, True])
def test_groupnorm_references_follow_torch_float64(name, silu, with_add):
    c = nr.plain_case(name)
    add = c.add if with_add else None
    r = nr.gn_ref64(c.x, c.gamma, c.beta, silu=silu)
    b = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, silu, add)
    y, act, track, dx, dgamma, dbeta = nr.gn_torch(c.x, c.gamma, c.beta, silu, c.g, add, dt=torch.float64)
    for got, want in ((r.y, y), (r.act, act), (r.track, track), (b.dx, dx), (b.dgamma, dgamma), (b.dbeta, dbeta)):
        assert nr.rel(got, want) < 1e-12
    xg = c.x.double().permute(0, 3, 1, 2).reshape(c.x.shape[0], nr.G, -1)
    assert nr.rel(r.mean, xg.mean(-1)) < 1e-12
    assert nr.elem_rel(r.rstd, 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + nr.EPS)) < 1e-12
    # the scales dgamma / dbeta are measured on bound them
    assert bool((b.dgamma.abs() <= b.dgamma_abs * (1 + 1e-12)).all()) and bool((b.dbeta.abs() <= b.dbeta_abs * (1 + 1e-12)).all())


def test_groupnorm_references_see_a_wrong_term():
    """what the comparison would have to notice: the last pixel left out of the statistics, the group mean of the gradient
    left out of dx -- each moves the reference by far more than any bar of the GPU test (1e-5 .. 2e-5)"""
    c = nr.plain_case("ragged_two")
    r = nr.gn_ref64(c.x, c.gamma, c.beta)
    short = nr.gn_ref64(c.x[:, :, :-1], c.gamma, c.beta)
    assert nr.elem_rel(short.rstd, r.rstd) > 1e-4
    b = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, True)
    shifted = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, True, add=torch.full_like(c.x, 1e-3))
    assert nr.rel(shifted.dx, b.dx) > 1e-4


def test_track_final_reference():
    ws = nr.track_ws(257, 130)
    assert float(ws.min()) >= 1e-6 and float(ws.max()) <= 1e3 and float(ws.max() / ws.min()) > 1e8
    ref = nr.track_final_ref64(ws, 771)
    assert ref.shape == (130,)
    assert abs(float(ref[5]) - math.fsum(ws[:, 5].tolist()) / 771) <= 1e-15 * float(ref[5])


# ---------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("name", sorted(nr.SHAPES))
def test_named_shapes_have_their_stated_properties(name):
    props = nr.shape_properties(name)
    for p in nr.STATED[name]:
        assert props[p], (name, p, nr.SHAPES[name])


def test_the_table_covers_every_property_and_every_channel_count():
    have = {p for name in nr.SHAPES for p in nr.STATED[name]}
    assert have >= {"hw_lt_pr", "one_chunk", "ragged_last", "trailing_empty", "gy8", "b64", "bwd_tail", "grid_stride",
                    "capped", "several_empty", "bwd_short", "per_halved", "one_full_chunk"}
    assert {s[1] for s in nr.SHAPES.values()} == {128, 256, 512}
    assert [nr.pr_of(c) for c in (128, 256, 512)] == [8, 4, 2]


def test_plans_at_the_worked_examples():
    """the figures the shape table quotes"""
    assert nr.stats_plan(2, 33 * 33, 512) == (34, 33)
    n, per = nr.stats_plan(2, 91 * 91, 512)
    assert n >= 256 and sum(1 for k in range(n) if k * per >= 91 * 91) >= 2
    assert nr.stats_plan(40, 64 * 64, 128)[0] == 1024 // 40
    assert nr.row_plan(2, 9, 256) == (16, 1)            # halved down to one unrolled pass: 9 of its 16 pixels exist
    assert nr.row_plan(40, 4096, 128) == (64, 64)       # halved once: 40 * 32 workgroups would be fewer than 2048
    assert nr.row_plan(64, 4096, 128) == (128, 32)      # not halved
    assert nr.final_gy(2, 258) == 8 and nr.final_gy(65, 258) == 1 and nr.final_gy(2, 255) == 1


# ---------------------------------------------------------------------------------------------------- value builders
def test_constant_builder_is_bit_constant():
    for name in ("tail_c256", "one_pixel"):
        c = nr.constant_case(name)
        B, H, W, C = c.x.shape
        cpg = C // nr.G
        bits = c.x.view(torch.int32)
        want = int(torch.tensor(nr.CONST_VALUE).view(torch.int32))
        for b, grp in c.info["const"]:
            assert bool((bits[b, :, :, grp * cpg:(grp + 1) * cpg] == want).all())
        assert (B - 1, nr.CONST_GROUP) in c.info["const"] and (B == 1 or len(c.info["const"]) == 1 + nr.G)
        r = nr.gn_ref64(c.x, c.gamma, c.beta)
        for b, grp in c.info["const"]:
            assert float(r.rstd[b, grp]) == 1.0 / math.sqrt(nr.EPS) and float(r.mean[b, grp]) == float(np.float32(nr.CONST_VALUE))
            assert torch.equal(r.y[b, :, :, grp * cpg:(grp + 1) * cpg],
                               c.beta.double()[grp * cpg:(grp + 1) * cpg].expand(H, W, cpg))
        bw = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, True, c.add)
        assert bool(bw.dx.isfinite().all()) and bool(bw.dgamma.isfinite().all()) and bool(bw.dbeta.isfinite().all())
    only = nr.constant_case("tail_c256")
    r = nr.gn_ref64(only.x[:1], only.gamma, only.beta)     # the constant image alone: the tracker vector is |beta|
    assert torch.equal(r.track, only.beta.double().abs())


@pytest.mark.parametrize("name", ["ragged_two", "tail_c256", "last_empty", "seven_pixels"])
@pytest.mark.parametrize("where", ["first", "last"])
def test_outlier_sits_where_a_thread_reads_first_or_last(name, where):
    """emulates the read order of gn_stats_partial_kernel: thread (pr, quad) of chunk k reads pixels p0 + pr, p0 + pr + PR, ...,
    four channels each"""
    c = nr.outlier_case(name, where)
    B, H, W, C = c.x.shape
    HW, PR, cpg = H * W, nr.pr_of(C), C // nr.G
    nchunk, per = nr.stats_plan(B, HW, C)
    flat = c.x.view(B, HW, C)
    assert len(c.info["at"]) == B * nr.G and int((flat == nr.OUTLIER).sum()) == B * nr.G
    seen = set()
    for b, pix, ch in c.info["at"]:
        assert float(flat[b, pix, ch]) == nr.OUTLIER
        seen.add((b, ch // cpg))
        k = pix // per
        p0, p1 = k * per, min(HW, (k + 1) * per)
        pr = (pix - p0) % PR
        mine = list(range(p0 + pr, p1, PR))          # the pixels of the thread that reads this one
        if where == "first":
            assert pix == mine[0] and ch % 4 == 0    # its pivot pv = v[0]
        else:
            assert pix == mine[-1] and ch % 4 == 3 and pix == p1 - 1
    assert len(seen) == B * nr.G                      # one per (image, group)


def test_silu_plants_lie_where_stated():
    for name in ("seven_pixels", "tail_c256", "last_empty"):
        c = nr.silu_case(name)
        plant, kind = c.info["plant"], c.info["kind"]
        r = nr.gn_ref64(c.x, c.gamma, c.beta, silu=True)
        C = c.x.shape[-1]
        for k, kname in enumerate(nr.GAMMA_KINDS):
            assert {float(plant[ch]) for ch in range(C) if kind[ch] == k} == set(nr.SILU_PLANTS), kname
        for ch in range(C):
            u = r.y[..., ch]
            if kind[ch] < 0:
                assert math.isnan(float(plant[ch])) and abs(float(c.beta[ch])) < 2
                continue
            assert float(c.beta[ch]) == float(plant[ch])
            if kind[ch] == 2:
                assert float(c.gamma[ch]) == 0.0 and bool((u == float(plant[ch])).all())
            else:
                assert (float(c.gamma[ch]) > 0) == (kind[ch] == 0) and 0.05 < abs(float(c.gamma[ch])) < 3
                # xhat of a group of n values is at most sqrt(n - 1); here a few units
                assert float((u - float(plant[ch])).abs().max()) <= abs(float(c.gamma[ch])) * float(r.xhat[..., ch].abs().max()) + 1e-9
                assert float((u - float(plant[ch])).abs().max()) < 16
        assert bool(r.act.isfinite().all())
        if name == "last_empty":   # a map large enough that the spread of a gamma != 0 channel crosses the overflow point itself
            for k in (0, 1):
                for b in (88.0, -88.0):
                    ch = next(i for i in range(C) if kind[i] == k and float(plant[i]) == b)
                    assert float(r.y[..., ch].min()) < b < float(r.y[..., ch].max())
        # below 1e-30 the float64 activation is nothing to take a ratio against
        assert float(r.act[..., (plant == -104.0)].abs().max()) < 1e-30


def test_one_hot_gradient_builder():
    c = nr.one_hot_case("tail_c512")
    B, H, W, C = c.x.shape
    assert int((c.g != 0).sum()) == B
    for b, pix, ch in c.info["hot"]:
        assert float(c.g.view(B, H * W, C)[b, pix, ch]) == 3.0
    ref = nr.gn_bwd_ref64(c.x, c.g, c.gamma, c.beta, False)
    cpg = C // nr.G
    for b, pix, ch in c.info["hot"]:
        grp = ch // cpg
        mask = torch.zeros(C, dtype=torch.bool)
        mask[grp * cpg:(grp + 1) * cpg] = True
        assert bool((ref.dx[b][..., ~mask] == 0).all())        # no pixel of any other group
        assert bool((ref.dx[b][..., mask] != 0).all())         # every pixel of the group


def test_large_mean_builder():
    for ratio in (30.0, 1000.0):
        c = nr.large_mean_case("tail_c256", ratio)
        ch = c.x.double().view(-1, c.x.shape[-1])
        got = (ch.mean(0).abs() / ch.std(0)).median()
        assert 0.5 * ratio < float(got) < 2 * ratio


# ---------------------------------------------------------------------------------------------------- dead-weight scan
def test_dead_layout_is_what_the_gpu_test_needs():
    for fill in (0.0, float("nan")):
        flat, segs, info = nr.dead_layout(fill)
        assert sorted(e - b for b, e in segs) == sorted(2 * list(nr.DEAD_LENGTHS))
        assert sorted((e - b, b % 4) for b, e in segs) == sorted([(L, a) for L in nr.DEAD_LENGTHS for a in (0, 1)])
        prev = 0
        for b, e in segs:            # a gap before every segment and after the last
            assert b - prev >= 3
            gap = flat[prev:b]
            assert bool(gap.isnan().all()) if math.isnan(fill) else bool((gap == 0).all())
            prev = e
        assert flat.numel() - prev >= 3
        inside = torch.cat([flat[b:e] for b, e in segs])
        assert int(inside.isnan().sum()) == 1 and info["nan"] is not None and len(info["inf"]) >= 2
        assert int(inside.isinf().sum()) == len(info["inf"])
        # every plant meets a first element, a last element and both sides of a chunk boundary somewhere
        plants = nr.dead_plants(nr.DEAD_THR)
        for where in ("first", "last", "before", "after"):
            vals = set()
            for s, p, v in info["planted"]:
                L = segs[s][1] - segs[s][0]
                if {"first": p == 0, "last": p == L - 1, "before": p % nr.DEAD_CHUNK == nr.DEAD_CHUNK - 1 and p != L - 1,
                        "after": p % nr.DEAD_CHUNK == 0 and p > 0 and p != L - 1}[where]:
                    vals.add(repr(v))
            assert len(vals) >= 3, (where, vals)
        assert {repr(v) for _, _, v in info["planted"]} == {repr(v) for v in plants}
        for s, p, v in info["planted"]:
            got = float(flat[segs[s][0] + p])
            assert got == float(np.float32(v)) and math.copysign(1, got) == math.copysign(1, v)
        c0 = nr.dead_chunk0(segs)
        assert int(c0[-1]) == sum(max(1, -(-(e - b) // nr.DEAD_CHUNK)) for b, e in segs) == 22


def test_dead_counts_strictness():
    t = np.float32(nr.DEAD_THR)
    below = float(np.nextafter(t, np.float32(0)))
    flat = torch.tensor([float(t), below, -float(t), -0.0, 1e-40, -below, float("inf"), float("nan"), 0.0])
    counts, sums = nr.dead_counts(flat, [(0, 6), (0, 7), (0, 8), (8, 9), (3, 3)], nr.DEAD_THR)
    assert counts == [4, 4, 4, 1, 0]
    assert sums[0] == pytest.approx(2 * float(t) + 2 * below + 1e-40, rel=1e-12) and sums[1] == math.inf and math.isnan(sums[2])
    # a `<=`, or a bound off by one, is a different count
    assert int((flat[:6].abs().numpy() <= t).sum()) == 6
    counts, _ = nr.dead_counts(flat, [(0, 6)], nr.DEAD_THR, athr=[below], use_fixed=False)
    assert counts == [2]


def _tracker(mode, thr=nr.TRACKER_THR, pct=nr.TRACKER_MEAN_PCT):
    from tracking.deadneuron import DeadNeuronTracker
    return DeadNeuronTracker(TARGET, [], threshold=thr, mean_percentage=pct, dead_type=mode)


@pytest.mark.parametrize("mode", ["threshold", "percent_of_mean", "both"])
def test_dead_reference_follows_the_tracker_formulas(mode):
    gen = torch.Generator().manual_seed(17)   # vetted: margin 1.2e-4 (seeds 11 and 13 put a value within 6e-6 of the line)
    parts = [torch.randn(70001, generator=gen) * 0.05, torch.zeros(64), torch.full((64,), 5e-10), torch.zeros(512),
             torch.randn(5, generator=gen) * 1e-5, torch.randn(33000, generator=gen) * 1e-4, torch.full((7,), 2e-9)]
    parts[3][17] = 1e-3            # one non-zero value: mean |w| = 2e-6, not degenerate
    parts[0][:50] = 0.0
    parts[0][50:100] = 5e-6
    segs, off = [], 0
    for p in parts:
        segs.append((off, off + p.numel()))
        off += p.numel()
    flat = torch.cat(parts)
    ref = nr.dead_ref(flat, segs, nr.TRACKER_THR, nr.TRACKER_MEAN_PCT, mode)
    assert ref["margin"] > 1e-5     # no |w| on the adaptive line: the fp32 and the float64 mean count alike
    t = _tracker(mode)
    for (b, e), got in zip(segs, ref["pct"]):
        assert got == pytest.approx(t.get_percentage(flat[b:e]), rel=1e-12, abs=0.0), (mode, b, e)
    if mode != "threshold":         # the degenerate branch was taken, with both outcomes
        assert ref["athr"][1] == 1e-9 and ref["athr"][2] == 1e-9 and ref["athr"][3] != 1e-9
        assert ref["pct"][1] == 100.0 and ref["pct"][2] == 100.0
    if mode == "percent_of_mean":
        assert ref["pct"][6] == 0.0   # mean 2e-9 is not degenerate, and nothing lies below a tenth of it


@pytest.fixture(scope="module")
def planted_model():
    import vae_oracle as vo
    m = vo.OracleAutoencoderKL()
    m.load_state_dict(vo.synthetic_state_dict(m, nr.TRACKER_SEED))
    nr.plant_tracker_params(dict(m.named_parameters()))
    return m


def test_tracker_plants(planted_model):
    p = {n: q.detach() for n, q in planted_model.named_parameters()}
    names = [n for n, _ in planted_model.named_parameters()]
    assert float(p[nr.PLANT_ZERO_BIAS].abs().max()) == 0.0
    assert bool((p[nr.PLANT_TINY_BIAS] == 5e-10).all())
    assert int((p[nr.PLANT_ONE_VALUE] != 0).sum()) == 1 and float(p[nr.PLANT_ONE_VALUE].abs().mean()) >= 1e-9
    w = p[nr.PLANT_LARGE_CONV].detach().permute(0, 2, 3, 1).reshape(-1)
    assert w.numel() > 2 * nr.DEAD_CHUNK and bool((w[:100] == 0).all()) and bool((w[-100:] == 0).all()) and float(w[100]) != 0.0
    i = names.index(nr.PLANT_BETWEEN)
    assert p[names[i - 1]].numel() > nr.DEAD_CHUNK and p[names[i + 1]].numel() + p[names[i + 2]].numel() > 0
    big_after = next(n for n in names[i + 1:] if p[n].numel() > nr.DEAD_CHUNK)
    assert names.index(big_after) - i <= 3 and p[nr.PLANT_BETWEEN].numel() < 1024
    assert int((p[nr.PLANT_BETWEEN] == 0).sum()) == (p[nr.PLANT_BETWEEN].numel() + 1) // 2


@pytest.mark.parametrize("mode", ["percent_of_mean", "both"])
def test_tracker_seed_is_unambiguous(planted_model, mode):
    """torch takes mean |w| in fp32, the scan in float64 (rounded to fp32 once): two thresholds that may differ in their last
    bits.  The model holds 84 M uniformly spread weights, some 40 of which lie within a relative 1e-5 of their parameter's
    threshold whatever the seed, so that margin cannot be asked of it; what the GPU test needs is asked instead: the two
    thresholds of every parameter lie within a relative 1e-5 of each other, no |w| lies between them, and so both ways of
    counting give the same percentage."""
    t = _tracker(mode)
    for name, p in t._eligible(planted_model):
        a = p.detach().abs().reshape(-1)
        ref = nr.dead_ref(a, [(0, a.numel())], nr.TRACKER_THR, nr.TRACKER_MEAN_PCT, mode)
        assert ref["pct"][0] == pytest.approx(t.get_percentage(p.detach()), rel=1e-12, abs=0.0), name
        m32 = a.mean().item()
        if abs(m32) < 1e-9 or ref["athr"][0] == 1e-9:
            assert abs(m32) < 1e-9 and ref["athr"][0] == 1e-9, name
            continue
        lo, hi = sorted((float(np.float32(nr.TRACKER_MEAN_PCT * m32)), float(np.float32(ref["athr"][0]))))
        assert (hi - lo) / hi < 1e-5, name
        assert int(((a >= lo) & (a < hi)).sum()) == 0, name
