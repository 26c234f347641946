"""Frozen parameters, host side (no GPU, no launch): prefix resolution, the merged arena ranges, the chunk table of the
*_ranges entry points, the reducer's plan over the trainable span, and the trainer state's refusal of another set."""
import pytest
import torch


@pytest.fixture(scope="module")
def vae():
    from vaehip.autoencoder import AutoencoderKLHip
    return AutoencoderKLHip()


def _norm_prefixes(vae):
    return [n for n, m in vae.named_modules() if isinstance(m, torch.nn.GroupNorm)]


def _sets(vae):
    return {"all": "all", "decoder": "decoder", "encoder": "encoder", "norms": _norm_prefixes(vae)}


def test_prefix_resolution_shorthands_and_errors(vae):
    from vaehip.trainable import resolve_trainable
    names = [n for n, _ in vae.named_parameters()]
    assert resolve_trainable(names, "all") == set(names)
    dec = resolve_trainable(names, "decoder")
    enc = resolve_trainable(names, "encoder")
    assert dec == {n for n in names if n.startswith("decoder.") or n.startswith("post_quant_conv.")}
    assert enc == {n for n in names if n.startswith("encoder.") or n.startswith("quant_conv.")}
    assert dec | enc == set(names) and not dec & enc
    # inside a list `decoder` is the plain prefix; `quant_conv` does not match `post_quant_conv`; a parameter's own name is a prefix
    assert resolve_trainable(names, ["decoder"]) == {n for n in names if n.startswith("decoder.")}
    assert resolve_trainable(names, ["quant_conv"]) == {"quant_conv.weight", "quant_conv.bias"}
    assert resolve_trainable(names, ["encoder.conv_in.bias"]) == {"encoder.conv_in.bias"}
    up3 = resolve_trainable(names, ["decoder.up_blocks.3", "encoder.mid_block"])
    assert up3 == {n for n in names if n.startswith("decoder.up_blocks.3.") or n.startswith("encoder.mid_block.")}
    # a prefix is a whole name component: up_blocks.1 must not take up_blocks.10 (here: `decoder.up` matches nothing)
    for bad in (["decoder.up"], ["decoder", "nope"], "vae.decoder", ["encoder.conv_in.w"]):
        with pytest.raises(ValueError, match="matches no parameter"):
            resolve_trainable(names, bad)
    with pytest.raises(ValueError, match="empty"):
        resolve_trainable(names, [])


def test_apply_sets_requires_grad_and_none_keeps_the_users(vae):
    from vaehip.trainable import apply_trainable
    try:
        apply_trainable(vae, "decoder")
        assert all(p.requires_grad == (n.startswith("decoder.") or n.startswith("post_quant_conv.")) for n, p in vae.named_parameters())
        apply_trainable(vae, None)  # leaves it
        assert not vae.encoder.conv_in.weight.requires_grad and vae.decoder.conv_in.weight.requires_grad
        vae.requires_grad_(False)
        with pytest.raises(ValueError, match="empty"):
            apply_trainable(vae, None)
    finally:
        vae.requires_grad_(True)


@pytest.mark.parametrize("which", ["all", "decoder", "encoder", "norms"])
def test_trainable_ranges_cover_exactly_the_trainable_entries(vae, which):
    from vaehip.trainable import apply_trainable, check_ranges
    a = vae.arena
    try:
        apply_trainable(vae, _sets(vae)[which])
        ranges = a.trainable_ranges()
        check_ranges(ranges, a.total)  # non-empty, sorted, disjoint, starts on multiples of 4
        assert all(b % 8 == 0 for b, _ in ranges)
        inside = torch.zeros(a.total, dtype=torch.bool)
        for b, e in ranges:
            assert not inside[b:e].any()
            inside[b:e] = True
        pad = torch.ones(a.total, dtype=torch.bool)
        for _, p, o, n in a.entries:
            pad[o:o + n] = False
            assert bool(inside[o:o + n].all()) if p.requires_grad else not bool(inside[o:o + n].any())
        # what a range holds beside trainable elements is zero padding between two trainable neighbours (or the arena's tail)
        tr = torch.zeros(a.total, dtype=torch.bool)
        for _, p, o, n in a.entries:
            if p.requires_grad:
                tr[o:o + n] = True
        assert bool((inside == tr)[~pad].all()) and bool(pad[inside & ~tr].all())
        # merged: no range starts where another could have continued (the entry before a range's first is frozen or absent)
        first = {o: i for i, (_, _p, o, _n) in enumerate(a.entries)}
        for b, _e in ranges:
            i = first[b]
            assert i == 0 or not a.entries[i - 1][1].requires_grad
        if which == "all":
            assert ranges == [(0, a.total)]
        elif which in ("decoder", "encoder"):
            assert len(ranges) == 1
            split = a.offset_of[id(vae.post_quant_conv.weight)]
            assert ranges[0] == ((split, a.total) if which == "decoder" else (0, split))
        else:
            # weight and bias of a GroupNorm are neighbours: one range per norm, both vectors in it
            norms = [m for m in vae.modules() if isinstance(m, torch.nn.GroupNorm)]
            assert len(ranges) == len(norms)
            assert sorted(e - b for b, e in ranges) == sorted(2 * m.num_channels for m in norms)
    finally:
        vae.requires_grad_(True)


def test_attach_grads_gives_frozen_parameters_none(vae):
    from vaehip.trainable import apply_trainable
    try:
        apply_trainable(vae, "encoder")
        vae.arena.attach_grads()
        for n, p in vae.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and p.grad.data_ptr() == vae.arena.grad.data_ptr() + 4 * vae.arena.offset_of[id(p)], n
            else:
                assert p.grad is None, n
    finally:
        vae.requires_grad_(True)
        vae.arena.attach_grads()


def test_chunk_prefix_against_a_brute_force_count():
    from vaehip.trainable import check_ranges, chunk_prefix
    C = 32768
    gen = torch.Generator().manual_seed(5)
    cases = [[(0, 1)], [(0, C)], [(0, C + 4)], [(0, 2 * C - 1)], [(8, 24)], [(0, 8), (8, 24)], [(0, 3 * C), (3 * C + 8, 3 * C + 9)]]
    b, many = 0, []
    for _ in range(130):
        n = int(torch.randint(1, 3 * C, (1,), generator=gen))
        many.append((b, b + n))
        b += (n + 7) // 8 * 8 + 8
    cases.append(many)
    for ranges in cases:
        check_ranges(ranges)
        got = chunk_prefix(ranges, C)
        # brute force: walk every range in steps of C and count the steps
        want, k = [0], 0
        for lo, hi in ranges:
            i = lo
            while i < hi:
                k += 1
                i += C
            want.append(k)
        assert got == want
        # every chunk lies inside its range and the chunks tile the ranges
        for s, (lo, hi) in enumerate(ranges):
            nch = got[s + 1] - got[s]
            assert nch >= 1 and lo + (nch - 1) * C < hi <= lo + nch * C


def test_range_table_contract_is_checked_when_it_is_built():
    from vaehip.trainable import check_ranges
    for bad in ([], [(2, 8)], [(8, 8)], [(8, 4)], [(0, 16), (8, 24)], [(16, 24), (0, 8)], [(-4, 8)]):
        with pytest.raises(ValueError, match="range table"):
            check_ranges(bad)
    with pytest.raises(ValueError, match="beyond"):
        check_ranges([(0, 16)], total=12)
    check_ranges([(0, 8), (8, 24), (1000, 1001)], total=1001)


@pytest.mark.parametrize("which", ["decoder", "encoder", "norms"])
def test_reducer_plan_stays_inside_the_trainable_span(vae, which):
    from vaehip.dp import GradBucketReducer
    from vaehip.trainable import apply_trainable, span_of
    a = vae.arena
    try:
        apply_trainable(vae, _sets(vae)[which])
        lo, hi = span_of(a.trainable_ranges())
        red = GradBucketReducer(a.grad, bucket_mb=16.0, span=(lo, hi))
        assert red.buckets[0][1] == hi and red.buckets[-1][0] == lo
        for (b0, b1), nxt in zip(red.buckets, red.buckets[1:] + [None]):
            assert lo <= b0 < b1 <= hi and b0 % 4 == 0
            assert nxt is None or nxt[1] == b0  # contiguous, from the end down
        assert GradBucketReducer(a.grad, bucket_mb=16.0).buckets[-1][0] == 0  # no span: the whole buffer, as before
        with pytest.raises(ValueError):
            GradBucketReducer(a.grad, span=(lo + 2, hi))
    finally:
        vae.requires_grad_(True)


def test_trainer_state_refuses_another_trainable_set():
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    w = SDXLVAEWrapper("synthetic:1")
    tr = HipTrainer(w, trainable="decoder", use_ema=True)
    sd = tr.state_dict()
    split = w.vae.arena.offset_of[id(w.vae.post_quant_conv.weight)]
    assert sd["trainable_ranges"] == [[split, w.vae.arena.total]]
    assert w.vae.encoder.conv_in.weight.requires_grad is False
    HipTrainer(w, trainable="decoder", use_ema=True).load_state_dict(sd)  # the same set loads
    other = HipTrainer(w, trainable="encoder", use_ema=True)
    with pytest.raises(ValueError) as ei:
        other.load_state_dict(sd)
    msg = str(ei.value)
    assert f"[{split}, {w.vae.arena.total})" in msg and f"[0, {split})" in msg  # names both sets
    # a state from before parameters could be frozen trained everything
    del sd["trainable_ranges"]
    with pytest.raises(ValueError, match=r"\[0, %d\)" % w.vae.arena.total):
        other.load_state_dict(sd)
    HipTrainer(w, trainable="all", use_ema=True).load_state_dict(sd)
    # set_trainable: refused inside an accumulation window
    tr.micro_step = 1
    with pytest.raises(RuntimeError, match="pending"):
        tr.set_trainable("all")
    tr.micro_step = 0
    tr.set_trainable(["decoder.up_blocks.3"])
    assert len(tr.trainable_ranges) == 1 and not w.vae.decoder.conv_in.weight.requires_grad


def test_config_key_is_read():
    import train
    assert train.trainable_setting({}) == "all" and train.trainable_setting({"trainable_modules": None}) == "all"
    assert train.trainable_setting({"trainable_modules": "decoder"}) == "decoder"
    assert train.trainable_setting({"trainable_modules": ["vae.encoder.mid_block", "decoder.up_blocks.3"]}) == \
        ["encoder.mid_block", "decoder.up_blocks.3"]
    with pytest.raises(ValueError):
        train.trainable_setting({"trainable_modules": 3})
