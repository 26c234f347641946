"""Weight-side channel dynamics without a GPU: the WeightDynamicsTracker's torch formulas against the float64 references of
tests/wdyn_refs.py, the WeightTable's offsets, chunks and OHWI column mapping on a fake arena, the special cases (frozen
parameter, before the first optimizer step), records / CSV / config handling, and the bound of wdyn_refs itself: an fp32
emulation of the longest chains it admits stays inside it, one dropped or doubled element falls outside."""
import csv
import io
import json
import math
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import wdyn_refs as R

SHAPES = [(1, 1, 1), (5, 1, 1), (3, 1, 7), (4, 1, 8), (2, 9, 3), (3, 9, 4), (5, 9, 5), (8, 9, 64), (2, 1, 260), (130, 1, 4)]
CONSTS_ARGS = (0.9, 0.999, 1e-8, 3)


def _consts():
    from tracking.weightdynamics import adam_constants
    return adam_constants(*CONSTS_ARGS)


# ---------------------------------------------------------------------------------------------------- tracker, torch path
class Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(6, 8, 3, padding=1).to(memory_format=torch.channels_last)
        self.norm = nn.GroupNorm(2, 8)
        self.fc = nn.Linear(8, 5)

    def forward(self, x):
        return self.fc(self.norm(self.conv(x)).mean(dim=(2, 3)))


def _small(steps: int, freeze=()):
    torch.manual_seed(3)
    net = Small()
    for n, p in net.named_parameters():
        if n in freeze:
            p.requires_grad_(False)
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-2, betas=(0.8, 0.95), eps=1e-6)
    x = torch.randn(4, 6, 5, 5)
    for _ in range(max(steps, 1)):
        opt.zero_grad()
        net(x).square().mean().backward()
        if steps:
            opt.step()
    return net, opt


def _okI(t):
    from tracking.weightdynamics import as_okI
    return as_okI(t.detach()).contiguous().numpy()


def test_torch_fallback_matches_the_references():
    from tracking.weightdynamics import METRICS, WeightDynamicsTracker, adam_constants
    net, opt = _small(3)
    assert net.conv.weight.is_contiguous(memory_format=torch.channels_last) and not net.conv.weight.is_contiguous()
    tr = WeightDynamicsTracker({"enabled": True})
    logs = tr.track(net, opt, 3)
    names = [n for n, _ in net.named_parameters()]
    assert sorted(tr.last_raw) == sorted(names) and tr.last_lr == 1e-2
    consts = adam_constants(0.8, 0.95, 1e-6, 3)
    for n, p in net.named_parameters():
        st = opt.state[p]
        r = R.ref(_okI(p), _okI(p.grad), _okI(st["exp_avg"]), _okI(st["exp_avg_sq"]), consts)
        assert sorted(tr.last_raw[n]) == sorted(r) and ("in" in r) == (p.dim() > 1)
        for view in r:
            sums, amax = tr.last_raw[n][view]
            assert np.allclose(sums, r[view]["sums"], rtol=0, atol=1e-13 * r[view]["scale"].max() + 1e-300)
            assert R.same_bits(amax, r[view]["absmax"])
            s = r[view]["sums"]
            want = {"weight_norm_per_channel": np.sqrt(s[:, 0]), "weight_abs_max_per_channel": r[view]["absmax"].astype(np.float64),
                    "grad_norm_per_channel": np.sqrt(s[:, 1]), "scale_gradient_per_channel": s[:, 2],
                    "update_ratio_per_channel": 1e-2 * np.sqrt(s[:, 5]) / np.maximum(np.sqrt(s[:, 0]), 1e-30),
                    "grad_momentum_cosine_per_channel": s[:, 4] / np.sqrt(s[:, 1] * s[:, 3])}
            for metric in METRICS:
                (step, vec), = tr.history[(n, view, metric)]
                assert step == 3 and vec.dtype == np.float64 and np.allclose(vec, want[metric], rtol=1e-11, atol=0), (n, view, metric)
                assert logs[f"weight_dynamics/{n}/{view}/{metric}_max"] == float(vec.max())
    cos = tr.history[("conv.weight", "out", "grad_momentum_cosine_per_channel")][0][1]
    assert (np.abs(cos) <= 1.0 + 1e-12).all() and cos.shape == (8,)
    assert tr.history[("conv.weight", "in", "weight_norm_per_channel")][0][1].shape == (6,)


def test_in_view_is_the_ohwi_column():
    """one input channel of the conv set to a marker: exactly that entry of the in view sees it, every out slice does"""
    from tracking.weightdynamics import WeightDynamicsTracker
    net, opt = _small(1)
    with torch.no_grad():
        net.conv.weight[:, 4] = 7.0
    tr = WeightDynamicsTracker({"enabled": True, "metrics": ["weight_abs_max_per_channel"]})
    tr.track(net, opt, 1)
    vin = tr.history[("conv.weight", "in", "weight_abs_max_per_channel")][0][1]
    vout = tr.history[("conv.weight", "out", "weight_abs_max_per_channel")][0][1]
    assert vin[4] == 7.0 and (np.delete(vin, 4) < 1.0).all() and (vout == 7.0).all()


def test_frozen_parameter_reports_weights_only():
    from tracking.weightdynamics import METRICS, WEIGHT_METRICS, WeightDynamicsTracker
    net, opt = _small(2, freeze=("norm.weight",))
    net.norm.weight.grad = torch.full_like(net.norm.weight, 1e6)  # its gradient slot may hold anything
    tr = WeightDynamicsTracker({"enabled": True})
    tr.track(net, opt, 2)
    for metric in METRICS:
        vec = tr.history[("norm.weight", "out", metric)][0][1]
        assert np.isfinite(vec).all() if metric in WEIGHT_METRICS else np.isnan(vec).all(), metric
        assert np.isfinite(tr.history[("norm.bias", "out", metric)][0][1]).all(), metric


def test_before_the_first_step_ratio_and_cosine_are_nan():
    from tracking.weightdynamics import METRICS, WeightDynamicsTracker
    net, opt = _small(0)
    tr = WeightDynamicsTracker({"enabled": True})
    tr.track(net, opt, 0)
    for metric in METRICS:
        vec = tr.history[("fc.weight", "out", metric)][0][1]
        assert np.isnan(vec).all() if metric in METRICS[4:] else np.isfinite(vec).all(), metric
    tr.track(net, None, 1)  # no optimizer at all: the same
    assert np.isnan(tr.history[("fc.weight", "in", METRICS[4])][1][1]).all()
    assert np.isfinite(tr.history[("fc.weight", "in", METRICS[2])][1][1]).all()


def test_records_csv_and_config():
    from tracking.weightdynamics import CSV_FIELDS, METRICS, VIEWS, WeightDynamicsTracker
    d = WeightDynamicsTracker()
    assert (d.enabled, d.track_interval, d.target_parameters, d.views, d.metrics) == (False, 100, None, VIEWS, METRICS)
    with pytest.raises(ValueError, match=r"weight_dynamics\.metrics: unknown \['weight_norm'\]; choose from"):
        WeightDynamicsTracker({"metrics": ["weight_norm"]})
    with pytest.raises(ValueError, match=r"weight_dynamics\.views: unknown \['both'\]; choose from \['out', 'in'\]"):
        WeightDynamicsTracker({"views": ["both"]})
    with pytest.raises(ValueError, match="unknown keys"):
        WeightDynamicsTracker({"interval": 3})
    net, opt = _small(2)
    with pytest.raises(ValueError, match="matches no parameter"):
        WeightDynamicsTracker({"target_parameters": ["conv2"]}).track(net, opt, 1)
    tr = WeightDynamicsTracker({"enabled": True, "target_parameters": ["vae.fc", "conv.weight"], "views": ["in"],
                                "metrics": ["update_ratio_per_channel", "weight_norm_per_channel"]})
    assert [n for n, _ in tr.targets(net)] == ["conv.weight", "fc.weight", "fc.bias"]
    tr.track(net, opt, 2)
    tr.track(net, opt, 4)
    recs = tr.export_records()
    assert [tuple(r) for r in recs] == [CSV_FIELDS] * len(recs)
    keys = [(r["global_step"], r["parameter"], r["view"], r["metric"]) for r in recs]
    want = [(s, p, "in", m) for s in (2, 4) for p in ("conv.weight", "fc.weight")  # fc.bias has no in view
            for m in ("weight_norm_per_channel", "update_ratio_per_channel")]
    assert sorted(keys) == sorted(want) and len(set(keys)) == len(keys)
    buf = io.StringIO()
    wr = csv.DictWriter(buf, fieldnames=list(CSV_FIELDS))
    wr.writeheader()
    wr.writerows(recs)
    rows = list(csv.DictReader(io.StringIO(buf.getvalue())))
    for row, rec in zip(rows, recs):
        vec = np.array(json.loads(row["metric_value"]))
        assert len(vec) == int(row["num_channels"]) == {"conv.weight": 6, "fc.weight": 8}[row["parameter"]]
        assert float(row["min"]) == vec.min() and float(row["max"]) == vec.max() and float(row["median"]) == float(np.median(vec))
        assert row["metric_type"] == rec["metric"][:-len("_per_channel")] + "_vector"


# ---------------------------------------------------------------------------------------------------- WeightTable
def _fake_arena(shapes, gap=8):
    params, off, offset_of = [], 0, {}
    for i, s in enumerate(shapes):
        p = torch.zeros(s)
        offset_of[id(p)] = off
        params.append((f"p{i}", p))
        off += (p.numel() + gap + 7) // 8 * 8
    return types.SimpleNamespace(flat=torch.zeros(off), total=off, offset_of=offset_of), params


def test_weight_table_offsets_chunks_and_whole_rows():
    from vaehip.lib import lib
    from vaehip.weight_table import WeightTable, rows_per_chunk
    chunk = lib.query("vae_wdyn_chunk")
    assert chunk == 32768
    shapes = [(8, 64, 3, 3), (5,), (130, 4), (2, chunk + 4), (40, 512, 3, 3), (3, 7), (16, 128, 1, 1)]
    arena, params = _fake_arena(shapes)
    order = [4, 0, 6, 1, 3, 2, 5]  # not memory order
    t = WeightTable(arena, [params[i] for i in order])
    assert [s.name for s in t.slots] == [f"p{i}" for i in order] and t.nseg == 7
    out0 = in0 = ws0 = chunk0 = 0
    for s, i in zip(t.slots, order):
        p = params[i][1]
        O, K, I = (p.shape[0], p.shape[2] * p.shape[3], p.shape[1]) if p.dim() == 4 else (p.shape[0], 1, p.shape[1] if p.dim() == 2 else 1)
        assert (s.off, s.O, s.K, s.I) == (arena.offset_of[id(p)], O, K, I)
        assert (s.out0, s.in0, s.ws0, s.chunk0) == (out0, in0, ws0, chunk0)
        rpc = rows_per_chunk(K, I, chunk)
        assert rpc >= 1 and (rpc * K * I <= chunk or rpc == 1)  # whole rows; a row longer than the chunk is one workgroup
        assert rpc <= 8 or I == 1
        assert s.nchunk == math.ceil(O / rpc) and (s.nchunk - 1) * rpc < O
        out0, chunk0 = out0 + O, chunk0 + s.nchunk
        if I > 1:
            in0, ws0 = in0 + I, ws0 + s.nchunk * I
    assert (t.n_out, t.n_in, t.nchunk, t.nwords) == (out0, in0, chunk0, ws0 * 7)
    assert t.slot("p4").nchunk == 40 // (chunk // 4608) + 1 and t.slot("p3").nchunk == 2 and t.slot("p1").nchunk == 1
    assert t.tab.dtype == torch.int64 and tuple(t.tab.shape) == (7, 8)
    assert t.tab.tolist() == [[s.off, s.O, s.K, s.I, s.out0, s.in0, s.ws0, s.chunk0] for s in t.slots]
    assert t.extent == max(s.off + s.O * s.K * s.I for s in t.slots) <= arena.total
    assert t.in_slice(t.slot("p1")) is None and t.in_slice(t.slot("p5")) == slice(t.slot("p5").in0, t.slot("p5").in0 + 7)


def test_weight_table_entry_addresses_the_ohwi_column():
    """one input channel of a conv weight set to a marker through the arena's own view (ParamArena.view_of): the entry's
    [O][K][I] indexing off + (o K + k) I + i finds the marker at exactly that i"""
    from vaehip.autoencoder import ParamArena
    from vaehip.weight_table import WeightTable
    shape, off = (5, 6, 3, 3), 16
    flat = torch.zeros(off + 5 * 6 * 9 + 8)
    p = ParamArena.view_of(flat, torch.empty(shape), off)
    assert tuple(p.shape) == shape
    p[:, 4] = 7.0
    arena = types.SimpleNamespace(flat=flat, total=flat.numel(), offset_of={id(p): off})
    s = WeightTable(arena, [("conv.weight", p)]).slots[0]
    assert (s.off, s.O, s.K, s.I) == (off, 5, 9, 6)
    idx = s.off + (torch.arange(s.O)[:, None, None] * s.K + torch.arange(s.K)[None, :, None]) * s.I + torch.arange(s.I)[None, None, :]
    got = flat[idx]  # [O][K][I]
    assert bool((got[:, :, 4] == 7.0).all()) and float(got.sum()) == 7.0 * 5 * 9 == float(flat.sum())


def test_weight_table_refuses_what_the_kernel_cannot_check():
    from vaehip.lib import VaeHipError, lib
    from vaehip.weight_table import WeightTable
    with pytest.raises(ValueError, match="overlaps"):
        WeightTable.from_entries([("a", 0, 4, 1, 8), ("b", 28, 2, 1, 4)], 64, "cpu")
    with pytest.raises(ValueError, match="beyond the buffers' 32 elements"):
        WeightTable.from_entries([("a", 4, 4, 1, 8)], 32, "cpu")
    with pytest.raises(ValueError, match="not on a multiple of 4"):
        WeightTable.from_entries([("a", 2, 4, 1, 8)], 64, "cpu")
    with pytest.raises(ValueError, match="empty shape"):
        WeightTable.from_entries([("a", 0, 0, 1, 8)], 64, "cpu")
    with pytest.raises(ValueError, match="no tensor"):
        WeightTable.from_entries([], 64, "cpu")
    arena, params = _fake_arena([(4, 4)])
    with pytest.raises(ValueError, match="does not live in the arena"):
        WeightTable(arena, [("x", torch.zeros(3))])
    t3 = torch.zeros(2, 2, 2)
    arena.offset_of[id(t3)] = 0
    with pytest.raises(ValueError, match="no conv weight"):
        WeightTable(arena, [("x", t3)])
    # the C side's own check of a host table
    import ctypes as C
    out = [C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)]
    refs = [C.byref(o) for o in out]
    good = torch.tensor([[0, 4, 1, 8, 0, 0, 0, 0], [32, 5, 1, 1, 4, 8, 8, 1]], dtype=torch.int64)
    lib.call("vae_wdyn_workspace", C.c_void_p(good.data_ptr()), 2, *refs)
    assert [o.value for o in out] == [2, 9, 8, 56]
    for row, col, val, msg in [(1, 0, 34, "multiple of 4"), (1, 0, -4, "negative"), (0, 1, 0, "bad shape"), (1, 4, 5, "running sums"),
                               (1, 5, 0, "running sums"), (1, 6, 0, "running sums"), (1, 7, 2, "running sums")]:
        bad = good.clone()
        bad[row, col] = val
        with pytest.raises(VaeHipError, match="wdyn_workspace.*" + msg):
            lib.call("vae_wdyn_workspace", C.c_void_p(bad.data_ptr()), 2, *refs)
    with pytest.raises(VaeHipError, match="wdyn_workspace.*nseg"):
        lib.call("vae_wdyn_workspace", C.c_void_p(good.data_ptr()), 0, *refs)
    with pytest.raises(VaeHipError, match="wdyn_workspace.*null"):
        lib.call("vae_wdyn_workspace", None, 2, *refs)


# ---------------------------------------------------------------------------------------------------- the bound itself
def _chain_sum(p: np.ndarray, n: int) -> float:
    """fp32 sum of the fp32 terms p in the longest sequential chains a tree of depth n admits: blocks of n - L terms added in
    order, the blocks combined pairwise in fp32 over L levels (plain sequential summation when they fit one chain)"""
    p = p.astype(np.float32).ravel()
    L = 0
    while math.ceil(p.size / max(1, n - L)) > 2 ** L:
        L += 1
    b = max(1, n - L)
    parts = []
    for i in range(0, p.size, b):
        s = np.float32(0.0)
        for x in p[i:i + b]:
            s = np.float32(s + x)
        parts.append(s)
    while len(parts) > 1:
        parts = [np.float32(parts[i] + parts[i + 1]) if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return float(parts[0])


def _fp32_terms(w, g, m, v, consts):
    f = np.float32
    bc1, bc2_sqrt, eps = (f(c) for c in consts)
    u = (m / bc1) / (np.sqrt(v) / bc2_sqrt + eps)  # float32 throughout: five correctly rounded operations
    assert u.dtype == np.float32
    return [w * w, g * g, w * g, m * m, g * m, u * u]


@pytest.mark.parametrize("O,K,I", SHAPES)
def test_bound_holds_for_the_longest_chains_it_admits(O, K, I):
    consts = _consts()
    w, g, m, v = R.draw((O, K, I), 100 + O * 7 + K * 3 + I)
    assert (w < 0).any() or w.size < 4
    assert (v > 0).all() and np.log2(v.max() / v.min()) >= (3 if v.size >= 8 else 0)
    r = R.ref(w, g, m, v, consts)
    bd = R.bounds(r, O, K, I, 32768)
    n_out, n_in = R.chains(O, K, I, 32768)
    terms = _fp32_terms(w, g, m, v, consts)
    for view, n, slices in (("out", n_out, [(o, slice(None), slice(None)) for o in range(O)]),
                            ("in", n_in, [(slice(None), slice(None), i) for i in range(I)] if I > 1 else [])):
        for idx, sl in enumerate(slices[:16]):
            for j, t in enumerate(terms):
                got = _chain_sum(t[sl], n)
                assert abs(got - r[view]["sums"][idx, j]) <= bd[view][idx, j], (view, idx, R.SUMS[j])


@pytest.mark.parametrize("O,K,I", [(1, 1, 1), (3, 1, 7), (8, 9, 64), (130, 1, 4)])
def test_one_dropped_or_doubled_element_is_outside_the_bound(O, K, I):
    consts = _consts()
    w, g, m, v = R.draw((O, K, I), 200 + O + K + I)
    r = R.ref(w, g, m, v, consts)
    bd = R.bounds(r, O, K, I, 32768)
    t64 = [t.astype(np.float64) for t in _fp32_terms(w, g, m, v, consts)]
    o, i = O - 1, I // 2
    for j in (0, 1, 3, 5):  # the sums of squares.  Dropped: the sum moves by -term, doubled: by +term
        # the slice's median term: draw() spreads the terms over some twenty binades (u^2 = m^2 / v over more), so the smallest
        # term of a slice can lie below any bound that is relative to the slice's sum; a typical one must not
        for view, idx, sl in (("out", o, t64[j][o]), ("in", i, t64[j][:, :, i])) if I > 1 else (("out", o, t64[j][o]),):
            term = np.sort(sl.ravel())[sl.size // 2]
            assert term > bd[view][idx, j], (view, R.SUMS[j], term, bd[view][idx, j])
    for j in (2, 4):  # the signed sums: the largest term of the slice
        k2, i2 = np.unravel_index(np.abs(t64[j][o]).argmax(), (K, I))
        assert abs(t64[j][o, k2, i2]) > bd["out"][o, j]


def test_chain_lengths_of_the_model_shapes():
    """the chains the bound is built from, spelled out for shapes the model holds"""
    assert R.chains(512, 1, 1, 32768) == (1, None)
    assert R.chains(512, 9, 512, 32768) == (5 * 4 + 6 + 1 + 2, 7 * 5 + 2)        # 128 units: 2 thread rows, 7 rows per chunk
    assert R.chains(128, 9, 3, 32768) == (1 + 6 + 1 + 2, 8 * 1 + 85)             # scalar: 3 lanes, 85 thread rows, 8 rows per chunk
    assert R.chains(2, 1, 32772, 32768) == (4 + 6 + 33 + 2, 1 + 1)               # a row longer than the chunk: 33 column tiles
