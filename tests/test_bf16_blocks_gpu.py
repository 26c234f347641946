"""Each block of the bf16 step against a float64 reference that rounds where the engine rounds (tests/bf16_refs.py).

The engine's own block (modules of SDXLVAEWrapper("synthetic:5") with gamma / beta / q / k given some contrast) runs under
set_precision("bf16") and _mode() with a tape, forward and run_tape, while every ops-level call it makes is recorded with the
tensors that come out (br.OpsRecorder: no forward hooks, the route is not changed).  Then

  a. stage by stage: the reference recomputes every recorded result in float64 from the engine's stored values of the tensors
     that the REFERENCE's wiring says feed it ("teacher forcing").  A stage fed by the wrong tensor, a stale image or an unrounded
     operand disagrees; rounding flips upstream do not blur the stages after them.  The sequence of calls must be the reference's;
  b. the block as a whole: its output, its input gradient and every parameter gradient (arena.grad_view) are the last stage that
     produces each, bit for bit, and meet the same criterion;
  c. the route: the kernel names ops.LaunchProfiler records are the ones the case pins.

Criterion (br.ratio <= 1, no element left out): fp32 result max |got - v| <= bar max|v|; bf16 result, every element,
|got - v| <= ulp_bf16(v) / 2 + bar max|v|; an attached image bit-equal to r16 of its tensor.  Bars: the serving kernel family's
existing ones (bf16_refs.py).  Where a kernel applies GroupNorm + SiLU while it stages x, or sums an upsampler's taps, the rounded
operand is the device's own (gn_apply_bf16 / upconv_phase_weights on the stored values), itself held to float64 as a stage.

Measured worst ratios per case and stage, and the reference's time, are recorded with the suite's other measured figures
(test_engine_gpu._record, kind "bf16_blocks"); profiles/bf16_blocks_measured.json is that record of a run on MI355X."""
import time

import pytest
import torch

import bf16_refs as br

pytestmark = pytest.mark.gpu
_RUNS = {}


class _Device:
    """the device's own transform / tap sums on stored values, for the operands no recorded call produces"""

    def __init__(self, dev, ops):
        self.dev, self.ops = dev, ops

    def gn_apply_bf16(self, x, st, xf):
        s = self.ops.Stats(None, None, st.scale.to(self.dev), st.shift.to(self.dev))
        return self.ops.gn_apply_bf16(x.to(self.dev).contiguous(), s, xf).cpu()

    def upconv_phase_weights(self, w):
        wv = w.to(self.dev).permute(0, 2, 3, 1).contiguous()          # OHWI memory
        return self.ops.upconv_phase_weights(wv).permute(0, 1, 4, 2, 3).contiguous().cpu()  # -> [4, Co, Ci, 3, 3]


@pytest.fixture(scope="module")
def vae(cuda):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    w = SDXLVAEWrapper("synthetic:5")
    w.to(cuda)
    restore = br.contrast(w.vae)
    w.vae.engine.set_precision("bf16")
    yield w.vae
    w.vae.engine.set_precision("no")
    restore()


def _run(case, vae, dev):
    """one engine run and one reference evaluation per case, shared by the tests of the case"""
    if case.id in _RUNS:
        return _RUNS[case.id]
    from vaehip import ops
    eng, arena = vae.engine, vae.arena
    P, named = br.params_of(case, vae)
    x_pre, x, dout = br.inputs_of(case, vae, ops)
    cfg = br.cfg_of(case, vae, ops)
    gbuf = torch.zeros_like(arena.grad)
    keep = ops.ACT_BF16
    ops.ACT_BF16 = case.act16
    prof = ops.PROFILER = ops.LaunchProfiler()
    calls0 = dict(ops.ATTN_CALLS)
    try:
        with eng._mode():
            with br.OpsRecorder(ops) as rec:
                out, dx = br.run_engine_block(case, vae, ops, x.to(dev), dout.to(dev), gbuf)
    finally:
        ops.PROFILER = None
        ops.ACT_BF16 = keep
    torch.cuda.synchronize()
    names = tuple(r[0] for r in prof.records if r[1] > 0 and not r[0].startswith("attn_"))
    attn = tuple(r[0] for r in prof.records if r[0].startswith("attn_")) + tuple(ops.ATTN_CALLS[k] - calls0[k] for k in sorted(calls0))
    got = {"out": out.cpu(), "dx": None if dx is None else dx.cpu()}
    got.update({n: arena.grad_view(p, gbuf).detach().cpu() for n, p in named.items()})
    t0 = time.perf_counter()
    E = br.Ev(forced=rec.record(), device=_Device(dev, ops))
    fin = br.reference(E, case, cfg, P, x_pre, x, dout)
    r = _RUNS[case.id] = {"names": names, "attn": attn, "stages": E.stages, "fin": fin, "got": got, "seconds": time.perf_counter() - t0,
                          "ratios": br.worst(E.stages)}
    return r


IDS = [c.id for c in br.CASES]


@pytest.mark.parametrize("case", br.CASES, ids=IDS)
def test_every_stage_meets_its_reference(case, vae, cuda):
    r = _run(case, vae, cuda)
    for k, v in r["ratios"].items():
        print(f"{case.id:32s} {k:28s} {v:.4f}")
    print(f"{case.id}: reference {r['seconds']:.2f} s")
    over = {k: v for k, v in r["ratios"].items() if not v <= 1.0}
    assert not over, (case.id, over)


@pytest.mark.parametrize("case", br.CASES, ids=IDS)
def test_block_results_are_the_last_stages(case, vae, cuda):
    r = _run(case, vae, cuda)
    by = {s.name: s for s in r["stages"]}
    assert ("dx" in r["fin"]) == (r["got"]["dx"] is not None), (case.id, "the input gradient is returned exactly when it is wanted")
    block = r.setdefault("block", {})
    for name, sname in r["fin"].items():
        s, g = by[sname], r["got"][name]
        assert g.dtype == s.got.dtype and torch.equal(g, s.got), (case.id, name, "is not what the stage", sname, "produced")
        block[name] = br.ratio(s._replace(got=g))
    over = {k: v for k, v in block.items() if not v <= 1.0}
    assert not over, (case.id, over)
    # every parameter of the block got its gradient from a stage
    assert set(r["got"]) - {"out", "dx"} <= set(r["fin"]), set(r["got"]) - set(r["fin"])


@pytest.mark.parametrize("case", br.CASES, ids=IDS)
def test_route_is_the_arm_the_case_is_for(case, vae, cuda):
    r = _run(case, vae, cuda)
    assert r["names"] == case.names, (case.id, r["names"])
    if case.block == "attn":   # ops.ATTN_CALLS: (blockwise_bwd, blockwise_fwd, materialised_fwd) of this run
        want = ("attn_fwd_kernel<bf16>", "attn_bwd_kernels<bf16>", 1, 1, 0) if "blockwise" in case.id else (0, 0, 1)
        assert r["attn"] == want, (case.id, r["attn"])


def test_zz_measured_figures_are_kept(vae, cuda):
    """(runs last in the module: records what the tests above measured; on its own it measures every case first)"""
    from test_engine_gpu import _record
    doc = {}
    for c in br.CASES:
        r = _run(c, vae, cuda)
        doc[c.id] = {"arm": c.arm, "storage": "bf16" if c.act16 else "fp32 + images", "reference_seconds": round(r["seconds"], 3),
                     "worst_ratio_to_allowed": max(r["ratios"].values()), "stages": r["ratios"],
                     "share_of_bar_used": {s.name: br.bar_used(s) for s in r["stages"]}}
        _record("bf16_blocks", c.id, doc[c.id])
    assert len(doc) == len(br.CASES)
