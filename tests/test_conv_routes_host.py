"""The conv-route cases of tests/conv_routes.py without a GPU: the line tracer and the statement set on a toy function, and
every case's route (kernel names, helper entry points, recursions, storage of the result) from a dry run in which the real
library answers every dispatch query and nothing is launched.  A change of csrc/dispatch.cpp that re-routes a case fails here,
so it cannot hollow out tests/test_conv_routes_gpu.py."""
import ctypes as C
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import conv_routes as cr  # noqa: E402
import make_dispatch_table as mdt  # noqa: E402


def _toy(a, b):
    """a docstring is no statement"""
    if a:
        x = 1
    else:
        x = 2
    if b < 0:
        raise ValueError(b)
    for _ in range(b):
        x += (1 if a
              else 2)
    return x


def test_tracer_and_statement_set_on_a_toy_function():
    stm = cr.statements(_toy)
    assert sorted(stm.values()) == sorted(["if a:", "x = 1", "x = 2", "if b < 0:", "for _ in range(b):", "x += (1 if a", "return x"])
    prev = sys.gettrace()
    seen = set()
    with cr.LineTracer({_toy.__code__}, seen):
        assert _toy(True, 0) == 1
    assert sys.gettrace() is prev
    assert cr.missed([_toy], seen) == ["x = 2", "x += (1 if a"]       # the missed branch and the empty loop's body are reported
    with cr.LineTracer({_toy.__code__}, seen):
        assert _toy(False, 2) == 6
    assert cr.missed([_toy], seen) == []                              # ... and covered ones are not
    other = set()
    with cr.LineTracer({_toy.__code__}, other):                       # only the given code objects are traced
        cr.statements(_toy)
    assert other == set()


def test_allowed_statements_still_occur_in_the_source():
    from vaehip import ops
    assert len(cr.ALLOWED) <= 5
    texts = set()
    for n in cr.TRACED:
        texts.update(cr.statements(getattr(ops, n)).values())
    assert set(cr.ALLOWED) <= texts, set(cr.ALLOWED) - texts


def test_case_ids_are_unique_and_every_issue_shape_is_used():
    ids = [c.id for c in cr.CASES]
    assert len(ids) == len(set(ids))
    shapes = {c.shape for c in cr.CASES}
    assert {cr.HALO, cr.WINO4, cr.RAGGED, cr.UNVEC, cr.UNFUS, cr.WIDE} <= shapes


SEEN = set()


@pytest.mark.parametrize("case", cr.CASES, ids=[c.id for c in cr.CASES])
def test_case_takes_the_route_its_label_claims(case):
    """dry run: the library's answers (vae_conv_io16_ok, vae_wgrad_io16_ok, vae_xf_fusable_rows, vae_wgrad_plan,
    vae_conv_phase_ok, vae_wgrad_phase_ok, the kernel names, ...) send the call down the pinned route"""
    from vaehip import ops
    lines = set()
    with cr.LineTracer(cr.traced_codes(ops), lines):
        r = cr.run(case, dev="cpu", dry=True)
    cr.check_route(case, r)
    if not case.raises:  # (a refused call compares no value: its lines do not count, as in the GPU module)
        SEEN.update(lines)
    if case.raises:  # no Winograd kernel (those take no storage check) and no fp32-copy recursion in front of the refusal
        assert case.mode == "f32" and r["route"].entries == 1 and not any("wino" in n for n in r["route"].names), r["route"].names


def test_the_dry_runs_execute_every_statement_too():
    """the same statement coverage as the GPU module's last test, from the dry runs: an arm that lost its case shows here first"""
    from vaehip import ops
    never = cr.missed([getattr(ops, n) for n in cr.TRACED], SEEN)
    assert set(never) <= set(cr.ALLOWED), never


def test_required_arms_have_their_cases():
    by = {c.id: c for c in cr.CASES}
    # conv_fwd's fp32-copy recursion, once per trigger; a re-stored result carries no statistics
    for t in ("track", "xf16", "unvec", "smallk"):
        c = by[f"fwd-rec-{t}-gstat"]
        assert c.entries == 2 and c.helpers == ("vae_unpack_bf16", "vae_pack_bf16") and c.dtype == "bf16" and c.attr is False, c
    for t in ("track", "xf16", "unvec"):
        assert by[f"fwd-rec-{t}-res32"].entries == 2 and by[f"fwd-rec-{t}-res16"].entries == 2
    # (the small-k trigger has no with-residual form: the small-k kernel takes no residual, so the bf16 flat kernel serves the
    # layer and takes every storage)
    for v in ("res32", "res16", "out32"):
        assert by[f"fwd-smallk-{v}"].entries == 1 and by[f"fwd-smallk-{v}"].names == ("igemm_rows_bf16_kernel",)
    assert by["fwd-rec-track-a16"].entries == 2
    # an unfusable transform is materialised exactly once, in both modes, forward and weight gradient
    for m in ("f32", "bf16", "act16"):
        assert by[f"fwd-unfus-4x4-{m}"].helpers.count("vae_gn_apply") == 1
        assert by[f"wgrad-unfus-unvec-{m}"].helpers.count("vae_gn_apply") == 1
    # the arm of the bug fixed in 65b1982: materialised once, then redone on fp32 copies
    c = by["wgrad-fixedbug"]
    assert c.entries == 2 and c.helpers.count("vae_gn_apply") == 1 and c.names == ("wgrad_kernel",)
    c = by["wgrad-io16-xf"]
    assert c.entries == 2 and "vae_gn_apply" not in c.helpers
    # all three forms of _reduce_splits, and none
    forms = {tuple(sorted(set(c.helpers) & {"vae_reduce_splits", "vae_reduce_splits2"})) for c in cr.CASES if c.op == "wgrad" and not c.raises}
    assert forms >= {(), ("vae_reduce_splits",), ("vae_reduce_splits2",)}
    assert by["wgrad-halo-bf16-nobias"].helpers == ("vae_reduce_splits",) and by["wgrad-halo-nowino"].helpers == ("vae_reduce_splits",)
    # the upsampler: phases with an image only on the wide kernel, the virtual-upsample kernel below it
    assert by["fwd-up-phase-wide16"].names == ("conv3_wide_bf16_kernel",) * 4 and by["fwd-up-below16"].names == ("conv3_tile_bf16_kernel",)
    assert by["fwd-up-below16-7"].names == ("conv3_tile_bf16_kernel",)
    assert by["dgrad-up-phase-wide16"].names == ("conv3_wide_bf16_kernel",) * 4
    assert "vae_sumpool2x2" in by["dgrad-up-below16"].helpers and "vae_sumpool2x2" in by["dgrad-up-ragged-f32"].helpers
    # the phases' `xb or dy is None -> False` with a valued route behind it: bf16 tensors that are no images (Co % 8 != 0)
    c = by["wgrad-up-co132"]
    assert c.entries == 2 and c.names == ("wgrad3_tile_bf16_kernel",) * 4 and c.helpers[:2] == ("vae_unpack_bf16",) * 2 and not c.raises
    assert sum(c.raises for c in cr.CASES if c.op == "fwd") >= 1 and sum(c.raises for c in cr.CASES if c.op == "dgrad") >= 1
    assert sum(c.raises for c in cr.CASES if c.op == "wgrad") >= 1


def test_a_phase_with_an_operand_image_runs_on_the_wide_kernel_which_writes_either_storage():
    """why _upconv_phase_fwd does not ask vae_conv_io16_ok: with an image (A16), vae_conv_phase_ok accepts only launches the
    wide-tile kernel serves, and that kernel takes the output as fp32 or bf16 -- over a grid of upsampler geometries"""
    from vaehip import ops
    from vaehip.lib import lib
    dll = lib.load()
    accepted = 0
    for B in (1, 2, 7, 13, 16):
        for H, W in ((4, 32), (8, 32), (8, 64), (32, 64), (64, 64), (12, 96)):
            for Ci, Co in ((128, 128), (128, 256), (256, 256), (512, 512), (64, 32)):
                for pa in (0, 1):
                    for pb in (0, 1):
                        for out16 in (0, 1):
                            a = mdt._copy(mdt.conv_ptrs(ops.phase_args(B, H, W, Co, Ci, False, prec=ops.PREC_BF16)),
                                          tapmask=ops._phase_tapmask(pa, pb), Wh=mdt.P, A16=mdt.P, out_bf16=out16)
                            if dll.vae_conv_phase_ok(C.byref(a)):
                                accepted += 1
                                assert dll.vae_conv_io16_ok(C.byref(a)) == 1, (B, H, W, Ci, Co, out16)
                                assert ops._kernel_name("vae_igemm_kernel_name", a).startswith("conv3_wide_bf16_kernel"), (B, H, W, Ci, Co)
    assert accepted >= 100
