"""Kernel selection pinned on the host: every pure dispatch query of libvaehip (kernel names, epilogue chunk counts, split
plans, capability answers) over the case grid of tests/golden/make_dispatch_table.py must give what the committed table
records.  Fake pointers, no launch: runs without a GPU."""
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_dispatch_table as mdt  # noqa: E402

FAMILIES = ["conv3_upwino", "conv3_wino4", "conv3_wino", "conv3_wide_bf16<*,2>", "conv3_wide_bf16<*,3>", "conv3_tile_bf16",
            "conv3_tile", "conv_thin_bf16", "conv_smallk", "conv_thinn_bf16", "conv_smalln", "conv1_bf16", "igemm_rows_bf16",
            "igemm_rows", "wgrad3_dma_bf16", "wgrad3_tile_bf16", "wgrad3_tile", "wgrad_thin_bf16", "wgrad_smallk", "wgrad_bf16",
            "wgrad"]


def _family(name):
    m = re.match(r"(\w+?)_kernel(<.*>)?$", name)
    assert m, name
    fam = m.group(1)
    if fam == "conv3_wide_bf16":
        fam += "<*," + m.group(2).rstrip(">").split(",")[-1] + ">"
    return fam


def test_dispatch_table_matches_golden():
    with open(os.path.join(HERE, "golden", "dispatch_table.json")) as f:
        golden = json.load(f)
    got = mdt.build_table()
    assert sorted(got) == sorted(golden), "the case grid changed: regenerate tests/golden/dispatch_table.json on purpose"
    diff = [k for k in sorted(golden) if got[k] != golden[k]]
    assert not diff, f"{len(diff)} cases differ, e.g. " + "; ".join(f"{k}: {got[k]} != {golden[k]}" for k in diff[:5])
    assert json.loads(mdt.dumps(got)) == golden

    # coverage: the grid cannot shrink silently
    names = [v[0] for k, v in golden.items() if not k.startswith("geom|")]
    seen = {_family(n) for n in names}
    missing = [f for f in FAMILIES if f not in seen]
    assert not missing, missing
    positions = {v[5] for k, v in golden.items() if k.startswith(("wgrad|", "wphase|", "gemm_tn"))}
    assert {9, 16} <= positions
    opts = {o for k in golden for o in k.rsplit("|", 1)[1].split(",") if o}
    assert opts == set(mdt.OPTIONS)
    # the stride-2 bf16 weight gradient under no_wgrad_dma
    assert any(k.startswith("wgrad|c3s2") and k.endswith("|no_wgrad_dma") and "dma" not in v[0] for k, v in golden.items())
    assert any(k.startswith("wgrad|c3s2") and "dma" in v[0] for k, v in golden.items())
    assert {1} <= {v[0] for k, v in golden.items() if k.startswith("geom|")}
    assert len(golden) > 1000


def test_image_queries_answer_for_the_blocks_ops_launches():
    """vae_bf16_act_image_ok / vae_bf16_grad_image_ok build their forward, dgrad and weight-gradient blocks by hand in
    csrc/dispatch.cpp; over EVERY geometry of the grid they must say what the dispatcher selects for the blocks ops.py
    launches there (bf16 arithmetic, the weights' image present)"""
    from vaehip import ops
    from vaehip.lib import lib
    dll = lib.load()
    n = act_yes = grad_yes = 0
    for kind, Ci, Co, div in mdt.LAYERS:
        for R in mdt.SIZES:
            for B in mdt.BATCHES:
                H = W = R // div
                fwd = mdt._copy(mdt.conv_ptrs(ops.fwd_args(kind, B, H, W, Ci, Co, Ci, prec=mdt.BF16)), Wh=mdt.P)
                dgrad = mdt._copy(mdt.conv_ptrs(ops.dgrad_args(kind, B, H, W, Co, Ci, prec=mdt.BF16)), Wh=mdt.P)
                wgrad = mdt.wgrad_ptrs(ops.wgrad_args(kind, B, H, W, Ci, Co, Ci, prec=mdt.BF16))
                tiles = kind == "c3" and Ci % 8 == 0 and ops._kernel_name("vae_wgrad_kernel_name", wgrad).startswith("wgrad3_tile_bf16_kernel")
                act = tiles and ops._kernel_name("vae_igemm_kernel_name", fwd).startswith("conv3_tile_bf16_kernel")
                grad = tiles and Co % 8 == 0 and ops._kernel_name("vae_igemm_kernel_name", dgrad).startswith("conv3_tile_bf16_kernel")
                g = ops._fwd_geom(kind, B, H, W, Ci)
                case = (kind, Ci, Co, H, W, B)
                assert bool(dll.vae_bf16_act_image_ok(C.byref(g), Co, Ci)) == act, case
                assert bool(dll.vae_bf16_grad_image_ok(C.byref(g), Co, Ci)) == grad, case
                n, act_yes, grad_yes = n + 1, act_yes + act, grad_yes + grad
    assert n == len(mdt.LAYERS) * len(mdt.SIZES) * len(mdt.BATCHES)
    assert min(act_yes, n - act_yes, grad_yes, n - grad_yes) >= 100, (n, act_yes, grad_yes)  # both answers occur: no pass by vacuity
