"""A/B of two (or more) builds of the fp32 Winograd convolutions in one process: this build against the parent commit's
libvaehip.so (built in a scratch worktree; nothing of it is committed), further builds optional (a lever of
one kernel switched the other way, e.g. conv3_wino4.hip compiled with -DVAE_W4_SWAVE=0 and linked into another file).

Per case the operands are filled once; every library builds its own transformed weights (vae_wino_weights) and launches
vae_igemm_rows into its own output, `gstat` workspace and `gnb` workspace, which start as NaN and are compared with the FIRST
library's BIT FOR BIT, as is the transformed-weight image U itself.  Then the arms are timed alternately with device events
around the convolution launch alone (warm-up, `--launches` launches per arm, interleaved launch by launch, the arm that opens a
round rotating): median, quartiles and extremes per arm.

Cases: F(4x4) forward and dgrad of the plain 3x3 layers of the fp32 step (256^2, batch 16), each bare and with the epilogue it
runs with in the step (forward: bias + residual + GroupNorm moments; dgrad: GroupNorm(+SiLU)-backward sums); the small cases
of tests/test_wino4_seat_gpu.py (bitwise only); the upsampler convolutions (csrc/conv3_upwino.hip forward and dgrad,
csrc/wgrad3_upwino.hip through vae_wgrad_wino); the small forwards also with GroupNorm + SiLU fused into the staging (epilogue
"xf": XF_AFFINE_SILU + bias + residual + moments).  `--only wino2` runs the small cases and the F(2x2)-only shapes of the kernel
tests under the library option no_wino4 (set on every library), so that csrc/conv3_wino.hip serves them.

With a third library named parent2 (a second copy of the parent's file) the run derives its own noise floor: per kernel the margin
is twice the largest |median(parent2) / median(parent) - 1| over that kernel's timed cases, and `within_margin` says whether
the new build's median stays inside it on every case (exit status 2 if not; 1 if anything differs in a bit).

usage: python tools/wino_seat_ab.py NEW.so PARENT.so [name=OTHER.so ...] [--launches 20] [--out FILE] [--only wino4|wino2|up]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import IgemmArgs, WgradArgs, lib  # noqa: E402

# kind, mode, B, H, W, Ci, Co, epilogue, timed      (H, W: the layer's forward input map)
STEP = [("c3", m, 16, hw, hw, ci, co, e, True) for ci, co, hw in [(128, 128, 256), (256, 128, 256), (256, 256, 128), (512, 256, 128), (512, 512, 64), (512, 512, 32)]
        for m in ("fwd", "dgrad") for e in (False, True)]
SMALL = ([("c3", "fwd", B, H, W, K, Co, False, False) for K in (64, 72, 80, 136) for B, H, W, Co in [(1, 16, 32, 64), (2, 32, 64, 128)]]
         + [("c3", "dgrad", B, H, W, 64, K, False, False) for K in (64, 72, 80, 136) for B, H, W in [(1, 16, 32), (2, 32, 64)]]
         + [("c3", "fwd", 1, 48, 96, 72, 64, False, False), ("c3", "dgrad", 1, 48, 96, 64, 72, False, False),
            ("c3", "fwd", 2, 32, 64, 128, 128, True, False), ("c3", "dgrad", 2, 16, 32, 128, 64, True, False),
            ("c3", "fwd", 2, 32, 64, 128, 128, "xf", False), ("c3", "fwd", 1, 16, 32, 72, 128, "xf", False)])
# under no_wino4: the small cases and the shapes only F(2x2) takes (partial 16 x 32 tiles, channel tails of 32 and 160)
WINO2 = SMALL + [("c3", m, B, H, W, Ci, Co, e, False) for B, H, W, Ci, Co in [(6, 16, 48, 128, 160), (2, 8, 16, 128, 32), (1, 48, 32, 256, 64)]
                 for m, e in (("fwd", False), ("dgrad", False), ("fwd", "xf")) if not (m == "dgrad" and Co < 64)]  # (K >= 64)
# ... and, timed, two layers of the step with the epilogues F(2x2) runs with (moments; GroupNorm-backward sums; fused GroupNorm + SiLU)
WINO2 += [("c3", m, 16, hw, hw, ci, co, e, True) for ci, co, hw in [(128, 128, 256), (512, 512, 64)]
          for m, e in (("fwd", True), ("dgrad", True), ("fwd", "xf"))]
UP = [("c3up", m, 16, hw, hw, ci, co, False, True) for ci, co, hw in [(512, 512, 32), (512, 512, 64), (256, 256, 128)] for m in ("fwd", "dgrad", "wgrad")]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    ia, wa, vp = C.POINTER(IgemmArgs), C.POINTER(WgradArgs), C.c_void_p
    for fn, res, argt in (("vae_igemm_rows", C.c_int, [ia, vp]), ("vae_wino_ok", C.c_int, [ia]), ("vae_wino_weight_floats", C.c_int64, [ia]),
                          ("vae_wino_weights", C.c_int, [ia, vp, vp]), ("vae_conv_gstat_chunks", C.c_int, [ia]), ("vae_conv_gnb_chunks", C.c_int, [ia]),
                          ("vae_igemm_kernel_name", C.c_int, [ia, C.c_char_p, C.c_int32]), ("vae_wgrad_wino", C.c_int, [wa, vp]),
                          ("vae_wgrad_wino_plan", C.c_int, [wa, C.POINTER(C.c_int32)]), ("vae_wgrad_wino_positions", C.c_int, [wa]),
                          ("vae_set_option", C.c_int, [C.c_char_p, C.c_int32])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = res, argt
    return dll


def _bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


class Case:
    """operands of one case, filled once; arm(dll) -> (launch function, outputs of that arm)"""

    def __init__(self, dev, kind, mode, B, H, W, Ci, Co, epi):
        self.dev, self.kind, self.mode, self.epi = dev, kind, mode, epi
        self.dims = (B, H, W, Ci, Co)
        g = torch.Generator(device=dev).manual_seed(7 + Ci + 3 * Co + H + B + (mode != "fwd"))
        Hy, Wy = ops.out_hw(kind, H, W)
        self.w = torch.randn((Co, 3, 3, Ci), device=dev, generator=g) / math.sqrt(9 * Ci)
        self.x = torch.randn((B, H, W, Ci), device=dev, generator=g) * 1.3 + 0.2
        self.dy = torch.randn((B, Hy, Wy, Co), device=dev, generator=g) if mode != "fwd" else None
        self.bias = torch.randn((Co,), device=dev, generator=g)
        self.res = torch.randn((B, Hy, Wy, Co), device=dev, generator=g) if (epi and mode == "fwd") else None
        if epi == "xf":
            self.scale, self.shift = torch.rand((B, Ci), device=dev, generator=g) + 0.5, torch.randn((B, Ci), device=dev, generator=g)
        if epi and mode == "dgrad":
            self.mean, self.rstd = torch.randn((B, 32), device=dev, generator=g) * 0.1, torch.rand((B, 32), device=dev, generator=g) + 0.5
            self.gamma, self.beta = 1 + 0.3 * torch.randn((Ci,), device=dev, generator=g), 0.2 * torch.randn((Ci,), device=dev, generator=g)
        if mode != "fwd":
            self.x = self.x if (mode == "wgrad" or (epi and mode == "dgrad")) else None

    def arm(self, dll, st):
        B, H, W, Ci, Co = self.dims
        dev, nan = self.dev, float("nan")
        if self.mode == "wgrad":
            a = ops.wgrad_args(self.kind, B, H, W, Ci, Co, Ci, prec=ops.PREC_F32)
            a.dY, a.X = _p(self.dy), _p(self.x)
            n = C.c_int32(0)
            assert dll.vae_wgrad_wino_plan(C.byref(a), C.byref(n)) == 0 and n.value > 0, "no Winograd weight gradient for this case"
            npos = dll.vae_wgrad_wino_positions(C.byref(a))
            slab, bpart = torch.full((n.value, npos * Ci * Co), nan, device=dev), torch.full((n.value, Co), nan, device=dev)
            a.nsplit, a.partial, a.bias_partial = n.value, _p(slab), _p(bpart)
            self.kernel = "wgrad3_upwino_kernel" if npos == 9 else "wgrad3_wino_kernel<0>"

            def launch():
                rc = dll.vae_wgrad_wino(C.byref(a), st)
                assert rc == 0, rc
            return launch, {"slab": slab, "bias_partial": bpart}, (a,)
        if self.mode == "fwd":
            a = ops.fwd_args(self.kind, B, H, W, Ci, Co, Ci, xf=ops.XF_AFFINE_SILU if self.epi == "xf" else ops.XF_NONE, prec=ops.PREC_F32)
            src, oshape = self.x, (B, *ops.out_hw(self.kind, H, W), Co)
            a.bias, a.res = _p(self.bias), _p(self.res)
            if self.epi == "xf":
                a.scale, a.shift = _p(self.scale), _p(self.shift)
        else:
            a = ops.up2x_dgrad_args(B, H, W, Co, Ci, prec=ops.PREC_F32) if self.kind == "c3up" else ops.dgrad_args(self.kind, B, H, W, Co, Ci, prec=ops.PREC_F32)
            src, oshape = self.dy, (B, H, W, Ci)
        out = torch.full(oshape, nan, device=dev)
        a.A, a.W, a.C = _p(src), _p(self.w), _p(out)
        assert dll.vae_wino_ok(C.byref(a)), "no Winograd kernel for this case"
        wu = torch.full((int(dll.vae_wino_weight_floats(C.byref(a))),), nan, device=dev)
        assert dll.vae_wino_weights(C.byref(a), _p(wu), st) == 0
        outs = {"out": out, "U": wu}
        a.Wu = _p(wu)  # (the epilogue queries below are about the kernel the transformed weights select)
        if self.epi and self.mode == "fwd":
            a.gstat_groups = 32
            nch = dll.vae_conv_gstat_chunks(C.byref(a))
            assert nch > 0 or self.epi == "xf"  # (the F(2x2)-only channel counts have no moments epilogue: 5, 1, 2 channels per group)
            if nch > 0:
                outs["gstat"] = torch.full((B, nch, 32, 2), nan, device=dev)
                a.gstat = _p(outs["gstat"])
            else:
                a.gstat_groups = 0
        if self.epi and self.mode == "dgrad":
            a.gnb_x, a.gnb_mean, a.gnb_rstd, a.gnb_gamma, a.gnb_beta = _p(self.x), _p(self.mean), _p(self.rstd), _p(self.gamma), _p(self.beta)
            a.gnb_groups, a.gnb_silu = 32, 1
            nch = dll.vae_conv_gnb_chunks(C.byref(a))
            assert nch > 0
            outs["gnb"] = torch.full((B, nch, Ci, 2), nan, device=dev)
            a.gnb_ws = _p(outs["gnb"])
        buf = C.create_string_buffer(128)
        dll.vae_igemm_kernel_name(C.byref(a), buf, 128)
        self.kernel = buf.value.decode()

        def launch():
            rc = dll.vae_igemm_rows(C.byref(a), st)
            assert rc == 0, rc
        return launch, outs, (a, wu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NEW.so PARENT.so [name=OTHER.so ...]")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "wino4", "wino2", "up"])
    arg = ap.parse_args()
    assert len(arg.libs) >= 2, "two libraries: this build and the parent's"
    names = ["new", "parent"] + [s.split("=", 1)[0] for s in arg.libs[2:]]
    dlls = [_open(s.split("=", 1)[-1]) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = WINO2 if arg.only == "wino2" else (STEP + SMALL if arg.only != "up" else []) + (UP if arg.only != "wino4" else [])
    for d in dlls:  # (an option of the library, so of every copy)
        d.vae_set_option(b"no_wino4", 1 if arg.only == "wino2" else 0)
    rows, all_equal = [], True
    for kind, mode, B, H, W, Ci, Co, epi, timed in cases:
        c = Case(dev, kind, mode, B, H, W, Ci, Co, epi)
        first, eq, launches, keep = None, {}, [], []
        for i, d in enumerate(dlls):  # one arm's outputs at a time beside the first's
            launch, outs, alive = c.arm(d, st)
            launch()
            torch.cuda.synchronize()
            if i == 0:
                first = outs
                finite = all(bool(torch.isfinite(t).all()) for t in outs.values())
            else:
                eq[names[i]] = all(_bits(outs[k], first[k]) for k in first)
            launches.append(launch)
            keep.append((alive, outs) if timed else None)  # (the timed launches keep writing their outputs)
            if i and not timed:
                del outs
        all_equal = all_equal and all(eq.values()) and finite
        row = {"kernel": c.kernel, "mode": mode, "B": B, "H": H, "W": W, "Cin": Ci, "Cout": Co, "epilogue": epi, "compared": sorted(first),
               "bitwise_equal_to_new": eq, "bitwise": all(eq.values()), "finite": finite}
        if timed:
            for _ in range(3):
                for launch in launches:
                    launch()
            ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(arg.launches)] for _ in dlls]
            for k in range(arg.launches):
                for i in ((k + j) % len(launches) for j in range(len(launches))):  # (every arm takes every place in the round equally often)
                    ev[i][k][0].record()
                    launches[i]()
                    ev[i][k][1].record()
            torch.cuda.synchronize()
            for i, nm in enumerate(names):
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[i])
                q = statistics.quantiles(ms, n=4)
                row[nm] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4),
                           "max_ms": round(ms[-1], 4)}
            for nm in names:
                if nm != "parent":
                    row[f"{nm}_over_parent"] = round(row[nm]["median_ms"] / row["parent"]["median_ms"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del c, first, launches, keep
        torch.cuda.empty_cache()
    res = {"libs": dict(zip(names, [os.path.basename(s.split("=", 1)[-1]) for s in arg.libs])), "launches_per_arm": arg.launches,
           "all_bitwise_equal": all_equal, "rows": rows}
    if "parent2" in names and any("parent" in r for r in rows):  # the run's own floor: what two copies of one file differ by, doubled
        floor = {}
        for r in rows:
            if "parent" in r:
                floor[r["kernel"]] = max(floor.get(r["kernel"], 0.0), abs(r["parent2"]["median_ms"] / r["parent"]["median_ms"] - 1))
        res["margin"] = {k: round(2 * v, 4) for k, v in floor.items()}
        for r in rows:
            if "parent" in r:
                r["within_margin"] = r["new"]["median_ms"] / r["parent"]["median_ms"] - 1 <= res["margin"][r["kernel"]]
        res["all_within_margin"] = all(r["within_margin"] for r in rows if "parent" in r)
        print("margins:", json.dumps(res["margin"]), "new within them on every case:", res["all_within_margin"])
    timed_rows = [r for r in rows if "parent" in r and "wino4" in r["kernel"]]
    if timed_rows:  # the step's F(4x4) launches, one of each: sum of the medians per arm
        res["wino4_sum_of_medians_ms"] = {nm: round(sum(r[nm]["median_ms"] for r in timed_rows), 4) for nm in names}
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res.get("wino4_sum_of_medians_ms", {})))
    print("all outputs and workspaces bitwise equal:", all_equal)
    return 1 if not all_equal else 0 if res.get("all_within_margin", True) else 2


if __name__ == "__main__":
    sys.exit(main())
