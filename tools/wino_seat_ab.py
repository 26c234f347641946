"""A/B of two (or more) builds of the fp32 Winograd convolutions in one process: this build against the parent commit's
libvaehip.so (built in a scratch worktree; nothing of it is committed), further builds optional (a lever of
one kernel switched the other way, e.g. conv3_wino4.hip compiled with -DVAE_W4_SWAVE=0 and linked into another file).

Per case the operands are filled once; every library builds its own transformed weights (vae_wino_weights) and launches
vae_igemm_rows into its own output, `gstat` workspace and `gnb` workspace, which start as NaN and are compared with the FIRST
library's BIT FOR BIT.  Then the arms are timed alternately with device events around the convolution launch alone (warm-up,
`--launches` launches per arm, interleaved launch by launch): median, quartiles and extremes per arm.

Cases: F(4x4) forward and dgrad of the plain 3x3 layers of the fp32 step (256^2, batch 16), each bare and with the epilogue it
runs with in the step (forward: bias + residual + GroupNorm moments; dgrad: GroupNorm(+SiLU)-backward sums); the small cases
of tests/test_wino4_seat_gpu.py (bitwise only); the upsampler convolutions (csrc/conv3_upwino.hip forward and dgrad,
csrc/wgrad3_upwino.hip through vae_wgrad_wino).

usage: python tools/wino_seat_ab.py NEW.so PARENT.so [name=OTHER.so ...] [--launches 20] [--out FILE] [--only wino4|up]"""
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
            ("c3", "fwd", 2, 32, 64, 128, 128, True, False), ("c3", "dgrad", 2, 16, 32, 128, 64, True, False)])
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
                          ("vae_wgrad_wino_plan", C.c_int, [wa, C.POINTER(C.c_int32)]), ("vae_wgrad_wino_positions", C.c_int, [wa])):
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
            a = ops.fwd_args(self.kind, B, H, W, Ci, Co, Ci, prec=ops.PREC_F32)
            src, oshape = self.x, (B, *ops.out_hw(self.kind, H, W), Co)
            a.bias, a.res = _p(self.bias), _p(self.res)
        else:
            a = ops.up2x_dgrad_args(B, H, W, Co, Ci, prec=ops.PREC_F32) if self.kind == "c3up" else ops.dgrad_args(self.kind, B, H, W, Co, Ci, prec=ops.PREC_F32)
            src, oshape = self.dy, (B, H, W, Ci)
        out = torch.full(oshape, nan, device=dev)
        a.A, a.W, a.C = _p(src), _p(self.w), _p(out)
        assert dll.vae_wino_ok(C.byref(a)), "no Winograd kernel for this case"
        outs = {"out": out}
        wu = torch.empty((int(dll.vae_wino_weight_floats(C.byref(a))),), device=dev)
        assert dll.vae_wino_weights(C.byref(a), _p(wu), st) == 0
        a.Wu = _p(wu)  # (the epilogue queries below are about the kernel the transformed weights select)
        if self.epi and self.mode == "fwd":
            a.gstat_groups = 32
            nch = dll.vae_conv_gstat_chunks(C.byref(a))
            assert nch > 0
            outs["gstat"] = torch.full((B, nch, 32, 2), nan, device=dev)
            a.gstat = _p(outs["gstat"])
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
    ap.add_argument("--only", default="", choices=["", "wino4", "up"])
    arg = ap.parse_args()
    assert len(arg.libs) >= 2, "two libraries: this build and the parent's"
    names = ["new", "parent"] + [s.split("=", 1)[0] for s in arg.libs[2:]]
    dlls = [_open(s.split("=", 1)[-1]) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = (STEP + SMALL if arg.only != "up" else []) + (UP if arg.only != "wino4" else [])
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
                for i, launch in enumerate(launches):
                    ev[i][k][0].record()
                    launch()
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
    timed_rows = [r for r in rows if "parent" in r and "wino4" in r["kernel"]]
    if timed_rows:  # the step's F(4x4) launches, one of each: sum of the medians per arm
        res["wino4_sum_of_medians_ms"] = {nm: round(sum(r[nm]["median_ms"] for r in timed_rows), 4) for nm in names}
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res.get("wino4_sum_of_medians_ms", {})))
    print("all outputs and workspaces bitwise equal:", all_equal)
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
