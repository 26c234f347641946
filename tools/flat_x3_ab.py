"""A/B of the flat implicit-GEMM kernels (csrc/igemm.hip) under the split-bf16 policy against exact fp32 products, in one process:
this build's libvaehip.so and the same tree built with -DVAE_FLAT_X3=0 (the A/B arm), optionally the parent commit's library as
a third, whose outputs the switched-off build must match BIT FOR BIT on every row (exit status 1 otherwise).

Rows: every distinct flat launch of the headline step (fp32, 256^2, batch 16): the three stride-2 downsamplers and the four 1x1
shortcuts, each forward / dgrad / wgrad; the attention linears (1x1 over 1024 tokens x 16 images, forward also with the GroupNorm
affine fused into the staging) and the three batched GEMMs at T = 1024, C = 512, z = 16.  Per row the operands are filled once;
every library launches into its own outputs (NaN before the launch).  Then the arms are timed alternately with device events
around the launch alone (3 warm-up rounds, `--launches` launches per arm, interleaved launch by launch, the opening arm rotating):
median, quartiles, new / off.  The error of both arms is taken against float64 (im2col and matmul on the device) on a part of the result
(the first image of a forward / dgrad, the first 8 output channels of a weight gradient, the first batch item of a GEMM), on the
scale of that reference's max.

OFF.so: `make -C vae-channel-dynamics_amd/csrc flat_x3_off` (csrc/libvaehip_x3off.so).

usage: python tools/flat_x3_ab.py NEW.so OFF.so [PARENT.so] [--launches 20] [--out FILE] [--small]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vae-channel-dynamics_amd", "src"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from vaehip import ops  # noqa: E402
from vaehip.lib import IgemmArgs, WgradArgs, lib  # noqa: E402

DOWN = [(128, 256), (256, 128), (512, 64)]                                   # channels, input map of the stride-2 layers
SHORT = [(128, 256, 128), (256, 512, 64), (512, 256, 128), (256, 128, 256)]  # Cin, Cout, map of the 1x1 shortcuts


def cases(small):
    B = 2 if small else 16
    s = 8 if small else 1  # (--small: maps an eighth the size, for a quick check of the tool itself)
    out = [("c3s2", m, B, hw // s, hw // s, c, c, 0) for c, hw in DOWN for m in ("fwd", "dgrad", "wgrad")]
    out += [("c1", m, B, hw // s, hw // s, ci, co, 0) for ci, co, hw in SHORT for m in ("fwd", "dgrad", "wgrad")]
    out += [("c1", m, B, 32, 32, 512, 512, xf) for m, xf in (("fwd", 0), ("fwd", ops.XF_AFFINE), ("dgrad", 0), ("wgrad", 0), ("wgrad", ops.XF_AFFINE))]
    T = 1024 // (s * s)
    out += [("gemm", m, B, 1, T, 512, 512, 0) for m in ("nt", "nn", "tn")]
    return out


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _open(path):
    lib.load()  # (one HIP runtime per process: the package's loader opens torch's copy first)
    dll = C.CDLL(os.path.abspath(path))
    ia, wa, vp = C.POINTER(IgemmArgs), C.POINTER(WgradArgs), C.c_void_p
    for fn, res, argt in (("vae_igemm_rows", C.c_int, [ia, vp]), ("vae_igemm_kernel_name", C.c_int, [ia, C.c_char_p, C.c_int32]),
                          ("vae_wgrad", C.c_int, [wa, vp]), ("vae_wgrad_plan", C.c_int, [wa, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
                          ("vae_wgrad_kernel_name", C.c_int, [wa, C.c_char_p, C.c_int32])):
        getattr(dll, fn).restype, getattr(dll, fn).argtypes = res, argt
    return dll


def _bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


class Case:
    """operands of one row, filled once; arm(dll, st) -> (launch, outputs); error(outputs) against float64"""

    def __init__(self, dev, kind, mode, B, H, W, Ci, Co, xf):
        self.dev, self.kind, self.mode, self.dims, self.xf = dev, kind, mode, (B, H, W, Ci, Co), xf
        g = torch.Generator(device=dev).manual_seed(5 + Ci + 3 * Co + H + W + len(mode))
        rnd = lambda *s: torch.randn(s, device=dev, generator=g)  # noqa: E731
        if kind == "gemm":  # z = B, T = W tokens, C = Ci
            T = W
            self.A, self.Bm = (rnd(B, T, Ci), rnd(B, T, Ci)) if mode == "nt" else (rnd(B, T, T), rnd(B, T, Ci))
            return
        k = 1 if kind == "c1" else 3
        self.k = k
        Hy, Wy = ops.out_hw(kind, H, W)
        self.w = rnd(Co, k, k, Ci) / math.sqrt(k * k * Ci)
        self.x = rnd(B, H, W, Ci) * 1.3 + 0.2 if mode != "dgrad" else None
        self.dy = rnd(B, Hy, Wy, Co) if mode != "fwd" else None
        self.bias = rnd(Co) if mode == "fwd" else None
        self.scale, self.shift = (torch.rand((B, Ci), device=dev, generator=g) + 0.5, rnd(B, Ci)) if xf else (None, None)

    def arm(self, dll, st):
        B, H, W, Ci, Co = self.dims
        dev, nan, buf = self.dev, float("nan"), C.create_string_buffer(128)
        if self.kind == "gemm" and self.mode != "tn":
            T = W
            M, N, K, bkm = (T, T, Ci, False) if self.mode == "nt" else (T, Ci, T, True)
            a = ops.gemm_rows_args(M, N, K, bkm, Ci ** -0.5 if self.mode == "nt" else 1.0, B, prec=ops.PREC_F32)
            outs = {"out": torch.full((B, M, N), nan, device=dev)}
            a.A, a.W, a.C = _p(self.A), _p(self.Bm), _p(outs["out"])
        elif self.kind == "gemm":
            a = ops.gemm_tn_args(W, Ci, W, 1.0, B, prec=ops.PREC_F32)
            outs = {"out": torch.full((B, W, Ci), nan, device=dev)}
            a.dY, a.X, a.out = _p(self.A), _p(self.Bm), _p(outs["out"])
        elif self.mode == "wgrad":
            a = ops.wgrad_args(self.kind, B, H, W, Ci, Co, Ci, xf=self.xf, prec=ops.PREC_F32)
            a.dY, a.X, a.scale, a.shift = _p(self.dy), _p(self.x), _p(self.scale), _p(self.shift)
            n, fus = C.c_int32(0), C.c_int32(0)
            assert dll.vae_wgrad_plan(C.byref(a), C.byref(n), C.byref(fus)) == 0 and n.value > 0
            assert fus.value or not self.xf, "the plan does not fuse the transform at this size"
            outs = {"slab": torch.full((n.value, Co * self.k * self.k * Ci), nan, device=dev), "bias_partial": torch.full((n.value, Co), nan, device=dev)}
            a.nsplit, a.bias_partial = n.value, _p(outs["bias_partial"])
            a.out, a.partial = (_p(outs["slab"]), None) if n.value == 1 else (None, _p(outs["slab"]))
        else:
            if self.mode == "fwd":
                a = ops.fwd_args(self.kind, B, H, W, Ci, Co, Ci, xf=self.xf, prec=ops.PREC_F32)
                src, oshape = self.x, (B, *ops.out_hw(self.kind, H, W), Co)
            else:
                a = ops.dgrad_args(self.kind, B, H, W, Co, Ci, prec=ops.PREC_F32)
                src, oshape = self.dy, (B, H, W, Ci)
            outs = {"out": torch.full(oshape, nan, device=dev)}
            a.A, a.W, a.C, a.bias, a.scale, a.shift = _p(src), _p(self.w), _p(outs["out"]), _p(self.bias), _p(self.scale), _p(self.shift)
        rows = isinstance(a, IgemmArgs)
        (dll.vae_igemm_kernel_name if rows else dll.vae_wgrad_kernel_name)(C.byref(a), buf, 128)
        self.kernel = buf.value.decode()
        fn = dll.vae_igemm_rows if rows else dll.vae_wgrad

        def launch():
            rc = fn(C.byref(a), st)
            assert rc == 0, rc
        return launch, outs, a

    def reference(self):
        """float64 on the device (im2col + matmul) -> (reference, function taking an arm's outputs to the same part of its result)"""
        B, H, W, Ci, Co = self.dims
        d = torch.float64
        if self.kind == "gemm":
            A, Bm = self.A[0].to(d), self.Bm[0].to(d)
            ref = {"nt": lambda: Ci ** -0.5 * A @ Bm.T, "nn": lambda: A @ Bm, "tn": lambda: A.T @ Bm}[self.mode]()
            return ref, lambda o: o["out"][0].double()
        k, s2 = self.k, self.kind == "c3s2"
        Hy, Wy = ops.out_hw(self.kind, H, W)
        w2 = self.w.to(d).permute(0, 3, 1, 2).reshape(Co, -1)  # [Co, (Ci, kh, kw)]: the row order of unfold

        def cols(x):  # NHWC [n, H, W, Ci] -> [n, Ci k k, Hy Wy]
            x = x.to(d).permute(0, 3, 1, 2)
            return F.unfold(F.pad(x, (0, 1, 0, 1)) if s2 else x, k, stride=2 if s2 else 1)

        def act(x, b0):
            if not self.xf:
                return x
            return x.to(d) * self.scale.to(d)[b0:b0 + x.shape[0], None, None, :] + self.shift.to(d)[b0:b0 + x.shape[0], None, None, :]
        if self.mode == "fwd":
            y = w2 @ cols(act(self.x[:1], 0))[0] + self.bias.to(d)[:, None]
            return y.T.reshape(1, Hy, Wy, Co), lambda o: o["out"][:1].double()
        if self.mode == "dgrad":
            c = w2.T @ self.dy[0].to(d).reshape(-1, Co).T  # [(Ci, kh, kw), Hy Wy]
            gx = F.fold(c[None], (H + 1, W + 1) if s2 else (H, W), k, stride=2 if s2 else 1)[:, :, :H, :W]
            return gx.permute(0, 2, 3, 1), lambda o: o["out"][:1].double()
        gw = torch.zeros(8, Ci * k * k, dtype=d, device=self.dev)
        for b in range(B):  # (image by image: the im2col of one image is 150 MB at most)
            gw += self.dy[b, :, :, :8].to(d).reshape(-1, 8).T @ cols(act(self.x[b:b + 1], b))[0].T
        return gw.view(8, Ci, k, k).permute(0, 2, 3, 1).reshape(8, -1), lambda o: o["slab"].double().sum(0).view(Co, -1)[:8]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+", help="NEW.so OFF.so [PARENT.so]")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--small", action="store_true")
    arg = ap.parse_args()
    assert 2 <= len(arg.libs) <= 3, "this build, the build with -DVAE_FLAT_X3=0, and optionally the parent's"
    names = ["new", "off", "parent"][:len(arg.libs)]
    dlls = [_open(s) for s in arg.libs]
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, off_is_parent = [], True
    for kind, mode, B, H, W, Ci, Co, xf in cases(arg.small):
        c = Case(dev, kind, mode, B, H, W, Ci, Co, xf)
        ref, part = c.reference()
        torch.cuda.synchronize()
        launches, keep, row = [], [], {"kind": kind, "mode": mode, "B": B, "H": H, "W": W, "Cin": Ci, "Cout": Co, "xf": xf}
        for nm, d in zip(names, dlls):
            launch, outs, a = c.arm(d, st)
            launch()
            torch.cuda.synchronize()
            launches.append(launch)
            keep.append((outs, a))
            if nm != "parent":
                row[f"{nm}_err_vs_float64"] = float((part(outs) - ref).abs().max() / ref.abs().max())
                row[f"{nm}_finite"] = all(bool(torch.isfinite(t).all()) for t in outs.values())
        row["kernel"] = c.kernel
        if "parent" in names:
            row["off_bitwise_parent"] = all(_bits(keep[1][0][k], keep[2][0][k]) for k in keep[1][0])
            off_is_parent = off_is_parent and row["off_bitwise_parent"]
        timed = launches[:2]
        for _ in range(3):
            for launch in timed:
                launch()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(arg.launches)] for _ in timed]
        for k in range(arg.launches):
            for i in ((k + j) % 2 for j in range(2)):
                ev[i][k][0].record()
                timed[i]()
                ev[i][k][1].record()
        torch.cuda.synchronize()
        for i, nm in enumerate(names[:2]):
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev[i])
            q = statistics.quantiles(ms, n=4)
            row[nm] = {"median_ms": round(statistics.median(ms), 4), "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "min_ms": round(ms[0], 4)}
        row["new_over_off"] = round(row["new"]["median_ms"] / row["off"]["median_ms"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del c, launches, keep, timed
        torch.cuda.empty_cache()
    res = {"libs": dict(zip(names, [os.path.basename(s) for s in arg.libs])), "launches_per_arm": arg.launches, "rows": rows,
           "sum_of_medians_ms": {nm: round(sum(r[nm]["median_ms"] for r in rows), 4) for nm in names[:2]},
           "sum_of_quartile_spreads_ms": {nm: round(sum(r[nm]["q3_ms"] - r[nm]["q1_ms"] for r in rows), 4) for nm in names[:2]}}
    if "parent" in names:
        res["off_bitwise_parent_on_every_row"] = off_is_parent
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}))
    if arg.out:
        with open(arg.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if off_is_parent else 1


if __name__ == "__main__":
    sys.exit(main())
