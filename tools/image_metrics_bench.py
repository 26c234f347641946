"""Time of the metrics portion of one evaluate.py batch, operands already on the device (one GPU):
  new  -- vaehip.metrics.ImageMetrics.update on the engine's channels-last reconstruction + the device-side KL sum
  old  -- what evaluate.main() did before the kernel existed: F.mse_loss(...).item(), kl.mean().item(),
          to_unit(rec).contiguous(), psnr_sums, ssim_per_image (float64 grouped 11 x 11 convolution in torch)
at 256 x 256 with batch 16 and at 1024 x 1024 with batch 2.  Device events around each repetition after a warm-up, arms
alternated, median per arm.  The results of the two arms are compared before anything is timed.
    python tools/image_metrics_bench.py [--reps 20] [--out profiles/image_metrics_measured.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/image_metrics_bench.py --only-new --out ""
    python tools/image_metrics_bench.py --merge-kernel-stats DIR/.../k_kernel_stats.csv   (kernel times into the JSON; no GPU)"""
import argparse
import csv
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = {"256x256_b16": (16, 3, 256, 256), "1024x1024_b2": (2, 3, 1024, 1024)}
DEFAULT_OUT = os.path.join(ROOT, "profiles", "image_metrics_measured.json")


def operands(shape, dev):
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(42)
    pv = torch.rand(shape, device=dev, generator=g) * 2.2 - 1.1
    rec = (pv + 0.1 * torch.randn(shape, device=dev, generator=g)).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    kl = torch.rand((B,), device=dev, generator=g) * 100
    return rec, pv, kl


def old_path(rec, pv, kl, ev):
    b = pv.shape[0]
    total_mse = F.mse_loss(rec.float(), pv.float(), reduction="mean").item() * b
    total_kl = kl.mean().item() * b
    r01, o01 = ev.to_unit(rec).contiguous(), ev.to_unit(pv)
    s, c = ev.psnr_sums(r01, o01)
    ssim_sum = ev.ssim_per_image(r01, o01).double().sum()
    return total_mse, total_kl, s, c, ssim_sum


def new_path(rec, pv, kl, metrics, kl_sum):
    metrics.update(rec.float(), pv)
    kl_sum += kl.double().sum()


def timed(fn, reps):
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return t


def measure(name, shape, reps, only_new):
    import evaluate as ev
    from vaehip.lib import lib
    from vaehip.metrics import ImageMetrics
    dev = torch.device("cuda:0")
    rec, pv, kl = operands(shape, dev)
    B, C, H, W = shape
    kl_sum = torch.zeros((), dtype=torch.float64, device=dev)
    m = ImageMetrics()
    new_path(rec, pv, kl, m, kl_sum)
    got = m.compute()
    n = ctypes.c_int64(0)
    lib.call("vae_image_metrics_workspace", B, C, H, W, ctypes.byref(n))
    # what the kernels must move: both operands once, and the workspace written, then read by the final pass
    res = {"shape": list(shape), "bytes_read_min": 2 * B * C * H * W * 4, "workspace_bytes": n.value * 8, "workgroups": n.value // 3}
    if not only_new:
        mse, _, s, c, ssim_sum = old_path(rec, pv, kl, ev)
        want = {"avg_mse": mse / B, "psnr": 10.0 * math.log10(1.0 / (float(s) / c)), "ssim": float(ssim_sum) / B}
        res["new_vs_old_relative_difference"] = {k: abs(got[k] - want[k]) / abs(want[k]) for k in want}
        assert all(v < 1e-5 for v in res["new_vs_old_relative_difference"].values()), res  # avg_mse of the old path is an fp32 mean
    t_new, t_old = [], []
    for _ in range(2):  # two blocks per arm, alternated
        m = ImageMetrics()
        t_new += timed(lambda: new_path(rec, pv, kl, m, kl_sum), reps // 2)
        if not only_new:
            t_old += timed(lambda: old_path(rec, pv, kl, ev), reps // 2)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    res["new_median_ms"] = round(med(t_new), 4)
    res["new_ms"] = [round(x, 4) for x in t_new]
    if t_old:
        res["old_median_ms"] = round(med(t_old), 4)
        res["old_ms"] = [round(x, 3) for x in t_old]
    print(name, json.dumps({k: v for k, v in res.items() if not k.endswith("_ms") or "median" in k}), flush=True)
    return res


def merge_kernel_stats(path, out):
    """average time of the two kernels from a rocprofv3 --kernel-trace --stats run of --only-new (both shapes in one run: the
    per-shape split comes from the trace's min / max, the 256^2 batch being the smaller launch)"""
    res = json.load(open(out))
    rows = {}
    for r in csv.DictReader(open(path)):
        for k in ("image_metrics_partial_kernel", "image_metrics_final_kernel"):
            if k in r["Name"]:
                rows[k] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                           "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}
    res["kernel_trace"] = rows
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--merge-kernel-stats", default=None)
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.out or DEFAULT_OUT)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured on the CPU")
    res = {"gpu": torch.cuda.get_device_name(0), "reps": a.reps,
           "what": "metrics portion of one evaluate batch, operands on the device; device events, median"}
    for name in a.shapes.split(","):
        res[name] = measure(name, SHAPES[name], a.reps, a.only_new)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
