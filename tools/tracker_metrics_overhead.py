"""Cost of the ActivityMonitor metric sets on the train step, 256x256, batch 16, fp32 and bf16 (one GPU):
  shipped  -- the 3 mean_abs layers of experiment_synthetic_test.yaml (fused trackers)
  hooks    -- the tracking set of experiment_synthetic_all_metrics.yaml (the reference's cifar10_test set + mean / std at
              decoder.conv_norm_out's input) on torch hooks (tracking.device_metrics: false)
  device   -- the same set with tracking.device_metrics: true
Arms alternate inside one process; each block runs 2 track_intervals of steps (monitor.step() included) after an untimed
warm-up step; per-step times are device events on the launch stream; medians per arm.
    python tools/tracker_metrics_overhead.py [--rounds 2] [--interval 4] [--out profiles/tracker_metrics_overhead.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402
import yaml  # noqa: E402

CFG = os.path.join(ROOT, "vae-channel-dynamics_amd", "configs")


def arms(interval):
    shipped = yaml.safe_load(open(os.path.join(CFG, "experiment_synthetic_test.yaml")))["tracking"]
    full = yaml.safe_load(open(os.path.join(CFG, "experiment_synthetic_all_metrics.yaml")))["tracking"]
    out = {"shipped": dict(shipped, track_interval=interval),
           "hooks": dict(full, track_interval=interval, device_metrics=False),
           "device": dict(full, track_interval=interval, device_metrics=True)}
    return out


def measure(dtype, rounds, interval, B=16, R=256):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    w = SDXLVAEWrapper("synthetic:42", device=dev)
    tr = HipTrainer(w, lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100, max_train_steps=10000,
                    mixed_precision="bf16" if dtype == "bf16" else "no")
    gen = torch.Generator(device=dev).manual_seed(42)
    x = torch.rand((B, 3, R, R), device=dev, generator=gen) * 2 - 1
    eps = torch.randn((B, 4, R // 8, R // 8), device=dev, generator=gen)
    cfgs = arms(interval)
    times = {k: [] for k in cfgs}
    info = {}
    for _ in range(rounds):
        for name, cfg in cfgs.items():
            mon = ActivityMonitor(w, cfg)
            info[name] = {"fused_layers": len(mon.fused_layers), "device_layers": len(mon.device_layers),
                          "hooks": sum(1 for m in w.modules() if m._forward_hooks or m._forward_pre_hooks)}
            # untimed: one step, then run up to the next track_interval boundary so every timed block holds 2 intervals
            tr.train_step(x, eps)
            while tr.global_step % interval:
                tr.train_step(x, eps)
            mon.step(tr.global_step)
            mon.hook_collected_buffer.clear()
            n = 2 * interval
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(n):
                tr.train_step(x, eps)
                mon.step(tr.global_step)
                ev[i + 1].record()
            torch.cuda.synchronize()
            times[name] += [ev[i].elapsed_time(ev[i + 1]) for i in range(n)]
            mon.remove_hooks()
            del mon
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    return {"median_ms": {k: round(v, 3) for k, v in med.items()},
            "overhead_vs_shipped": {k: round(med[k] / med["shipped"] - 1.0, 4) for k in med},
            "steps_per_arm": len(times["shipped"]), "arms": info,
            "step_ms": {k: [round(t, 2) for t in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--interval", type=int, default=4)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracker_metrics_overhead.json"))
    a = ap.parse_args()
    res = {"shape": "256x256, batch 16, one GPU", "track_interval": a.interval, "rounds": a.rounds,
           "gpu": torch.cuda.get_device_name(0)}
    for dt in a.dtypes.split(","):
        res[dt] = measure(dt, a.rounds, a.interval)
        print(dt, json.dumps(res[dt]["median_ms"]), json.dumps(res[dt]["overhead_vs_shipped"]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
