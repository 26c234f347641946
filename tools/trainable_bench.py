"""What freezing part of the model saves and what the optimizer step over ranges costs, on one GPU, one process:

  steps    HipTrainer at 256x256 (fp32 batch 16, bf16 batch 32): one trainer, set_trainable('all') and set_trainable('decoder')
           alternating, blocks of --steps timed steps after an untimed one; per arm the median step, the spread between
           repeats and the peak allocated memory of a step.  Accepted when the decoder-only median is below the full median by
           more than the spread of the full step (max - min of its block medians).
  kernels  device events around windows of --calls calls at the real arena: vae_sqnorm + vae_adamw over the whole arena | the
           two *_ranges calls with one whole-arena range | with the `decoder` range | with the GroupNorm ranges.

    timeout -k 10 900 python tools/trainable_bench.py [--out profiles/trainable_measured.json]

The program ends itself after --limit seconds as well.  No GPU: it fails (there is nothing to measure on a CPU)."""
import argparse
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))

import torch  # noqa: E402

HYPER = (1e-5, 0.9, 0.999, 1e-8, 1e-2)   # lr, betas, eps, weight decay: small steps, the state stays of the size it starts with


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3), "n": len(xs)}


def step_arms(mode, B, steps, rounds, dev, R=256):
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from vaehip.trainer import HipTrainer
    gen = torch.Generator(device=dev).manual_seed(42)
    x = torch.rand((B, 3, R, R), device=dev, generator=gen) * 2 - 1
    eps = torch.randn((B, 4, R // 8, R // 8), device=dev, generator=gen)
    tr = HipTrainer(SDXLVAEWrapper("synthetic:42", device=dev), lr=1e-5, max_grad_norm=1.0, kl_weight=1e-6, lr_warmup_steps=100,
                    max_train_steps=100000, mixed_precision=mode)
    arms = ("all", "decoder")
    for arm in arms:   # every shape and every table of the timed blocks, once
        tr.set_trainable(arm)
        tr.train_step(x, eps)
    torch.cuda.synchronize()
    ms, medians, peak = {a: [] for a in arms}, {a: [] for a in arms}, {}
    for _ in range(rounds):
        for arm in arms:
            tr.set_trainable(arm)
            tr.train_step(x, eps)
            tr.last = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            ev[0].record()
            for i in range(steps):
                tr.train_step(x, eps)
                ev[i + 1].record()
            torch.cuda.synchronize()
            block = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
            ms[arm] += block
            medians[arm].append(sorted(block)[len(block) // 2])
            peak[arm] = torch.cuda.max_memory_allocated()
    out = {arm: {"step_ms": spread(ms[arm]), "block_medians_ms": [round(v, 3) for v in medians[arm]],
                 "peak_allocated_GiB": round(peak[arm] / 2 ** 30, 3), "images_per_s": round(B / spread(ms[arm])["median"] * 1e3, 2)}
           for arm in arms}
    full_spread = max(medians["all"]) - min(medians["all"])
    gain = out["all"]["step_ms"]["median"] - out["decoder"]["step_ms"]["median"]
    out.update(batch=B, resolution=R, full_step_spread_between_repeats_ms=round(full_spread, 3), decoder_saves_ms=round(gain, 3),
               decoder_over_all=round(out["decoder"]["step_ms"]["median"] / out["all"]["step_ms"]["median"], 4),
               accepted=bool(gain > full_spread))
    return out


def kernel_arms(calls, rounds, dev):
    from vaehip import ops
    from vaehip.autoencoder import AutoencoderKLHip
    from vaehip.trainable import RangeTable, apply_trainable
    vae = AutoencoderKLHip()   # on the CPU: only its arena layout is wanted
    a = vae.arena
    n = a.total
    tables = {"ranges_whole_arena": RangeTable([(0, n)], dev, n)}
    for name, value in (("ranges_decoder", "decoder"),
                        ("ranges_groupnorms", [k for k, m in vae.named_modules() if isinstance(m, torch.nn.GroupNorm)])):
        apply_trainable(vae, value)
        tables[name] = RangeTable(a.trainable_ranges(), dev, n)
    gen = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=gen) * 0.05
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    m = torch.randn(n, device=dev, generator=gen) * 1e-4
    v = torch.rand(n, device=dev, generator=gen) * 1e-6
    sq, ws = torch.zeros(1, device=dev), torch.empty(2048, device=dev)

    def whole():
        ops.sqnorm(g, sq, ws)
        ops.adamw(p, g, m, v, sq, 1.0, *HYPER, 100)

    def over(t):
        def fn():
            ops.sqnorm_ranges(g, t, sq)
            ops.adamw_ranges(p, g, m, v, None, t, sq, 1.0, *HYPER, 100)
        return fn
    arms = {"sqnorm+adamw_whole_arena": whole}
    arms.update({k: over(t) for k, t in tables.items()})
    us = {k: [] for k in arms}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in arms.items():
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    out = {}
    for name, xs in us.items():
        t = tables.get(name)
        elems = n if t is None else t.numel
        s = spread(xs)
        out[name] = {"us_per_pair": s, "ranges": 1 if t is None else t.nseg, "chunks": None if t is None else t.nchunk, "elements": elems,
                     "GB_per_s_at_median": round(8 * elems * 4 / (s["median"] * 1e-6) / 1e9, 1)}   # 1 pass for the norm, 7 for the update
    old, new = out["sqnorm+adamw_whole_arena"]["us_per_pair"], out["ranges_whole_arena"]["us_per_pair"]
    out["whole_arena_ranges_minus_old_pair_us"] = round(new["median"] - old["median"], 3)
    out["old_pair_spread_us"] = round(old["max"] - old["min"], 3)
    out["whole_arena_ranges_slower_than_spread"] = bool(new["median"] - old["median"] > old["max"] - old["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="optimizer call pairs per timed window")
    ap.add_argument("--kernel-rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=6, help="train steps per timed block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=900, help="seconds after which the program ends itself")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainable_measured.json"))
    a = ap.parse_args()
    signal.alarm(a.limit)
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    dev = torch.device("cuda:0")
    res = {"gpu": torch.cuda.get_device_name(0), "calls_per_window": a.calls, "kernel_rounds": a.kernel_rounds,
           "steps_per_block": a.steps, "rounds": a.rounds}
    res["optimizer_kernels"] = kernel_arms(a.calls, a.kernel_rounds, dev)
    print("kernels", json.dumps(res["optimizer_kernels"]), flush=True)
    torch.cuda.empty_cache()
    for key, mode, B in (("steps_256_b16_fp32", "no", 16), ("steps_256_b32_bf16", "bf16", 32)):
        res[key] = step_arms(mode, B, a.steps, a.rounds, dev)
        print(key, json.dumps(res[key]), flush=True)
        torch.cuda.empty_cache()
    if os.path.exists(a.out):   # the headline comparison (bench.py at this commit and at its parent) is merged in from outside
        old = json.load(open(a.out))
        if "headline" in old:
            res["headline"] = old["headline"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
