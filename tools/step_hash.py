"""One Engine.forward_backward on the synthetic model in this process (library: VAEHIP_LIB, default the tree's build): SHA-256 of `scalars`, of
`arena.grad` and of the LaunchProfiler kernel-name sequence, as one JSON line -- to set two builds of the library next to each other, a
fresh process each (profiles/bf16_tile_common_measured.json).
usage: python tools/step_hash.py no|bf16 R B [ck] [metrics] [family=SUB,SUB,...]     (ck: with checkpoint_decoder; family: the substrings
that pick `family_kernels` out of the step's kernel names, default the bf16 halo-tile family; metrics: instead, four HipTrainer steps with
`tracking.device_metrics` on at seven capture points, and the hashes of the monitor's exported records, of `arena.grad` and of the names)"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vae-channel-dynamics_amd", "src"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
import vae_oracle as vo
from models.sdxl_vae_wrapper import SDXLVAEWrapper
from vaehip import ops
mode, R, B, ck = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), "ck" in sys.argv[4:]
subs = ([a.split("=", 1)[1] for a in sys.argv[4:] if a.startswith("family=")] or ["tile_bf16,wide_bf16,dma_bf16"])[0].split(",")
dev = torch.device("cuda:0")
o = vo.OracleWrapper(seed=42)
w = SDXLVAEWrapper("synthetic:1")
w.vae.load_state_dict(o.vae.state_dict())
w.to(dev)
if "metrics" in sys.argv[4:]:  # the trainer's steps with the ActivityMonitor served from the device reductions
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    all4 = ["mean_abs_activation_per_channel", "full_activation_map", "mean_activation", "std_activation"]
    points = [("vae.encoder.conv_in", "output"), ("vae.encoder.down_blocks.0.resnets.0.norm1", "input"), ("vae.encoder.down_blocks.0.resnets.0.norm1", "output"),
              ("vae.encoder.down_blocks.0.resnets.0.conv1", "input"), ("vae.decoder.up_blocks.0.upsamplers.0.conv", "output"), ("vae.encoder", "input"),
              ("vae.decoder.conv_norm_out", "input")]
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mode, checkpoint_decoder=ck)
    mon = ActivityMonitor(w, {"enabled": True, "track_interval": 2, "device_metrics": True,
                              "target_layers": [{"name": n, "capture_point": p, "metrics": all4} for n, p in points]})
    prof = ops.PROFILER = ops.LaunchProfiler()
    for s in range(1, 5):
        tr.train_step(vo.synthetic_pixels(B, R, 5, s).to(dev), vo.synthetic_eps(B, R, 5, s).to(dev))
        mon.step(s)
    torch.cuda.synchronize()

    def canon(o):  # tensors and arrays as the hash of their bytes, floats as their exact repr
        if isinstance(o, torch.Tensor):
            return hashlib.sha256(o.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
        if isinstance(o, dict):
            return {str(k): canon(v) for k, v in sorted(o.items(), key=lambda kv: str(kv[0]))}
        if isinstance(o, (list, tuple)):
            return [canon(v) for v in o]
        return repr(o.tolist()) if hasattr(o, "tolist") else repr(o)
    rec = mon.export_all_processed_data_to_records()
    names = [str(r[0]) for r in prof.records]
    print(json.dumps({"lib": os.path.basename(os.environ.get("VAEHIP_LIB", "libvaehip.so")), "mode": mode, "R": R, "B": B, "checkpoint_decoder": ck,
                      "device_metrics": True, "records": len(rec), "records_sha256": hashlib.sha256(json.dumps(canon(rec), sort_keys=True).encode()).hexdigest(),
                      "grad_sha256": hashlib.sha256(w.vae.arena.grad.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest(),
                      "launches": len(names), "names_sha256": hashlib.sha256("\n".join(names).encode()).hexdigest()}))
    sys.exit(0)
eng = w.vae.engine
eng.set_precision(mode)
ops.ACT_BF16 = mode == "bf16"
eng.checkpoint_decoder = ck
x, eps = vo.synthetic_pixels(B, R, 42, 5).to(dev), vo.synthetic_eps(B, R, 42, 5).to(dev)
prof = ops.PROFILER = ops.LaunchProfiler()
res = eng.forward_backward(x, eps, 1e-4)
torch.cuda.synchronize()
h = lambda t: hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
names = [str(r[0]) for r in prof.records]
fam = sorted({n for n in names if any(s in n for s in subs)})
print(json.dumps({"lib": os.path.basename(os.environ.get("VAEHIP_LIB", "libvaehip.so")), "mode": mode, "R": R, "B": B, "checkpoint_decoder": ck,
                  "scalars": [float(v) for v in res["scalars"].cpu()], "scalars_sha256": h(res["scalars"]), "grad_sha256": h(w.vae.arena.grad),
                  "launches": len(names), "names_sha256": hashlib.sha256("\n".join(names).encode()).hexdigest(), "family_kernels": fam}))
