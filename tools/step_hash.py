"""One Engine.forward_backward on the synthetic model in this process (library: VAEHIP_LIB, default the tree's build): SHA-256 of `scalars`, of
`arena.grad` and of the LaunchProfiler kernel-name sequence, as one JSON line -- to set two builds of the library next to each other, a
fresh process each (profiles/bf16_tile_common_measured.json).
usage: python tools/step_hash.py no|bf16 R B [ck] [family=SUB,SUB,...]     (ck: with checkpoint_decoder; family: the substrings
that pick `family_kernels` out of the step's kernel names, default the bf16 halo-tile family)"""
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
