"""tracking.device_metrics: every ActivityMonitor metric served from device reductions (ops.moments, csrc/track.hip) --
the kernel against float64, the monitor against the reference's golden fixture and against its own hook path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chanhist_refs as HR

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = "mean_abs_activation_per_channel"
ALL4 = [FUSED, "full_activation_map", "mean_activation", "std_activation"]
TOL = 1e-5  # per-channel mean |y| and std: relative; mean: relative to max(|mean|, std)


def _record(name, data):
    """measured deviations -> $VAEHIP_MEASURED_DIR/tracker_metrics_measured.json when that directory is given (the copy kept
    for the record is profiles/tracker_metrics_measured.json)"""
    out_dir = os.environ.get("VAEHIP_MEASURED_DIR")
    if not out_dir:
        return
    path = os.path.join(out_dir, "tracker_metrics_measured.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        cur = json.load(open(path)) if os.path.exists(path) else {}
        cur[name] = data
        json.dump(cur, open(path, "w"), indent=1)
    except OSError:
        pass


def _stats(B, ld, dev, seed):
    from vaehip.ops import Stats
    g = torch.Generator(device="cpu").manual_seed(seed)
    sc = (torch.rand((B, ld), generator=g) * 1.5 + 0.25).to(dev)
    sh = (torch.randn((B, ld), generator=g) * 0.5).to(dev)
    return Stats(None, None, sc, sh)


def _ref(x, st, xf):
    """float64 [per-channel mean |y|, mean, unbiased std] of y = XF(x) on the widened tensor"""
    from vaehip.ops import XF_AFFINE_SILU, XF_NONE
    Cc = x.shape[-1]
    y = x.float().double()
    if xf != XF_NONE:
        ld = st.scale.shape[1]
        sc = st.scale.double()[:, :Cc].reshape(x.shape[0], 1, 1, Cc)
        sh = st.shift.double()[:, :Cc].reshape(x.shape[0], 1, 1, Cc)
        assert ld >= Cc
        y = y * sc + sh
        if xf == XF_AFFINE_SILU:
            y = y * torch.sigmoid(y)
    return y.abs().mean(dim=(0, 1, 2)).cpu(), y.mean().cpu(), y.std().cpu()


def _errors(got, ref):
    ma, mean, std = ref
    Cc = ma.numel()
    g = got.double()
    e_ma = float(((g[:Cc] - ma).abs() / ma.abs().clamp_min(1e-30)).max())
    e_mean = float((g[Cc] - mean).abs() / max(abs(float(mean)), float(std)))
    e_std = float((g[Cc + 1] - std).abs() / std)
    return e_ma, e_mean, e_std


def _cases():
    out = []
    shapes = [(1, 7, 13), (3, 16, 16), (3, 7, 13), (1, 32, 24)]
    i = 0
    for Cc in (1, 3, 4, 8, 128, 256, 257, 512):
        for dt in (torch.float32, torch.bfloat16):
            for xf in (0, 1, 2):
                out.append((Cc, dt, xf) + shapes[i % len(shapes)])
                i += 1
    return out


@pytest.mark.parametrize("Cc,dt,xf,B,H,W", _cases())
def test_moments_against_float64(cuda, Cc, dt, xf, B, H, W):
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(Cc * 131 + xf * 7 + B)
    x = (torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4).to(cuda).to(dt)
    st = _stats(B, Cc, cuda, Cc + xf) if xf else None
    got = ops.moments(x, st, xf)
    torch.cuda.synchronize()
    errs = _errors(got.cpu(), _ref(x, st, xf))
    _record(f"moments/C{Cc}/{str(dt)[6:]}/xf{xf}/{B}x{H}x{W}", errs)
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("Cc,B,H,W,layout,dt,xf", HR.frame_params((0, 1, 2)))
def test_moments_at_the_edges_of_the_shared_frame(cuda, Cc, B, H, W, layout, dt, xf):
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(Cc * 131 + xf * 7 + B)
    x = HR.frame_layout((torch.randn((B, H, W, Cc), generator=g) * 1.3 + 0.4).to(cuda).to(dt), layout)
    st = _stats(B, x.stride(2), cuda, Cc + xf) if xf else None
    errs = _errors(ops.moments(x, st, xf).cpu(), _ref(x, st, xf))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("xf", [0, 2])
def test_moments_of_a_channel_prefix_view(cuda, dt, xf):
    """the encoder's input: the 3-channel view x4[..., :3] of a 4-channel buffer, read in place (pixel stride 4)"""
    from vaehip import ops
    g = torch.Generator(device="cpu").manual_seed(5)
    x4 = (torch.randn((3, 7, 13, 4), generator=g) - 0.2).to(cuda).to(dt)
    x4[..., 3] = 1e6  # the pad channel must not leak into the statistics
    x = x4[..., :3]
    st = _stats(3, 4, cuda, 9) if xf else None
    got = ops.moments(x, st, xf)
    errs = _errors(got.cpu(), _ref(x, st, xf))
    _record(f"moments/view3of4/{str(dt)[6:]}/xf{xf}", errs)
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("xf", [0, 2])
def test_moments_at_the_benchmark_norm1_size(cuda, xf):
    """16 x 256 x 256 x 128 fp32 (537 MB): the encoder's first GroupNorm at the benchmark shape"""
    from vaehip import ops
    torch.manual_seed(3)
    x = torch.randn((16, 256, 256, 128), device=cuda) * 0.8 + 0.3
    st = _stats(16, 128, cuda, 11) if xf else None
    got = ops.moments(x, st, xf)
    errs = _errors(got.cpu(), _ref(x, st, xf))
    _record(f"moments/bench_norm1/xf{xf}", errs)
    assert max(errs) <= TOL, errs


def test_moments_cancellation(cuda):
    """100 + 0.01 N(0, 1): a sum of y^2 in fp32 loses the std; the shifted sums keep it"""
    from vaehip import ops
    torch.manual_seed(4)
    x = 100.0 + 0.01 * torch.randn((4, 64, 64, 128), device=cuda)
    got = ops.moments(x)
    ref = _ref(x, None, 0)
    errs = _errors(got.cpu(), ref)
    n = x.numel()
    naive_var = (float((x * x).sum()) - float(x.sum()) ** 2 / n) / (n - 1)  # fp32 sums, for the record
    naive = abs(np.sqrt(max(naive_var, 0.0)) - float(ref[2])) / float(ref[2])
    _record("moments/cancellation", {"errors": errs, "naive_fp32_std_rel": naive})
    assert max(errs) <= TOL, errs


def test_moments_repeatable(cuda):
    from vaehip import ops
    torch.manual_seed(6)
    for dt, xf in ((torch.float32, 0), (torch.bfloat16, 2)):
        x = torch.randn((3, 40, 56, 256), device=cuda).to(dt)
        st = _stats(3, 256, cuda, 1) if xf else None
        a = ops.moments(x, st, xf)
        b = ops.moments(x, st, xf)
        assert torch.equal(a, b)
    x = torch.randn((2, 9, 11, 3), device=cuda)
    assert torch.equal(ops.moments(x), ops.moments(x))


# ---------------------------------------------------------------------------------------------------- monitor, golden
def _has_hooks(model):
    return [n for n, m in model.named_modules() if m._forward_hooks or m._forward_pre_hooks]


@pytest.fixture(scope="module")
def golden_device(cuda):
    """test_host_gpu.py's golden scenario with tracking.device_metrics on"""
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    g = json.load(open(os.path.join(G, "e2e_r32.json")))
    tcfg = dict(json.load(open(os.path.join(G, "tracker.json")))["config"], device_metrics=True)
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), 42))
    w.to(cuda)
    tr = HipTrainer(w, lr=g["lr"], lr_warmup_steps=g["warmup"], max_train_steps=g["max_steps"], kl_weight=g["kl_weight"],
                    max_grad_norm=1.0)
    mon = ActivityMonitor(w, tcfg)
    hooks = _has_hooks(w)
    logs = {}
    for s in range(1, 5):
        tr.train_step(vo.synthetic_pixels(g["B"], g["R"], 42, s).to(cuda), vo.synthetic_eps(g["B"], g["R"], 42, s).to(cuda))
        if s == 3:
            w.eval()
            tr.eval_step(vo.synthetic_pixels(g["B"], g["R"], 42, 100).to(cuda))
            w.train()
        lg = mon.step(s)
        if lg:
            logs[str(s)] = lg
    return mon, hooks, logs


def test_golden_with_device_metrics(golden_device):
    mon, hooks, logs = golden_device
    assert mon.device_layers == ["vae.decoder.conv_norm_out.input"]
    assert len(mon.fused_layers) == 3
    assert hooks == []
    ref = json.load(open(os.path.join(G, "tracker.json")))
    arr = np.load(os.path.join(G, "arrays.npz"))
    assert set(logs) == set(ref["step_logs"])
    for s, d in ref["step_logs"].items():
        assert set(d) == set(logs[s])
    per_key = {}
    for key in arr.files:
        if not key.startswith("track/"):
            continue
        _, s, rest = key.split("/", 2)
        lid, metric = rest.rsplit("/", 1)
        got = np.asarray(mon.get_data_for_step(int(s))[lid][metric], dtype=np.float64)
        refv = arr[key].astype(np.float64)
        if metric == "mean_activation":
            scale = max(abs(float(refv)), abs(float(arr[f"track/{s}/{lid}/std_activation"])))
            rel = float(np.max(np.abs(got - refv))) / scale
        else:
            rel = float(np.max(np.abs(got - refv) / (np.abs(refv) + 1e-12)))
        per_key[key] = rel
    _record("golden_device_metrics_rel", per_key)
    assert any("mean_activation" in k for k in per_key) and any("std_activation" in k for k in per_key)
    for key, rel in per_key.items():
        assert rel < 1e-4, (key, rel)
    recs = mon.export_all_processed_data_to_records()
    assert [(r["global_step"], r["layer_identifier"], r["metric_type"]) for r in recs] == \
           [(r["global_step"], r["layer_identifier"], r["metric_type"]) for r in ref["records"]]


# ---------------------------------------------------------------------------------------------- hook path vs device path
POINTS = [("vae.encoder.conv_in", "output"),
          ("vae.encoder.down_blocks.0.resnets.0.norm1", "input"),
          ("vae.encoder.down_blocks.0.resnets.0.norm1", "output"),
          ("vae.encoder.down_blocks.0.resnets.0.conv1", "input"),
          ("vae.decoder.up_blocks.0.upsamplers.0.conv", "output"),
          ("vae.encoder", "input"),
          ("vae.decoder.conv_norm_out", "input")]


def _run(cuda, device_metrics, mixed_precision, checkpoint_decoder):
    import vae_oracle as vo
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    from tracking.monitor import ActivityMonitor
    from vaehip.trainer import HipTrainer
    cfg = {"enabled": True, "track_interval": 2, "device_metrics": device_metrics,
           "target_layers": [{"name": n, "capture_point": p, "metrics": list(ALL4)} for n, p in POINTS]}
    w = SDXLVAEWrapper("synthetic:1")
    w.vae.load_state_dict(vo.synthetic_state_dict(vo.OracleAutoencoderKL(), 7))
    w.to(cuda)
    tr = HipTrainer(w, lr=1e-4, lr_warmup_steps=1, max_train_steps=10, mixed_precision=mixed_precision,
                    checkpoint_decoder=checkpoint_decoder)
    mon = ActivityMonitor(w, cfg)
    counts, logs = {}, {}
    R, B = 64, 2
    for s in range(1, 5):
        tr.train_step(vo.synthetic_pixels(B, R, 5, s).to(cuda), vo.synthetic_eps(B, R, 5, s).to(cuda))
        if s == 3:
            w.eval()
            tr.eval_step(vo.synthetic_pixels(B, R, 5, 100).to(cuda))
            w.train()
        counts[s] = {lid: {m: len(v) for m, v in md.items() if m != "full_activation_map"}
                     for lid, md in mon.hook_collected_buffer.items()}
        lg = mon.step(s)
        if lg:
            logs[s] = lg
    torch.cuda.synchronize()
    data = {s: mon.get_data_for_step(s) for s in (2, 4)}
    return mon, counts, logs, data, mon.export_all_processed_data_to_records()


@pytest.mark.parametrize("mode", ["fp32", "bf16_ckpt"])
def test_hook_path_against_device_path(cuda, mode):
    prec, ckpt = ("no", False) if mode == "fp32" else ("bf16", True)
    mh, ch, lh, dh, rh = _run(cuda, False, prec, ckpt)
    assert mh.device_layers == []
    mh.remove_hooks()
    md, cd, ld, dd, rd = _run(cuda, True, prec, ckpt)
    assert sorted(md.device_layers) == sorted(f"{n}.{p}" for n, p in POINTS)
    assert _has_hooks(md.model) == []
    assert ch == cd  # the same number of buffered forwards per layer and metric
    assert set(lh) == set(ld) == {2, 4}
    worst = {}
    for s in (2, 4):
        assert list(dh[s]) == list(dd[s])
        for lid in dh[s]:
            assert list(dh[s][lid]) == list(dd[s][lid])
            for metric, a in dh[s][lid].items():
                b = dd[s][lid][metric]
                if metric == "full_activation_map":
                    assert isinstance(b, torch.Tensor) and b.dtype == torch.float32
                    assert a.shape == b.shape and a.stride() == b.stride(), (lid, a.stride(), b.stride())
                    assert torch.equal(a, b), lid
                    continue
                a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
                if metric == "mean_activation":
                    scale = max(abs(float(a64)), abs(float(dh[s][lid]["std_activation"])))
                    rel = float(np.abs(a64 - b64)) / scale
                else:
                    rel = float(np.max(np.abs(a64 - b64) / np.abs(a64)))
                worst[f"{s}/{lid}/{metric}"] = rel
        for key, v in lh[s].items():
            assert key in ld[s]
            if "full_activation_map" in key:
                assert ld[s][key] == v, key
    _record(f"hook_vs_device/{mode}", worst)
    for k, rel in worst.items():
        assert rel <= TOL, (k, rel)
    assert [(r["global_step"], r["layer_identifier"], r["original_metric_name"], r["metric_type"]) for r in rh] == \
           [(r["global_step"], r["layer_identifier"], r["original_metric_name"], r["metric_type"]) for r in rd]
    for a, b in zip(rh, rd):
        if a["metric_type"].startswith("full_map_"):
            assert a["metric_value"] == b["metric_value"], a


def test_train_cli_with_all_metrics(cuda, tmp_path):
    """src/train.py with configs/experiment_synthetic_all_metrics.yaml: the CSV carries the rows the hook run writes"""
    import csv
    import yaml
    src = os.path.join(ROOT, "vae-channel-dynamics_amd", "src")
    c = yaml.safe_load(open(os.path.join(ROOT, "vae-channel-dynamics_amd", "configs", "experiment_synthetic_all_metrics.yaml")))
    assert c["tracking"]["device_metrics"] is True
    c["output_dir"] = str(tmp_path)
    c["data"]["dataset_name"] = "synthetic:48"  # 6 steps/epoch x 2 epochs: the tracker fires at step 10
    c["data"]["resolution"] = 32
    cpath = str(tmp_path / "cfg.yaml")
    yaml.safe_dump(c, open(cpath, "w"))
    env = dict(os.environ, PYTHONPATH=src)
    r = subprocess.run([sys.executable, os.path.join(src, "train.py"), "--config_path", cpath], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = list(csv.DictReader(open(tmp_path / c["run_name"] / "tracked_activation_stats.csv")))
    kinds = {(row["layer_identifier"], row["metric_type"]) for row in rows}
    for lid in ("vae.encoder.down_blocks.0.resnets.0.norm1.output", "vae.encoder.down_blocks.0.resnets.0.norm1.input"):
        for k in ("full_map_shape", "full_map_mean", "full_map_std", "full_map_min", "full_map_max"):
            assert (lid, k) in kinds, (lid, k)
    assert ("vae.decoder.conv_norm_out.input", "scalar") in kinds
    assert ("vae.encoder.down_blocks.0.resnets.0.norm1.output", "per_channel_overall_mean") in kinds
    shapes = {row["metric_value"] for row in rows if row["metric_type"] == "full_map_shape"}
    assert shapes == {"(8, 128, 32, 32)"}
