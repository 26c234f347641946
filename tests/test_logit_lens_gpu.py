"""The logit-lens kernels (csrc/lens.hip), their wrappers and the analyzer on the device, against tests/lens_refs.py: maps and
ranges bit-identical to the source values, the display normalisation bit-identical to torch's fp32 expression on the CPU, the
mini-decoder projection within the bound derived from its float64 reference; the same calls in guarded, poisoned memory;
the model boundary and the two command-line tools end to end."""
import os
import subprocess
import sys

import pytest
import torch

import lens_refs as R
from guarded import GuardedPool, guarded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vae-channel-dynamics_amd")
LENS_LAYERS = ["encoder.down_blocks.0.resnets.0.norm1", "encoder.down_blocks.1.resnets.0.conv_shortcut"]


def _idx(ch, dev):
    return torch.tensor(ch, dtype=torch.int32, device=dev)


def _check_planes(got, x_cpu, S, ch, what):
    maps, rng, norm = (t.cpu() for t in got)
    rmaps, rrng, rnorm = R.planes_ref(x_cpu, S, ch)
    assert maps.dtype == rng.dtype == norm.dtype == torch.float32
    assert maps.shape == rmaps.shape and rng.shape == rrng.shape and norm.shape == rnorm.shape, what
    assert torch.equal(maps, rmaps), (what, "maps")
    assert torch.equal(rng, rrng), (what, "range")
    assert torch.equal(norm, rnorm), (what, "norm", float((norm - rnorm).abs().max()))
    flat = (rrng[..., 1] - rrng[..., 0]) <= 1e-6
    assert bool((norm[flat] == 0).all()), (what, "flat planes")


def _check_project(got, x_cpu, S, ch, full_map, w, what):
    ref, tol = R.project_ref(R.project_inputs(x_cpu, S, ch, full_map), *w)
    got = got.cpu()
    assert got.dtype == torch.float32
    assert got.shape == ((S, *ref.shape[1:]) if full_map else (S, len(ch), *ref.shape[1:])), (what, got.shape)
    err = (got.double().reshape(ref.shape) - ref).abs()
    ratio = float((err / tol).max())
    print(f"{what}: max error {float(err.max()):.3e}, worst error / bound {ratio:.3f}")
    assert bool((err <= tol).all()), (what, float(err.max()), ratio)


def test_tile_edge(cuda):
    """the map sizes of lens_refs sit on the kernel's real tile edge"""
    from vaehip.lib import lib
    assert lib.query("vae_lens_tile") == R.T
    assert (R.T, R.T) in R.MAP_SIZES and (R.T + 1, R.T) in R.MAP_SIZES and (R.T + 1, R.T + 1) in R.MAP_SIZES


@pytest.mark.parametrize("case", R.plane_cases(), ids=R.case_id)
def test_planes_and_single_channel_projection(cuda, case):
    from vaehip import ops
    H, W, cc, B, S, bf16 = case
    buf, Cn = R.make_input(H, W, cc, B, bf16)
    x_cpu = buf[..., :Cn]
    x = buf.to(cuda)[..., :Cn]  # "3of4": a channel-prefix view with pixel stride 4
    w = R.decoder_weights(1)
    wd = [t.to(cuda) for t in w]
    for ch in R.channel_lists(Cn):
        what = f"{R.case_id(case)} channels {ch}"
        _check_planes(ops.lens_planes(x, S, _idx(ch, cuda), ch), x_cpu, S, ch, what)
        _check_project(ops.lens_project(x, S, _idx(ch, cuda), *wd, False, ch), x_cpu, S, ch, False, w, what)


@pytest.mark.parametrize("case", R.full_map_cases(), ids=R.case_id)
def test_full_map_projection(cuda, case):
    from vaehip import ops
    Cn, H, W, B, S, bf16 = case
    x_cpu, _ = R.make_input(H, W, str(Cn), B, bf16)
    x = x_cpu.to(cuda)
    w = R.decoder_weights(Cn)
    ch = list(range(Cn))
    got = ops.lens_project(x, S, _idx(ch, cuda), *[t.to(cuda) for t in w], True, ch)
    _check_project(got, x_cpu, S, ch, True, w, R.case_id(case))
    if Cn == 4:  # the list's order is the input's channel order
        ch = [3, 0, 2, 1]
        got = ops.lens_project(x, S, _idx(ch, cuda), *[t.to(cuda) for t in w], True)
        _check_project(got, x_cpu, S, ch, True, w, R.case_id(case) + " permuted")


@pytest.mark.parametrize("H,W", [(1, 1), (17, 13), (40, 33)])
def test_flat_planes_normalise_to_zero(cuda, H, W):
    """a constant plane, one whose spread is 5e-7, one just above the 1e-6 threshold and an ordinary one (40 x 33: two chunks)"""
    from vaehip import ops
    g = torch.Generator().manual_seed(H)
    x = torch.randn(2, H, W, 4, generator=g) * 10.0
    x[..., 0] = 3.25
    x[..., 1] = torch.rand(2, H, W, generator=g) * 5e-7
    x[..., 2] = torch.rand(2, H, W, generator=g) * 2e-6
    if H * W > 1:
        x[:, 0, 0, 1], x[:, -1, -1, 1] = 0.0, 5e-7
        x[:, 0, 0, 2], x[:, -1, -1, 2] = 0.0, 2e-6
    ch = [0, 1, 2, 3]
    got = ops.lens_planes(x.to(cuda), 2, _idx(ch, cuda), ch)
    _check_planes(got, x, 2, ch, f"flat {H}x{W}")
    norm = got[2].cpu()
    assert float(norm[:, :2].abs().max()) == 0.0
    if H * W > 1:
        assert float(norm[:, 2].max()) == 1.0 and float(norm[:, 3].max()) == 1.0 and float(norm[:, 2:].min()) == 0.0


GUARDED_CASES = [(1, 1, "1", 1, 1, False), (1, 5, "3of4", 3, 1, True), (R.T, R.T, "4", 3, 1, False), (R.T + 1, R.T + 1, "128", 3, 1, True),
                 (17, 13, "3of4", 3, 3, False), (R.T + 1, R.T, "128", 1, 1, False)]


@pytest.mark.parametrize("case", GUARDED_CASES, ids=R.case_id)
def test_guarded(cuda, case):
    """operands, results and workspaces between poisoned guards: nothing is stored outside a result, every element of every
    result and workspace is written, and a load past the last row, column or sample (the high-side halo) would poison a value"""
    from vaehip import ops
    H, W, cc, B, S, bf16 = case
    buf, Cn = R.make_input(H, W, cc, B, bf16)
    x_cpu = buf[..., :Cn]
    pool = GuardedPool("cuda")
    x = pool.put(buf, "x")[..., :Cn]
    w1 = R.decoder_weights(1)
    wf = R.decoder_weights(Cn)
    w1d = [pool.put(t, f"w1_{i}") for i, t in enumerate(w1)]
    wfd = [pool.put(t, f"wf_{i}") for i, t in enumerate(wf)]
    lists = R.channel_lists(Cn)
    idx = [pool.put(torch.tensor(ch, dtype=torch.int32), f"channels{i}") for i, ch in enumerate(lists)]
    full = list(range(Cn))
    idx_full = pool.put(torch.tensor(full, dtype=torch.int32), "channels_full")
    pool.snapshot()
    with guarded(pool, ops):
        planes = [ops.lens_planes(x, S, i, ch) for i, ch in zip(idx, lists)]
        single = [ops.lens_project(x, S, i, *w1d, False, ch) for i, ch in zip(idx, lists)]
        fullmap = ops.lens_project(x, S, idx_full, *wfd, True, full)
    torch.cuda.synchronize()
    viol, changed, unwritten = pool.violations(), pool.changed(), pool.unwritten_report()
    print(f"{R.case_id(case)}: {len(pool.blocks)} blocks; violations {viol}; changed {changed}; unwritten {unwritten}")
    assert viol == [] and changed == [] and unwritten == [], (viol, changed, unwritten)
    for ch, p, s in zip(lists, planes, single):
        _check_planes(p, x_cpu, S, ch, f"guarded {ch}")
        _check_project(s, x_cpu, S, ch, False, w1, f"guarded single {ch}")
    _check_project(fullmap, x_cpu, S, full, True, wf, "guarded full map")


def test_analyzer_takes_both_forms_of_an_activation(cuda, tmp_path):
    """a device NHWC tensor (fp32 and bf16) and the CPU (B, C, H, W) tensor of the same values give the same tensors; only the
    planes that are drawn leave the host; weights loaded into mini_decoder are the ones used"""
    from analysis.logit_lens import VAELogitLens
    torch.manual_seed(5)
    lens = VAELogitLens(logit_lens_config={"mini_decoder_input_channels": 1}, main_experiment_output_dir=str(tmp_path))
    x_cpu, _ = R.make_input(R.T + 1, 11, "128", 3, False)
    nchw = x_cpu.permute(0, 3, 1, 2)
    ch = [127, 0, 64]
    w = [p.detach().clone() for p in (lens.mini_decoder[0].weight, lens.mini_decoder[0].bias, lens.mini_decoder[2].weight, lens.mini_decoder[2].bias)]
    a = lens.channel_maps(x_cpu.to(cuda), 2, ch)
    b = lens.channel_maps(nchw, 2, ch)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    _check_planes(a, x_cpu, 2, ch, "analyzer")
    pa, pb = lens.project(x_cpu.to(cuda), 2, ch), lens.project(nchw, 2, ch)
    assert torch.equal(pa, pb)
    _check_project(pa, x_cpu, 2, ch, False, w, "analyzer single")
    x16 = x_cpu.to(torch.bfloat16)
    _check_planes(lens.channel_maps(x16.to(cuda), 3, ch), x16, 3, ch, "analyzer bf16")
    new = R.decoder_weights(1, seed=99)
    lens.mini_decoder.load_state_dict({"0.weight": new[0], "0.bias": new[1], "2.weight": new[2], "2.bias": new[3]})
    _check_project(lens.project(nchw, 1, ch), x_cpu, 1, ch, False, new, "analyzer reloaded weights")
    full = VAELogitLens(logit_lens_config={"mini_decoder_input_channels": 128}, main_experiment_output_dir=str(tmp_path))
    wf = [p.detach().clone() for p in (full.mini_decoder[0].weight, full.mini_decoder[0].bias, full.mini_decoder[2].weight, full.mini_decoder[2].bias)]
    _check_project(full.project(nchw, 2, range(128), "mini_decoder_full_map"), x_cpu, 2, list(range(128)), True, wf, "analyzer full map")
    # pictures from a device tensor, all four kinds
    lens.visualize_channel_activation_maps(x_cpu.to(cuda), "enc.norm1", 7, num_channels_to_viz=1, num_batch_samples_to_viz=2)
    lens.run_logit_lens_with_activations(7, ["enc.norm1"], 1, "mini_decoder_single_channel", {"enc.norm1": x_cpu.to(cuda)})
    full.run_logit_lens_with_activations(7, ["enc.norm1"], 2, "mini_decoder_full_map", {"enc.norm1": nchw})
    lens.project_with_mini_decoder(x_cpu.to(cuda), "enc.norm1", 7, channel_idx=127, sample_idx=2)
    base = tmp_path / "logit_lens_visualizations" / "step_7" / "enc_norm1"
    for rel in ("sample_0_all_channels.png", "sample_1_all_channels.png", "logit_lens_projections/lens_sample_0_single_channel_projections_combined.png",
                "logit_lens_projections/lens_sample_0_full_map.png", "logit_lens_projections/lens_sample_1_full_map.png",
                "mini_decoded/sample_2_channel_127_projected.png"):
        assert (base / rel).is_file() and (base / rel).stat().st_size > 0, rel
    from PIL import Image
    import numpy as np
    png = np.asarray(Image.open(base / "mini_decoded" / "sample_2_channel_127_projected.png"))
    ref, _ = R.project_ref(R.project_inputs(x_cpu[2:3], 1, [127], False), *new)
    assert png.shape == (4 * (R.T + 1), 44, 3) and int(np.abs(png.astype(int) - (ref[0] * 255).round().numpy().astype(int)).max()) <= 1


def test_model_boundary_captures_on_the_device(cuda, tmp_path):
    """add_device_captures on the two default lens layers of a synthetic model: device fp32 NHWC snapshots whose maps are bit for
    bit, and whose projections within the bound of, what the add_hooks path captures in a second identical forward"""
    from analysis.logit_lens import VAELogitLens
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    import vae_oracle as vo
    w = SDXLVAEWrapper("synthetic:3")
    w.to(cuda)
    w.vae.eval()
    x = vo.synthetic_pixels(2, 32, 11).to(cuda)
    with torch.no_grad():
        w.add_device_captures(LENS_LAYERS)
        w(x, sample_posterior=False)
        dev = dict(w.get_captured_activations())
        w.remove_hooks()
        assert w.get_captured_activations() == {}
        w.add_hooks(LENS_LAYERS)
        w(x, sample_posterior=False)
        host = dict(w.get_captured_activations())
        w.remove_hooks()
        w(x, sample_posterior=False)  # nothing is registered any more
        assert w.get_captured_activations() == {}
    assert sorted(dev) == sorted(host) == sorted(LENS_LAYERS)
    torch.manual_seed(3)
    lens = VAELogitLens(model_for_lens=w.vae, main_experiment_output_dir=str(tmp_path))
    wts = [p.detach().clone() for p in (lens.mini_decoder[0].weight, lens.mini_decoder[0].bias, lens.mini_decoder[2].weight, lens.mini_decoder[2].bias)]
    for name in LENS_LAYERS:
        d, h = dev[name], host[name]
        assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous() and not h.is_cuda
        assert tuple(d.shape) == (h.shape[0], h.shape[2], h.shape[3], h.shape[1]), (name, d.shape, h.shape)
        assert lens.get_layer_logit_length(d, name) == lens.get_layer_logit_length(h, name) == h.shape[1]
        nhwc = h.float().permute(0, 2, 3, 1)
        ch = [0, 1, 2, h.shape[1] - 1]
        _check_planes(lens.channel_maps(d, 2, ch), nhwc, 2, ch, name)
        _check_project(lens.project(d, 2, ch), nhwc, 2, ch, False, wts, name)


def _run(cmd, cwd, timeout=600):
    r = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, cwd=str(cwd), timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r


def test_evaluate_draws_the_first_batch(cuda, tmp_path):
    """evaluate.py on a tiny synthetic checkpoint: the lens's pictures under logit_lens_visualizations_eval/step_0/<layer>/, and
    first_batch_activations.pt with the keys and logical (B, C, H, W) fp32 CPU tensors the hook path wrote -- or, switched off, absent"""
    from models.sdxl_vae_wrapper import SDXLVAEWrapper
    ckpt = tmp_path / "ckpt"
    w = SDXLVAEWrapper("synthetic:42")
    w.vae.save_pretrained(str(ckpt / "vae"))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("model:\n  pretrained_vae_name: \"synthetic:42\"\ndata:\n  dataset_name: \"synthetic:8\"\n  resolution: 32\n  batch_size: 4\n"
                   "  num_workers: 0\nlogit_lens:\n  num_channels_to_viz: 3\n  colormap: magma\n")
    base = [os.path.join(PKG, "src", "evaluate.py"), "--config_path", str(cfg), "--checkpoint_path", str(ckpt), "--eval_split", "train",
            "--num_samples_to_save", "1", "--logit_lens_num_samples", "2"]
    _run(base + ["--output_dir", str(tmp_path / "a")], tmp_path)
    for layer in LENS_LAYERS:
        d = tmp_path / "a" / "logit_lens_visualizations_eval" / "step_0" / layer.replace(".", "_")
        for rel in ("sample_0_all_channels.png", "sample_1_all_channels.png",
                    "logit_lens_projections/lens_sample_0_single_channel_projections_combined.png",
                    "logit_lens_projections/lens_sample_1_single_channel_projections_combined.png"):
            assert (d / rel).is_file() and (d / rel).stat().st_size > 0, (layer, rel)
    acts = torch.load(str(tmp_path / "a" / "first_batch_activations.pt"))
    assert sorted(acts) == sorted(LENS_LAYERS)
    # what the hook path captures for the same checkpoint and batch: same keys, shapes, dtype, device -- and values
    w.to(cuda)
    w.vae.eval()
    from data_utils import create_dataloader, load_and_preprocess_dataset
    ds = load_and_preprocess_dataset(dataset_name="synthetic:8", dataset_config_name=None, image_column="image", resolution=32,
                                     max_samples=None, split="train")
    batch = next(iter(create_dataloader(ds, batch_size=4, num_workers=0, shuffle=False)))
    with torch.no_grad():
        w.add_hooks(LENS_LAYERS)
        w(batch["pixel_values"].to(cuda, dtype=torch.float32), sample_posterior=False)
        hooked = dict(w.get_captured_activations())
        w.remove_hooks()
    for k, v in hooked.items():
        assert acts[k].shape == v.shape and acts[k].dtype == v.dtype == torch.float32 and not acts[k].is_cuda, k
        assert torch.equal(acts[k], v), k
    assert (tmp_path / "a" / "eval_metrics.txt").is_file()
    _run(base + ["--output_dir", str(tmp_path / "b"), "--save_first_batch_activations", "false", "--logit_lens_projection_type",
                 "mini_decoder_full_map", "--logit_lens_mini_decoder_input_channels", "128", "--logit_lens_layers", LENS_LAYERS[0]], tmp_path)
    assert not (tmp_path / "b" / "first_batch_activations.pt").exists()
    d = tmp_path / "b" / "logit_lens_visualizations_eval" / "step_0" / LENS_LAYERS[0].replace(".", "_")
    assert (d / "sample_0_all_channels.png").is_file() and (d / "logit_lens_projections" / "lens_sample_1_full_map.png").is_file()


def test_train_draws_at_the_lens_interval(cuda, tmp_path):
    """train.py on configs/experiment_synthetic_logit_lens.yaml: channel maps and projections of both tracked targets (one named
    with the `.full_activation_map` suffix, one without) at every lens interval"""
    import yaml
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "experiment_synthetic_logit_lens.yaml")))
    cfg["output_dir"] = str(tmp_path / "run")
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    _run([os.path.join(PKG, "src", "train.py"), "--config_path", str(path)], tmp_path)
    steps = 16 // 4
    interval = cfg["logit_lens"]["visualization_interval"]
    assert interval == cfg["tracking"]["track_interval"]
    hits = []
    for dirpath, _, files in os.walk(str(tmp_path / "run")):
        hits += [os.path.join(dirpath, f) for f in files if f.endswith(".png")]
    for step in range(interval, steps + 1, interval):
        for layer in ("vae_encoder_down_blocks_0_resnets_0_norm1_output", "vae_encoder_conv_in_output"):
            for rel in ("sample_0_all_channels.png", os.path.join("logit_lens_projections", "lens_sample_0_single_channel_projections_combined.png")):
                want = os.path.join("logit_lens_visualizations", f"step_{step}", layer, rel)
                assert any(h.endswith(want) for h in hits), (want, hits)
