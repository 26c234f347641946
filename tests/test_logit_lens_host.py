"""analysis.logit_lens.VAELogitLens and the lens entry points of the library, as far as they go without a device: the
mini-decoder's weights, the directory and naming contract, rendering from host arrays, the fairness condition of the projection
bound (tests/lens_refs.py), argument checks of the C ABI and of the wrappers, and evaluate.py's flag check."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lens_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vae-channel-dynamics_amd")


def _lens(tmp_path, **cfg):
    from analysis.logit_lens import VAELogitLens
    return VAELogitLens(logit_lens_config=cfg or None, main_experiment_output_dir=str(tmp_path))


@pytest.mark.parametrize("cin", [1, 128])
def test_mini_decoder_draws_the_weights_of_the_four_modules(tmp_path, cin):
    """same modules in the same order: under one seed the analyzer's mini-decoder holds what torch gives the modules built directly"""
    torch.manual_seed(1234)
    lens = _lens(tmp_path, mini_decoder_input_channels=cin)
    torch.manual_seed(1234)
    up = dict(kernel_size=3, stride=2, padding=1, output_padding=1)
    ref = torch.nn.Sequential(torch.nn.ConvTranspose2d(cin, 16, **up), torch.nn.ReLU(), torch.nn.ConvTranspose2d(16, 3, **up),
                              torch.nn.Sigmoid())
    assert [type(m) for m in lens.mini_decoder] == [type(m) for m in ref]
    assert lens.mini_decoder[0].in_channels == cin
    got, want = lens.mini_decoder.state_dict(), ref.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert all(p.device.type == "cpu" for p in lens.mini_decoder.parameters())
    lens.mini_decoder.load_state_dict(want)  # a user can load weights into it


def test_constructor_needs_no_gpu_and_creates_the_directory(tmp_path):
    lens = _lens(tmp_path, visualization_output_subdir="lens_out")
    assert lens.visualization_base_dir == os.path.join(str(tmp_path), "lens_out") and os.path.isdir(lens.visualization_base_dir)
    assert (lens.default_num_channels, lens.default_batch_samples, lens.mini_decoder[0].in_channels) == (4, 1, 1)
    default = _lens(tmp_path / "d")
    assert default.visualization_base_dir.endswith("logit_lens_visualizations") and os.path.isdir(default.visualization_base_dir)


def test_layer_names_and_logit_length(tmp_path):
    lens = _lens(tmp_path)
    assert lens._get_safe_layer_name("vae.encoder/down_blocks.0.norm1") == "vae_encoder_down_blocks_0_norm1"
    assert lens.get_layer_logit_length(torch.zeros(2, 5, 3, 4), "l") == 5  # a CPU tensor is (B, C, H, W)
    assert lens.get_layer_logit_length(torch.zeros(5, 3, 4), "l") is None
    assert lens.get_layer_logit_length(np.zeros((2, 5, 3, 4)), "l") is None
    assert lens.get_layer_logit_length(None, "l") is None
    # the skip paths that need no device: not 4-D, no activations, a layer without one
    lens.visualize_channel_activation_maps(torch.zeros(3, 4), "l", 0)
    lens.run_logit_lens_with_activations(0, ["l"], 1, "mini_decoder_single_channel", {})
    lens.run_logit_lens_with_activations(0, ["missing"], 1, "mini_decoder_single_channel", {"l": torch.zeros(1, 1, 2, 2)})
    assert os.listdir(lens.visualization_base_dir) == []


def test_rendering_from_host_arrays(tmp_path, monkeypatch):
    """the four file names of the reference's layout, written from synthetic host arrays, with the expected number of subplots"""
    from PIL import Image

    from analysis import logit_lens as L
    g = np.random.default_rng(0)
    step = tmp_path / "step_3" / "enc_norm1"
    (step / "logit_lens_projections").mkdir(parents=True)
    (step / "mini_decoded").mkdir()
    p = str(step / "sample_0_all_channels.png")
    assert L.render_channel_maps(g.random((4, 6, 5), dtype=np.float32), p, "viridis") == 4 and os.path.getsize(p) > 0
    p1 = str(step / "sample_1_all_channels.png")
    assert L.render_channel_maps(g.random((1, 6, 5), dtype=np.float32), p1, "magma") == 1 and os.path.getsize(p1) > 0  # bare `axes`
    p = str(step / "logit_lens_projections" / "lens_sample_0_single_channel_projections_combined.png")
    assert L.render_single_channel_projections(g.random((3, 8, 8, 3), dtype=np.float32), p) == 3 and os.path.getsize(p) > 0
    p = str(step / "logit_lens_projections" / "lens_sample_0_single_channel_projections_combined_1.png")
    assert L.render_single_channel_projections(g.random((1, 8, 8, 3), dtype=np.float32), p) == 1
    img = g.random((8, 12, 3), dtype=np.float32)
    img[0, 0], img[0, 1] = (0.0, 1.0, 0.5), (0.498, 0.502, 0.25)
    for p in (str(step / "logit_lens_projections" / "lens_sample_0_full_map.png"), str(step / "mini_decoded" / "sample_0_channel_2_projected.png")):
        L.save_projection_png(img, p)
        back = np.asarray(Image.open(p))
        assert back.shape == (8, 12, 3) and back.dtype == np.uint8
        assert np.array_equal(back, (torch.from_numpy(img) * 255).round().byte().numpy())  # evaluate.save_png's definition
    import matplotlib.pyplot as plt
    assert plt.get_fignums() == []  # every figure is closed
    # matplotlib missing: a clear error when a figure is rendered (the module itself imported fine above)
    import builtins
    real = builtins.__import__

    def no_matplotlib(name, *a, **k):
        if name.split(".")[0] == "matplotlib":
            raise ImportError("No module named 'matplotlib'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_matplotlib)
    with pytest.raises(RuntimeError, match="matplotlib"):
        L.render_channel_maps(np.zeros((1, 2, 2), dtype=np.float32), str(step / "never.png"))
    assert not (step / "never.png").exists()


def _projection_cases():
    """every (input, channel list, mode) the GPU test projects, as (id, NCHW input, weights)"""
    for case in R.plane_cases():
        H, W, cc, B, S, bf16 = case
        x, Cn = R.make_input(H, W, cc, B, bf16)
        for ch in R.channel_lists(Cn):
            yield f"single-{R.case_id(case)}-{ch}", R.project_inputs(x[..., :Cn], S, ch, False), R.decoder_weights(1)
    for case in R.full_map_cases():
        Cn, H, W, B, S, bf16 = case
        x, _ = R.make_input(H, W, str(Cn), B, bf16)
        yield f"full-{R.case_id(case)}", R.project_inputs(x, S, list(range(Cn)), True), R.decoder_weights(Cn)


def test_the_projection_bound_is_fair_to_fp32():
    """the condition of the derived bound: torch's own fp32 mini-decoder stays inside it on every input of the GPU test"""
    worst = {}
    n = 0
    for cid, x, w in _projection_cases():
        ref, tol = R.project_ref(x, *w)
        err = (R.project_fp32_torch(x, *w).double() - ref).abs()
        assert bool((err <= tol).all()), (cid, float(err.max()), float(tol.min()))
        key = cid.split("-")[0] + "-C" + str(x.shape[1])
        worst[key] = max(worst.get(key, 0.0), float(err.max()))
        n += 1
    print(f"{n} projections; worst fp32 error by mode and Cin: {worst}")
    assert n > 100


def test_the_bound_sees_a_wrong_tap_a_missing_halo_and_a_dropped_channel():
    x, _ = R.make_input(R.T + 1, R.T + 1, "4", 1, False)
    xin = R.project_inputs(x, 1, [0, 1, 2, 3], True)
    w = R.decoder_weights(4)
    ref, tol = R.project_ref(xin, *w)
    flipped = [w[0].flip(3).contiguous()] + w[1:]             # taps 0 and 2 of a row exchanged
    no_halo = xin.clone()
    no_halo[:, :, R.T, :] = 0                                 # the row a tile's high-side halo brings in
    dropped = xin.clone()
    dropped[:, 3] = 0
    for what, got in (("tap", R.project_ref(xin, *flipped)[0]), ("halo", R.project_ref(no_halo, *w)[0]), ("channel", R.project_ref(dropped, *w)[0])):
        assert float(((got - ref).abs() / tol).max()) > 1e3, what


def test_workspace_query_and_argument_checks_need_no_gpu():
    from vaehip.lib import lib, VaeHipError
    dll = lib.load()
    assert lib.query("vae_lens_tile") == R.T
    n, one = C.c_int64(0), C.c_int64(0)
    lib.call("vae_lens_workspace", 2, 3, 64, 64, C.byref(n))
    lib.call("vae_lens_workspace", 1, 3, 64, 64, C.byref(one))
    assert n.value > 0 and n.value == 2 * one.value and n.value % (2 * 3 * 2) == 0
    with pytest.raises(VaeHipError, match="null result"):
        lib.call("vae_lens_workspace", 1, 1, 4, 4, None)
    p = C.c_void_p(256)  # stands for device memory: an argument error returns before anything dereferences or launches
    ok_list = (C.c_int32 * 2)(0, 3)

    def planes(x=p, B=2, H=4, W=5, Cc=4, ld=4, S=2, ch=p, host=ok_list, K=2, maps=p, ws=p):
        return dll.vae_lens_planes_partial(x, 0, B, H, W, Cc, ld, S, ch, host, K, maps, ws, None)

    def project(x=p, B=2, H=4, W=5, Cc=4, ld=4, S=2, ch=p, host=ok_list, K=2, w1=p, b1=p, w2=p, b2=p, out=p):
        return dll.vae_lens_project(x, 0, B, H, W, Cc, ld, S, ch, host, K, 0, w1, b1, w2, b2, out, None)

    bad = [(dict(x=None), b"null args"), (dict(ch=None), b"null args"), (dict(S=3), b"1 <= S <= B"), (dict(S=0), b"1 <= S <= B"),
           (dict(K=0, host=None), b"K >= 1"), (dict(H=0), b"H >= 1"), (dict(W=0), b"W >= 1"), (dict(ld=3), b"ld >= C"),
           (dict(host=(C.c_int32 * 2)(0, 4)), b"outside [0, 4)"), (dict(host=(C.c_int32 * 2)(-1, 0)), b"outside [0, 4)")]
    for fn, extra in ((planes, [(dict(maps=None), b"null args"), (dict(ws=None), b"null args")]),
                      (project, [(dict(w1=None), b"null args"), (dict(b2=None), b"null args"), (dict(out=None), b"null args")])):
        for kw, msg in bad + extra:
            assert fn(**kw) == -1 and msg in dll.vae_last_error(), (fn.__name__, kw, dll.vae_last_error())
    assert dll.vae_lens_planes_final(None, p, 1, 1, 4, 4, p, p, None) == -1 and b"null args" in dll.vae_last_error()
    assert dll.vae_lens_planes_final(p, p, 1, 0, 4, 4, p, p, None) == -1 and b"K >= 1" in dll.vae_last_error()
    assert dll.vae_lens_planes_final(p, p, 1, 1, 4, 0, p, p, None) == -1 and b"W >= 1" in dll.vae_last_error()


def test_wrappers_refuse_before_the_library_is_asked(tmp_path):
    from vaehip import ops
    x = torch.zeros(2, 4, 5, 3)
    idx = torch.zeros(1, dtype=torch.int32)
    w = R.decoder_weights(1)
    with pytest.raises(ValueError, match="CUDA tensor"):  # CPU tensors: no fallback
        ops.lens_planes(x, 1, idx)
    with pytest.raises(ValueError, match="CUDA tensor"):
        ops.lens_project(x, 1, idx, *w, False)
    lens = _lens(tmp_path, mini_decoder_input_channels=8)
    with pytest.raises(ValueError, match="expects 8 input channels"):
        lens.project(torch.zeros(1, 4, 3, 3), 1, [0, 1, 2, 3], "mini_decoder_full_map")
    with pytest.raises(ValueError, match="expects 8 input channels"):
        lens.project(torch.zeros(1, 4, 3, 3), 1, [0], "mini_decoder_single_channel")
    with pytest.raises(ValueError, match="Unknown projection_type"):
        lens.project(torch.zeros(1, 4, 3, 3), 1, [0], "pca")
    with pytest.raises(ValueError, match="do not fit"):
        _lens(tmp_path).channel_maps(torch.zeros(1, 4, 3, 3), 1, [4])
    with pytest.raises(ValueError, match="do not fit"):
        _lens(tmp_path).channel_maps(torch.zeros(1, 4, 3, 3), 2, [0])


def test_evaluate_refuses_full_map_without_the_channel_count(tmp_path):
    """exit status 1 from the flag check, before a checkpoint is opened or a device asked for"""
    r = subprocess.run([sys.executable, os.path.join(PKG, "src", "evaluate.py"), "--config_path",
                        os.path.join(PKG, "configs", "experiment_synthetic_logit_lens.yaml"), "--checkpoint_path", str(tmp_path / "none"),
                        "--logit_lens_projection_type", "mini_decoder_full_map"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 1, r.stderr[-2000:]
    assert "--logit_lens_mini_decoder_input_channels must be specified" in r.stderr + r.stdout
    assert "no GPU visible" not in r.stderr + r.stdout and not (tmp_path / "none").exists()
