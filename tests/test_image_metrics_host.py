"""vaehip.metrics.ImageMetrics (the accumulation of evaluate.py's image metrics over batches) against a hand computation, and
the library's workspace query for the image-metrics kernel.  Nothing here touches a device."""
import ctypes as C
import math

import pytest
import torch


def test_accumulation_over_unequal_batches():
    """PSNR comes from the summed squared error over the summed element count (not a mean of per-batch PSNRs), SSIM is the
    mean over images, avg_mse = sum of sse_raw / (n * C*H*W)"""
    from vaehip.metrics import ImageMetrics
    numel = 3 * 16 * 16
    batches = [torch.tensor([[7.5, 1.25, 0.91], [3.0, 0.5, 0.97], [9.0, 2.0, 0.80]], dtype=torch.float64),
               torch.tensor([[0.75, 0.125, 0.99]], dtype=torch.float64),
               torch.tensor([[30.0, 6.0, 0.55], [12.0, 3.5, 0.61]], dtype=torch.float64)]
    m = ImageMetrics()
    assert m.compute()["n"] == 0 and math.isnan(m.compute()["psnr"]) and math.isnan(m.compute()["ssim"])
    for t in batches:
        m.update_from(t, numel)
    got = m.compute()
    n = 6
    sse_raw = 7.5 + 3.0 + 9.0 + 0.75 + 30.0 + 12.0
    sse_unit = 1.25 + 0.5 + 2.0 + 0.125 + 6.0 + 3.5
    ssim = 0.91 + 0.97 + 0.80 + 0.99 + 0.55 + 0.61
    assert set(got) == {"n", "avg_mse", "psnr", "ssim"} and got["n"] == n
    assert got["avg_mse"] == pytest.approx(sse_raw / (n * numel), rel=1e-14)
    assert got["psnr"] == pytest.approx(10.0 * math.log10(1.0 / (sse_unit / (n * numel))), rel=1e-14)
    assert got["ssim"] == pytest.approx(ssim / n, rel=1e-14)
    # ... which is not what averaging per-batch figures gives
    per_batch = [10.0 * math.log10(1.0 / (float(t[:, 1].sum()) / (t.shape[0] * numel))) for t in batches]
    assert abs(sum(per_batch) / 3 - got["psnr"]) > 0.1
    assert abs(sum(float(t[:, 2].mean()) for t in batches) / 3 - got["ssim"]) > 0.01
    # identical images: no squared error at all
    z = ImageMetrics()
    z.update_from(torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float64), numel)
    assert z.compute() == {"n": 1, "avg_mse": 0.0, "psnr": float("inf"), "ssim": 1.0}
    with pytest.raises(ValueError):
        m.update_from(torch.zeros(3), numel)


def test_workspace_query_needs_no_gpu():
    from vaehip.lib import lib, VaeHipError
    n = C.c_int64(0)
    lib.call("vae_image_metrics_workspace", 2, 3, 64, 64, C.byref(n))
    assert n.value > 0 and n.value % (2 * 3 * 3) == 0  # three doubles per (image, channel, tile)
    one = C.c_int64(0)
    lib.call("vae_image_metrics_workspace", 1, 3, 64, 64, C.byref(one))
    assert n.value == 2 * one.value
    dll = lib.load()
    for shape in [(2, 3, 10, 64), (2, 3, 64, 10)]:
        rc = dll.vae_image_metrics_workspace(*shape, C.byref(n))
        assert rc == -1 and b"smaller than the 11 x 11" in dll.vae_last_error()  # VAE_EINVAL
    with pytest.raises(VaeHipError, match="image_metrics_workspace"):
        lib.call("vae_image_metrics_workspace", 0, 3, 64, 64, C.byref(n))
    # the launch entry points refuse the same shapes on the host, before any launch
    with pytest.raises(VaeHipError, match="smaller than"):
        lib.call("vae_image_metrics_final", C.c_void_p(8), 1, 3, 10, 64, C.c_void_p(8), None)
    with pytest.raises(VaeHipError, match="null args"):
        lib.call("vae_image_metrics_partial", None, 0, 0, 0, 0, None, 0, 0, 0, 0, 1, 3, 64, 64, None, None)


def test_wrapper_refuses_before_the_library_is_asked():
    from vaehip import ops
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="one GPU"):  # CPU tensors: no fallback
        ops.image_metrics(x, x)
    with pytest.raises(ValueError, match="one shape"):
        ops.image_metrics(x, x[:, :2])
    with pytest.raises(ValueError, match="float32"):
        ops.image_metrics(x.double(), x.double())
