"""References, bounds and cases shared by tests/test_logit_lens_host.py and tests/test_logit_lens_gpu.py (a helper module, not a
test).

Projection reference: torch.nn.functional.conv_transpose2d / relu / sigmoid on the CPU in float64, the functions behind the
modules the reference's VAELogitLens is built from.  Its bound is derived, not measured: with u = 2^-24, n1 = 4 Cin + 1 and
n2 = 65 (a stride-2 3x3 transposed convolution sums at most 4 taps per input channel, plus the bias)
    err_h   = (n1 + 2) u sum|x w1|                      at each hidden element (ReLU is 1-Lipschitz)
    err_pre = (n2 + 2) u sum|h w2| + sum|w2| err_h      at each output element before the sigmoid
    tol     = err_pre / 4 + 4 u                         (sigmoid is 1/4-Lipschitz; its evaluation costs a few ulp of a value <= 1)
Normalisation reference: torch's own fp32 (x - x.min()) / (x.max() - x.min()) on the CPU; the kernel makes the same one IEEE
subtraction and one IEEE division, so the results are compared bit for bit.
"""
import itertools

import torch
import torch.nn.functional as F

U = 2.0 ** -24
CT = dict(stride=2, padding=1, output_padding=1)
T = 8  # input tile edge of the projection kernel (held to the library by test_tile_edge)

MAP_SIZES = [(1, 1), (1, 5), (3, 7), (T, T), (T + 1, T), (T + 1, T + 1), (17, 13)]
BATCHES = [(1, 1), (3, 1), (3, 3)]             # (B, S)
CHANNELS = ["1", "3of4", "4", "128"]           # "3of4": the [..., :3] prefix of a 4-wide buffer
FULL_MAP_CASES = [(4, (T + 1, T)), (4, (3, 7)), (128, (T + 1, T)), (128, (1, 1)), (512, (T + 1, T)), (512, (1, 5))]  # (C, map)


def channel_lists(C):
    """[0], [C - 1], the first 4, and a list that is not monotonic (with a repeat where C allows one)"""
    lists = [[0], [C - 1], list(range(min(4, C)))]
    lists.append([C - 1, 0, C // 2, 0] if C > 1 else [0, 0])
    out = []
    for l in lists:
        if l not in out:
            out.append(l)
    return out


def plane_cases():
    """(H, W, channel config, B, S, bf16): every map size with every channel config and storage; (B, S) rotates"""
    cases = []
    for i, ((H, W), cc, bf16) in enumerate(itertools.product(MAP_SIZES, CHANNELS, (False, True))):
        B, S = BATCHES[i % len(BATCHES)]
        cases.append((H, W, cc, B, S, bf16))
    return cases


def full_map_cases():
    """(C, H, W, B, S, bf16)"""
    cases = []
    for i, ((C, (H, W)), bf16) in enumerate(itertools.product(FULL_MAP_CASES, (False, True))):
        B, S = BATCHES[(i + 1) % len(BATCHES)]
        cases.append((C, H, W, B, S, bf16))
    return cases


def case_id(case):
    return "-".join("bf16" if v is True else "f32" if v is False else str(v) for v in case)


def make_input(H, W, cc, B, bf16, seed=0):
    """-> (the NHWC CPU tensor as stored, possibly a channel-prefix view, its channel count): seeded normal values scaled by 10"""
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B + seed)
    wide = 4 if cc == "3of4" else int(cc)
    buf = (torch.randn(B, H, W, wide, generator=g) * 10.0)
    if bf16:
        buf = buf.to(torch.bfloat16)
    C = 3 if cc == "3of4" else wide
    return buf, C


def decoder_weights(cin, seed=7):
    """the four parameters of VAELogitLens(...).mini_decoder under a fixed seed (torch's default initialisation)"""
    torch.manual_seed(seed)
    w = [torch.nn.ConvTranspose2d(cin, 16, 3, **CT), torch.nn.ConvTranspose2d(16, 3, 3, **CT)]
    return [w[0].weight.detach(), w[0].bias.detach(), w[1].weight.detach(), w[1].bias.detach()]


def planes_ref(x_nhwc, S, channels):
    """-> (maps [S, K, H, W], range [S, K, 2], norm [S, K, H, W]) in fp32 from the CPU tensor as stored"""
    maps = x_nhwc[:S].float()[..., channels].permute(0, 3, 1, 2).contiguous()
    mn, mx = maps.amin(dim=(2, 3)), maps.amax(dim=(2, 3))
    norm = torch.zeros_like(maps)
    for s in range(maps.shape[0]):
        for k in range(maps.shape[1]):
            p = maps[s, k]
            if p.max() - p.min() > 1e-6:
                norm[s, k] = (p - p.min()) / (p.max() - p.min())
    return maps, torch.stack([mn, mx], dim=-1), norm


def project_ref(x_nchw, w1, b1, w2, b2):
    """x_nchw: [N, Cin, H, W] (any float dtype, taken as exact) -> (float64 reference [N, 4H, 4W, 3], per-element bound)"""
    x = x_nchw.double()
    w1, b1, w2, b2 = (t.double() for t in (w1, b1, w2, b2))
    n1, n2 = 4 * x.shape[1] + 1, 65
    h = F.relu(F.conv_transpose2d(x, w1, b1, **CT))
    err_h = (n1 + 2) * U * F.conv_transpose2d(x.abs(), w1.abs(), b1.abs(), **CT)
    pre = F.conv_transpose2d(h, w2, b2, **CT)
    err_pre = (n2 + 2) * U * F.conv_transpose2d(h, w2.abs(), b2.abs(), **CT) + F.conv_transpose2d(err_h, w2.abs(), None, **CT)
    tol = err_pre / 4 + 4 * U
    return torch.sigmoid(pre).permute(0, 2, 3, 1).contiguous(), tol.permute(0, 2, 3, 1).contiguous()


def project_inputs(x_nhwc, S, channels, full_map):
    """the NCHW input of the mini-decoder for a kernel call: full map [S, K, H, W], single channel [S * K, 1, H, W]"""
    planes = x_nhwc[:S].float()[..., channels].permute(0, 3, 1, 2)
    return planes if full_map else planes.reshape(-1, 1, *planes.shape[2:])


def project_fp32_torch(x_nchw, w1, b1, w2, b2):
    """torch's own fp32 mini-decoder (the condition under which the bound is a fair one) -> [N, 4H, 4W, 3]"""
    h = F.relu(F.conv_transpose2d(x_nchw.float(), w1, b1, **CT))
    return torch.sigmoid(F.conv_transpose2d(h, w2, b2, **CT)).permute(0, 2, 3, 1)
