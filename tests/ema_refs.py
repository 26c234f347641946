"""float64 reference of the weight average (EMA) the fused optimizer step keeps, and its decay schedule written out a second
time, independently of vaehip/optim.py (a helper module, not a test).

The kernel computes e' = fmaf(omd, p' - e, e) with omd = float32(1 - d): one rounding of p' - e, one of the result.  The
reference takes the same fp32 omd (the hyper-parameter the kernel was given, not the exact 1 - d) and does the rest in float64."""
from __future__ import annotations

import numpy as np
import torch

EMA_DECAY = 0.9999


def decay_schedule(t: int, ema_decay: float = EMA_DECAY) -> float:
    """decay of the t-th optimizer update, t from 1: diffusers' EMAModel defaults.  The first update copies the weights."""
    if t == 1:
        return 0.0
    return min(ema_decay, t / (9 + t))


def ema_ref64(e: torch.Tensor, p_new: torch.Tensor, d: float) -> torch.Tensor:
    """e + float64(float32(1 - d)) (p_new - e) in float64; p_new itself for d == 0"""
    p64 = p_new.detach().double()
    if d == 0:
        return p64
    e64 = e.detach().double()
    return e64 + float(np.float32(1.0 - d)) * (p64 - e64)


def step_bound(e: torch.Tensor, p_new: torch.Tensor) -> torch.Tensor:
    """elementwise 4 * 2^-24 * max(|e|, |p'|): p' - e is at most 2 max in size and rounds once (2^-24 * 2 max), the result is
    at most max in size and rounds once (2^-24 max); 4 covers both with room for the fp32 omd product inside the fma"""
    return 4.0 * 2.0 ** -24 * torch.maximum(e.detach().double().abs(), p_new.detach().double().abs())
