"""Which parameters of the VAE train (`training.trainable_modules`, HipTrainer(trainable=...)).

A value is None (leave requires_grad as the user set it), 'all', one of the shorthands 'decoder' (= decoder + post_quant_conv)
and 'encoder' (= encoder + quant_conv), or a list of module-name prefixes: a parameter trains if its name equals a prefix or
starts with `prefix.`.  Everything here is host logic on names and offsets, up to RangeTable, which puts a checked list of
ranges on the device for ops.sqnorm_ranges / ops.adamw_ranges.
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence, Set, Tuple, Union

import torch

SHORTHANDS = {"decoder": ("decoder", "post_quant_conv"), "encoder": ("encoder", "quant_conv")}
Trainable = Union[None, str, Sequence[str]]


def resolve_trainable(names: Iterable[str], value: Trainable) -> Set[str]:
    """the parameter names of `names` that `value` makes trainable.  A prefix that matches nothing and an empty set are
    ValueErrors.  A shorthand is a shorthand only as the whole value: inside a list 'decoder' is the plain prefix."""
    names = list(names)
    if value is None:
        raise ValueError("resolve_trainable: None means 'as requires_grad stands'; there is nothing to resolve")
    if isinstance(value, str):
        if value == "all":
            return set(names)
        prefixes: List[str] = list(SHORTHANDS.get(value, (value,)))
    else:
        prefixes = [str(v) for v in value]
    chosen: Set[str] = set()
    for pre in prefixes:
        hit = [n for n in names if n == pre or n.startswith(pre + ".")]
        if not hit:
            raise ValueError(f"trainable_modules: prefix {pre!r} matches no parameter of the VAE")
        chosen.update(hit)
    if not chosen:
        raise ValueError("trainable_modules: the trainable set is empty")
    return chosen


def apply_trainable(vae, value: Trainable) -> None:
    """sets requires_grad on every parameter of `vae` (value None: leaves it as it is); an empty set is a ValueError"""
    params = list(vae.named_parameters())
    if value is not None:
        chosen = resolve_trainable([n for n, _ in params], value)
        for n, p in params:
            p.requires_grad_(n in chosen)
    if not any(p.requires_grad for _, p in params):
        raise ValueError("no parameter of the VAE has requires_grad: the trainable set is empty")


def chunk_prefix(ranges: Sequence[Tuple[int, int]], chunk: int) -> List[int]:
    """[len(ranges) + 1] prefix sum of ceil(length / chunk): the seg_chunk0 table of the *_ranges entry points"""
    out = [0]
    for b, e in ranges:
        out.append(out[-1] + (e - b + chunk - 1) // chunk)
    return out


def check_ranges(ranges: Sequence[Tuple[int, int]], total: Optional[int] = None) -> None:
    """the contract of the *_ranges entry points: non-empty ranges, sorted, disjoint, starts on multiples of 4 elements"""
    if not ranges:
        raise ValueError("range table: no range")
    prev = 0
    for b, e in ranges:
        if b % 4:
            raise ValueError(f"range table: [{b}, {e}) does not start on a multiple of 4 elements")
        if not prev <= b < e:
            raise ValueError(f"range table: [{b}, {e}) is empty, out of order or overlaps the range before it")
        prev = e
    if total is not None and prev > total:
        raise ValueError(f"range table: ends at {prev}, beyond the buffer's {total} elements")


def span_of(ranges: Sequence[Tuple[int, int]]) -> Tuple[int, int]:
    """[first trainable offset, end of the last trainable range): what data-parallel ranks exchange"""
    return ranges[0][0], ranges[-1][1]


class RangeTable:
    """device tables of the *_ranges entry points (ops.sqnorm_ranges, ops.adamw_ranges) for a list of [begin, end) element
    ranges of arena-sized buffers.  The list is checked here, once (check_ranges); the launch path checks nothing about it."""

    def __init__(self, ranges, device, total: Optional[int] = None):
        from .lib import lib
        self.ranges = [(int(b), int(e)) for b, e in ranges]
        check_ranges(self.ranges, total)
        self.total = total
        chunk0 = chunk_prefix(self.ranges, lib.query("vae_dead_scan_chunk"))
        self.nseg, self.nchunk = len(self.ranges), chunk0[-1]
        self.numel = sum(e - b for b, e in self.ranges)
        self.seg_off = torch.tensor(self.ranges, dtype=torch.int64).reshape(-1, 2).to(device)
        self.seg_chunk0 = torch.tensor(chunk0, dtype=torch.int32).to(device)
        self.ws = torch.empty(self.nchunk, device=device, dtype=torch.float32)  # sqnorm_ranges: one partial per chunk
