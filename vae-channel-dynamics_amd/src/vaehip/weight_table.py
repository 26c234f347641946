"""WeightTable: the device table of ops.weight_dynamics (csrc/wdyn.hip) for a list of parameter tensors of the flat arenas.

An entry is {off, O, K, I, out0, in0, ws0, chunk0}: the tensor's element offset into every arena, its memory shape [O][K][I]
(OHWI conv weight: K = kh kw; linear [out][in]: K = 1; 1-D: K = I = 1) and four running sums in table order: its first output
slice, its first input slice (a tensor with I == 1 has none), its first column row of the workspace and its first workgroup.
Everything is built and checked here, once, and uploaded once; the launch path checks nothing about the table's contents.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

TAB_WORDS = 8
N_SUMS = 6


class Slot(NamedTuple):
    """where one tensor's results lie in the vectors ops.weight_dynamics returns"""
    name: str
    off: int
    O: int
    K: int
    I: int
    out0: int
    in0: int      # of its input slices (I of them); meaningless when I == 1
    ws0: int
    chunk0: int
    nchunk: int


def okI_of(shape: Sequence[int]) -> Tuple[int, int, int]:
    """memory shape [O][K][I] of a parameter of logical shape `shape` in the arena (ParamArena.view_of)"""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 4:
        o, i, kh, kw = shape
        return o, kh * kw, i
    if len(shape) == 2:
        return shape[0], 1, shape[1]
    if len(shape) == 1:
        return shape[0], 1, 1
    raise ValueError(f"weight table: a parameter of shape {shape} is no conv weight, linear weight or vector")


MAX_ROWS = 8  # most rows of a chunk when I > 1 (WD_ROWS of csrc/wdyn.hip)


def rows_per_chunk(K: int, I: int, chunk: int) -> int:
    """whole output rows a workgroup owns (wd_rpc of csrc/wdyn.hip): what fits the chunk, at most MAX_ROWS when I > 1; a row
    longer than the chunk is still one workgroup"""
    fit = max(1, chunk // (K * I))
    return fit if I == 1 else min(MAX_ROWS, fit)


class WeightTable:
    """table of ops.weight_dynamics for `params` = [(name, parameter)] of `arena` (in any order; the results come in that order).
    Checked here: shapes, offsets on multiples of 4 elements, disjoint tensors, off + O K I <= arena.total."""

    def __init__(self, arena, params: Sequence[Tuple[str, torch.Tensor]]):
        entries = []
        for name, p in params:
            if id(p) not in arena.offset_of:
                raise ValueError(f"weight table: parameter {name!r} does not live in the arena")
            entries.append((name, arena.offset_of[id(p)]) + okI_of(p.shape))
        self._build(entries, int(arena.total), arena.flat.device)

    @classmethod
    def from_entries(cls, entries: Sequence[Tuple[str, int, int, int, int]], total: int, device) -> "WeightTable":
        """from (name, off, O, K, I) tuples over buffers of `total` elements"""
        self = cls.__new__(cls)
        self._build(list(entries), int(total), torch.device(device))
        return self

    def _build(self, entries, total: int, device):
        from .lib import lib
        if not entries:
            raise ValueError("weight table: no tensor")
        self.chunk = int(lib.query("vae_wdyn_chunk"))
        self.total = total
        self.slots: List[Slot] = []
        out0 = in0 = ws0 = chunk0 = 0
        for name, off, O, K, I in entries:
            off, O, K, I = int(off), int(O), int(K), int(I)
            if min(O, K, I) < 1:
                raise ValueError(f"weight table: {name!r} has an empty shape [{O}][{K}][{I}]")
            if off < 0 or off % 4:
                raise ValueError(f"weight table: {name!r} starts at element {off}, not on a multiple of 4")
            if off + O * K * I > total:
                raise ValueError(f"weight table: {name!r} ends at {off + O * K * I}, beyond the buffers' {total} elements")
            rpc = rows_per_chunk(K, I, self.chunk)
            nch = (O + rpc - 1) // rpc
            self.slots.append(Slot(name, off, O, K, I, out0, in0, ws0, chunk0, nch))
            out0 += O
            if I > 1:
                in0 += I
                ws0 += nch * I
            chunk0 += nch
        prev_end, prev_name = 0, None
        for s in sorted(self.slots, key=lambda s: s.off):
            if s.off < prev_end:
                raise ValueError(f"weight table: {s.name!r} overlaps {prev_name!r}")
            prev_end, prev_name = s.off + s.O * s.K * s.I, s.name
        self.nseg = len(self.slots)
        self.extent = prev_end  # elements an arena needs for this table
        host = torch.tensor([[s.off, s.O, s.K, s.I, s.out0, s.in0, s.ws0, s.chunk0] for s in self.slots], dtype=torch.int64)
        # the C side's own check of the same table (offsets, shapes, running sums), and its totals
        nchunk, n_out, n_in, nwords = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        lib.call("vae_wdyn_workspace", C.c_void_p(host.data_ptr()), self.nseg, C.byref(nchunk), C.byref(n_out), C.byref(n_in),
                 C.byref(nwords))
        if (nchunk.value, n_out.value, n_in.value) != (chunk0, out0, in0):
            raise RuntimeError("weight table: the library counts this table differently")
        self.nchunk, self.n_out, self.n_in, self.nwords = chunk0, out0, in0, int(nwords.value)
        self.host = host
        self.device = torch.device(device)
        self.tab = host.to(self.device)  # uploaded once

    def slot(self, name: str) -> Slot:
        for s in self.slots:
            if s.name == name:
                return s
        raise KeyError(name)

    def out_slice(self, s: Slot) -> slice:
        return slice(s.out0, s.out0 + s.O)

    def in_slice(self, s: Slot) -> Optional[slice]:
        return slice(s.in0, s.in0 + s.I) if s.I > 1 else None
