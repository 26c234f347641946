"""The chunk rule of the per-channel statistics passes (ops._stat_chunks) against the three rules it replaced, written out here
as they stood in moments(), chanhist() and changrad_chunks(); no GPU."""
import itertools

from vaehip import ops

TARGET = 1024  # ops._GN_TARGET when the rules were written
GRID = list(itertools.product((1, 2, 16, 1024, 2048), (1, 15, 16, 63, 576, 65536), (1, 3, 4, 8, 128, 132, 256, 260, 1028)))


def moments_rule(B, HW, Cc):
    units = Cc // 4 if Cc % 4 == 0 else Cc
    pr = max(1, 256 // min(256, units))
    tiles = (units + 255) // 256
    nch = max(1, min(TARGET // max(B * tiles, 1), HW // (16 * pr)))
    per = (HW + nch - 1) // nch
    return (HW + per - 1) // per


def chanhist_rule(B, HW, Cc):
    units, tile = (Cc // 4, 32) if Cc % 4 == 0 else (Cc, 128)
    pr = max(1, 256 // min(tile, units))
    tiles = (units + tile - 1) // tile
    nch = max(1, min(TARGET // max(B * tiles, 1), HW // (16 * pr)))
    per = (HW + nch - 1) // nch
    return (HW + per - 1) // per


def changrad_rule(B, HW, Cc):
    units, tile = (Cc // 4, 64) if Cc % 4 == 0 else (Cc, 256)
    pr = max(1, 256 // min(tile, units))
    tiles = (units + tile - 1) // tile
    nch = max(1, min(TARGET // max(B * tiles, 1), HW // (16 * pr)))
    per = (HW + nch - 1) // nch
    return (HW + per - 1) // per


def test_stat_chunks_are_the_three_rules_and_leave_no_empty_chunk():
    assert ops._GN_TARGET == TARGET
    assert len(GRID) == 5 * 6 * 9
    for B, HW, Cc in GRID:
        got = {
            "moments": (ops._stat_chunks(B, HW, Cc, *ops._MOMENTS_TILE), moments_rule(B, HW, Cc)),
            "chanhist": (ops._stat_chunks(B, HW, Cc, *ops._CHANHIST_TILE), chanhist_rule(B, HW, Cc)),
            "changrad": (ops.changrad_chunks(B, HW, Cc), changrad_rule(B, HW, Cc)),
            "changroup": (ops.changroup_chunks(B, HW, Cc), changrad_rule(B, HW, Cc)),
            "actreg": (ops.actreg_chunks(B, HW, Cc), changrad_rule(B, HW, Cc)),
        }
        for who, (nch, want) in got.items():
            assert nch == want, (who, B, HW, Cc, nch, want)
            assert nch >= 1 and (nch - 1) * -(-HW // nch) < HW, (who, B, HW, Cc, nch)  # no empty chunk
