"""Symmetric Schur items from 4 x 4 blocks (csrc/lba_schur_items.h:k_schur_fused<true, false, true>, csrc/schur_plan.h:schur_step /
schur_instr_list), checked on the CPU through the host-only exports osh_lba_schur_block_list and osh_lba_schur_plan_shapes: the
instructions of one k step store every entry of every live pose pair exactly once, at exactly the places the whole-tile path stores,
for every item shape; the plan statistic counts them; and the headline window's matrix-pipe cycles are the ones DESIGN.md section 8(1)
states.  Needs no GPU."""
from collections import Counter

import pytest

from orb_slam3_study_kr_amd import lba, synth
from test_schur_plan_cpu import plan_stats


def stores(instrs, live):
    """Counter of the places (row, column) of the item's 48 x 48 product that the instructions store; live(sa, sb): the pose pair has a slot."""
    at = Counter()
    for ins in instrs:
        if ins[0] == "tile":
            _, ti, tj = ins
            for r in range(16 * ti, 16 * ti + 16):
                for c in range(16 * tj, 16 * tj + 16):
                    if live(r // 6, c // 6):
                        at[r, c] += 1
        else:
            for br, bc, use in ins[1]:
                for r in range(4 * br, 4 * br + 4) if use else ():
                    for c in range(4 * bc, 4 * bc + 4):
                        if live(r // 6, c // 6):
                            at[r, c] += 1
                            if use == 2 and r // 6 == c // 6:
                                at[c, r] += 1
    return at


@pytest.mark.parametrize("nx", range(1, 9))
def test_symmetric_items_store_every_entry_once_where_the_tiles_do(nx):
    live = lambda sa, sb: sa <= sb < nx
    blocks, tiles = lba.schur_block_list(True, nx, nx), lba.schur_block_list(True, nx, nx, use_blocks=False)
    assert all(k == "tile" for k, *_ in tiles) and len(tiles) == ((6 * nx + 15) // 16) * ((6 * nx + 15) // 16 + 1) // 2
    got, ref = stores(blocks, live), stores(tiles, live)
    assert set(got.values()) == {1}, {k: v for k, v in got.items() if v != 1}
    assert set(got) == set(ref)
    # every entry on or above the diagonal of every live pose pair (a diagonal pair's lower triangle: as far as the tiles store it)
    need = {(r, c) for r in range(6 * nx) for c in range(r, 6 * nx)}
    assert need <= set(got)
    assert all(r // 6 == c // 6 for r, c in set(got) - need)
    # only tiles whose four block rows all hold image rows stay tiles; a pose subset of the item stores a subset
    assert all(6 * nx >= 16 * tj + 13 for k, *t in blocks if k == "tile" for tj in [t[1]])
    sub = lambda sa, sb: sa <= sb < nx and sa != 0
    assert stores(blocks, sub) == stores(tiles, sub)


@pytest.mark.parametrize("ny", range(1, 5))
@pytest.mark.parametrize("nx", range(1, 9))
def test_cross_items_keep_their_tiles(nx, ny):
    live = lambda sa, sb: sa < nx and sb < ny
    blocks = lba.schur_block_list(False, nx, ny)
    assert blocks == lba.schur_block_list(False, nx, ny, use_blocks=False)
    got = stores(blocks, live)
    assert set(got.values()) == {1} and set(got) == {(r, c) for r in range(6 * nx) for c in range(6 * ny)}


def quarters(sym, nx, ny):
    """issued matrix work of one k step in quarters of a 16x16x4 instruction"""
    return sum(4 if k == "tile" else 1 for k, *_ in lba.schur_block_list(sym, nx, ny))


def test_instruction_counts_per_shape():
    assert [quarters(True, n, n) for n in range(1, 9)] == [2, 3, 5, 7, 10, 13, 19, 21]   # whole tiles: 4, 4, 12, 12, 12, 24, 24, 24
    assert [quarters(False, 8, n) for n in range(1, 5)] == [12, 12, 24, 24]


# matrix-pipe cycles of the headline window with blocks / with whole tiles, all items (2 683 008 of the
# 3 477 888 cycles with whole tiles are the symmetric items') and the symmetric items alone
HEADLINE_RATIO, HEADLINE_RATIO_SYM = 0.8811, 0.8459


def test_headline_window_shapes_cycles_and_statistic():
    w = synth.make_config2(100)
    shapes, tiles, blocks = lba.schur_plan_shapes(w, 64)      # items of at most 64 landmarks, as in the batch of 512
    sym = {k: v for k, v in shapes.items() if k[0] == 1}
    assert sum(sym.values()) == 301 and {k[1] for k in sym} == set(range(1, 9))
    assert sum(v for k, v in shapes.items() if k[0] == 0) == 85 and {k[1:3] for k in shapes if k[0] == 0} <= {(8, 1), (8, 2), (8, 3), (8, 4)}
    assert abs(blocks / tiles - HEADLINE_RATIO) < 5e-4, blocks / tiles
    # the cycles are the instruction lists at 64 / 17 cycles; the plan statistic is the same work in 16x16x4 instructions
    ksteps = lambda n: 6 * ((n + 7) // 8)
    cyc = lambda s, nx, ny, use: sum(64 if k == "tile" else 17 for k, *_ in lba.schur_block_list(s, nx, ny, use))
    assert tiles == sum(v * ksteps(n) * cyc(s, nx, ny, False) for (s, nx, ny, n), v in shapes.items())
    assert blocks == sum(v * ksteps(n) * cyc(s, nx, ny, True) for (s, nx, ny, n), v in shapes.items())
    sym_tiles = sum(v * ksteps(n) * cyc(1, nx, ny, False) for (_, nx, ny, n), v in sym.items())
    assert sym_tiles == 2683008 and abs((blocks - (tiles - sym_tiles)) / sym_tiles - HEADLINE_RATIO_SYM) < 5e-4
    one, _, _ = lba.schur_plan_shapes(w)                     # (a single window: what plan_stats builds)
    assert plan_stats(w)["mfma"] == sum(v * (quarters(s, nx, ny) * ksteps(n) // 4) for (s, nx, ny, n), v in one.items())
