"""CPU checks around the constant region of the fisheye mask (csrc/superpoint.hip sp_plan_mask_skip, csrc/tile_walk.h; the GPU side is
tests/test_gpu_mask_skip.py): the tile walk the persistent kernels share -- the decode of a tile's number among the tiles that run into (tile row,
tile column) by multiply-high or hardware division, and into its number in the full grid -- enumerates every tile outside the rectangle exactly
once, for every rectangle of several grids (the header itself, compiled with g++ into tests/cpp/tile_walk_pin.cpp); the plan bench.py mirrors for
its FLOP accounting gives the rectangles worked out by hand for 600 x 480 (docs/history/rounds_2_to_5.md, round 3)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_walk") / "tile_walk_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "tile_walk_pin.cpp")])
    return exe


def _walks(pin, tiles_x, tiles_y, batch, rects):
    """tile_walk_pin over rectangles (ty0, ty1, tx0, tx1): per rectangle None (refused) or an [n][3] array of full-grid tile numbers in walk order
    (multiply-high (row, column), hardware-division (row, column), index form)"""
    args = [str(v) for r in rects for v in r]
    raw = np.frombuffer(subprocess.run([pin, str(tiles_x), str(tiles_y), str(batch)] + args, capture_output=True, check=True).stdout, np.uint16)
    out, i = [], 0
    for _ in rects:
        n = int(raw[i]); i += 1
        if n == 65535:
            out.append(None)
            continue
        out.append(raw[i:i + 3 * n].reshape(n, 3).astype(np.int64)); i += 3 * n
    assert i == len(raw)
    return out


def _expected(tiles_x, tiles_y, batch, ty0, ty1, tx0, tx1):
    b, y, x = np.meshgrid(np.arange(batch), np.arange(tiles_y), np.arange(tiles_x), indexing="ij")
    skip = ty1 > ty0 and tx1 > tx0
    keep = ~(skip & (y >= ty0) & (y < ty1) & (x >= tx0) & (x < tx1))
    return (b * tiles_x * tiles_y + y * tiles_x + x)[keep]                # row-major, image by image


def test_tile_walk_enumerates_the_tiles_outside_the_rectangle_once(pin):
    """the (tile row, tile column) form of the five persistent conv kernels, both divisions; rectangles up to the full width of the grid (bw = 0)"""
    full_width = 0
    for tx, ty in [(19, 60), (10, 30), (5, 15), (1, 1), (2, 3), (3, 8)]:
        rects = [(0, 0, 0, 0)] + [(a, b, c, d) for a in range(ty) for b in range(a + 1, ty + 1) for c in range(tx) for d in range(c + 1, tx + 1)
                                  if (b - a) * (d - c) < tx * ty and (ty <= 20 or (a % 7 == 4 and b % 5 == 4))]
        for rect, seen in zip(rects, _walks(pin, tx, ty, 2, rects)):
            want = _expected(tx, ty, 2, *rect)
            assert seen is not None, (tx, ty, rect)
            for form in (0, 1):
                assert np.array_equal(np.sort(seen[:, form]), want) and len(np.unique(seen[:, form])) == len(want), (tx, ty, rect, form)
            full_width += rect[3] - rect[2] == tx
    assert full_width > 100
    # refused: outside the grid, the whole image
    assert _walks(pin, 5, 3, 1, [(0, 4, 0, 1), (0, 1, 4, 6), (-1, 1, 0, 1), (0, 3, 0, 5)]) == [None] * 4


def test_mobilenetvlad_tile_walk_enumerates_the_tiles_outside_the_rectangle_once(pin):
    """the index form of the persistent block kernel of MobileNetVLAD under the fisheye mask (round 6): rectangles up to the full width of the grid
    (no tile left in a band row)"""
    for tx, ty in [(19, 30), (10, 15), (5, 8), (1, 2), (3, 4)]:
        rects = [(0, 0, 0, 0)] + [(a, b, c, d - c) for a in range(ty) for b in range(a + 1, ty + 1) for c in range(tx) for d in range(c + 1, tx + 1)
                                  if (b - a) * (d - c) < tx * ty and (ty <= 8 or (a % 5 == 3 and b % 4 == 1))]
        walks = _walks(pin, tx, ty, 3, [(a, b, c, c + w) for a, b, c, w in rects])
        for (sy0, sy1, sx0, sw), seen in zip(rects, walks):
            want = _expected(tx, ty, 3, sy0, sy1, sx0, sx0 + sw)
            assert seen is not None and np.array_equal(seen[:, 2], want), (tx, ty, sy0, sy1, sx0, sw)      # (in order: the walk is monotonic)


def test_plan_for_600x480_is_the_one_worked_out_by_hand():
    """omni_sp_mask_skip_plan (the library's own plan, pure arithmetic: callable without a device) -- bench.py takes its executed-FLOP accounting from the
    same function through omni_sp_stage_tiles_left_out"""
    import omni_loader
    capi = omni_loader.load().capi
    plan = lambda h, w, prec, layer: capi.sp_mask_skip_plan(w, h, prec, layer)
    F16, SPLIT, F32 = capi.PREC_F16, capi.PREC_SPLIT, capi.PREC_F32
    # rows 360-479 are blanked; conv1a is constant on rows 361-479; conv1b on 362-478 x 1-598 -> tile rows 46-58 (13 of 60), tile columns 1-17 (of 19)
    assert plan(480, 600, F16, 1) == ((46, 59, 1, 18), 13 * 17 / (60 * 19))
    assert plan(480, 600, F16, 2) == ((23, 29, 1, 9), 6 * 8 / (30 * 10))            # 240 x 300: rows 182-237 x columns 2-297 -> tile rows 23-28, columns 1-8
    assert plan(480, 600, F16, 3) == ((23, 29, 1, 9), 6 * 8 / (30 * 10))
    assert plan(480, 600, F16, 4) == ((12, 14, 1, 4), 2 * 3 / (15 * 5))             # 120 x 150: rows 93-116 x columns 3-146 -> tile rows 12-13, columns 1-3
    assert plan(480, 600, F16, 0)[1] == 0.0                                          # conv1a is fused into conv1b on the fp16 path
    # OMNI_PREC_SPLIT: conv1a in 8-row tile rows over the whole width (rows 361-479 -> tile rows 46-59), the cin = 64 layers in 4 x 32 tiles
    assert plan(480, 600, SPLIT, 0) == ((46, 60, 0, 19), 14 / 60)
    assert plan(480, 600, SPLIT, 1) == ((91, 119, 1, 18), 28 * 17 / (120 * 19))      # rows 362-478 -> 4-row tile rows 91-118
    assert plan(480, 600, SPLIT, 2) == ((46, 59, 1, 9), 13 * 8 / (60 * 10))          # rows 182-237
    assert plan(480, 600, SPLIT, 5) == ((47, 58, 1, 4), 11 * 3 / (60 * 5))           # conv3b, 120 x 150, 2 x 32 tiles: rows 94-115 x columns 4-145
    assert plan(480, 600, F16, 5) == ((16, 19, 1, 4), 3 * 3 / (20 * 5))              # conv3b on the fp16 register-stationary kernel: 6 x 32 tiles, rows 96-113
    for layer in range(6):
        assert plan(64, 96, F16, layer)[1] == 0.0                                    # the band is thinner than a tile row
        assert plan(480, 600, F32, layer)[1] == 0.0
