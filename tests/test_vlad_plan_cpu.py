"""CPU checks of the plan of a MobileNetVLAD handle (csrc/vlad_plan.h, compiled with g++ into tests/cpp/vlad_plan_pin.cpp): which kernel every block runs
on for every combination of the precision, the packed forms a block has, the switches and the sizes on either side of the two pixel thresholds, and the
handle-level choices (fused or layer by layer, the stem form, the NetVLAD head, the FC, which passes use the fisheye mask's constant region), restated here
independently -- in the terms vlad.hip's vlad_backbone_fused / vlad_forward / omni_vlad_create used before the plan existed (v_sblock, mfma_late,
mblock_max_px, mfma_max_px, fc_mfma, skip, skip_mode, own) -- and compared row by row; the rows the production table takes, by name; the rectangles of the
constant region against a brute-force propagation of the mask through the 3x3 convolutions; and that the host code of vlad.hip decides nothing next to
the plan and allocates nothing next to the one owner of device memory."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omni-swarm_amd", "csrc")
F32, F16 = 0, 1                                             # include/omni_hip.h
VB_HBLOCK, VB_SBLOCK, VB_MBLOCK, VB_PW_MFMA3, VB_VALU = range(5)
STEM4, STEM_B0 = 0, 1
ASSIGN_AGG, ASSIGN2_AGG8 = 0, 1
FC_VALU, FC4, FC_MFMA = 0, 1, 2
B_IN = ["prec", "blob", "mblob", "hblob", "sblob", "SBLOCK", "MFMA", "expand", "cin", "hid", "MBLOCK_PX", "MFMA_PX", "px"]
CIN, HID, MBLOCK_PX, MFMA_PX = np.array([24, 12]), np.array([144, 44]), np.array([0, 1200]), np.array([0, 400])       # vlad_plan_pin.cpp: block_table
PX = np.array([399, 400, 401, 1200, 1201, 2048, 2049, 72000])
H_IN = ["UNFUSED", "fusable", "STEM_FUSE", "shape", "K", "FC_MFMA", "out_dim", "Dm", "SBLOCK", "MASK_SKIP", "prec", "mask", "calibrating"]
H_OUT = ["fused", "stem", "head", "fc", "has_skip", "own", "leave_out"]
KS, OUT_DIMS, DMS = np.array([16, 32, 33, 64]), np.array([4096, 4080]), np.array([112, 100, 128])
# stem cout, stem stride, block 0: cin, hid, cout, stride, expand, res; the last row: no blocks (vlad_plan_pin.cpp: kShapes)
SHAPES = np.array([[16, 2, 16, 16, 8, 1, 0, 0], [32, 2, 16, 16, 8, 1, 0, 0], [16, 1, 16, 16, 8, 1, 0, 0], [16, 2, 8, 16, 8, 1, 0, 0], [16, 2, 16, 32, 8, 1, 0, 0],
                   [16, 2, 16, 16, 16, 1, 0, 0], [16, 2, 16, 16, 8, 2, 0, 0], [16, 2, 16, 16, 8, 1, 1, 0], [16, 2, 16, 16, 8, 1, 0, 1], [16, 2, 0, 0, 0, 0, 0, 0]])


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vlad_plan") / "vlad_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "vlad_plan_pin.cpp")])
    return exe


def _table(pin, cmd, names, n_rows):
    t = np.frombuffer(subprocess.run([pin, cmd], capture_output=True, check=True).stdout, np.int32).reshape(-1, len(names))
    assert len(t) == n_rows
    return {n: t[:, i].astype(np.int64) for i, n in enumerate(names)}


def test_every_block_takes_the_path_of_the_parents_if_chain(pin):
    r = _table(pin, "blocks", B_IN + ["path"], 2 * 16 * 2 ** 7 * 8)
    b = lambda n: r[n] != 0
    # omni_vlad_create: the copies of the switches
    v_sblock, mfma_late, mblock_max_px = b("SBLOCK"), b("MFMA"), MBLOCK_PX[r["MBLOCK_PX"]]
    mfma_max_px = np.where(MFMA_PX[r["MFMA_PX"]] > 0, MFMA_PX[r["MFMA_PX"]], 2048)
    B_cin, B_hid, hin_win = CIN[r["cin"]], HID[r["hid"]], PX[r["px"]]
    # vlad_backbone_fused: the chain, first match wins
    hblock = (r["prec"] == F16) & b("hblob")
    sblock = v_sblock & b("sblob")
    mblock = b("mblob") & (hin_win <= mblock_max_px)
    mfma3 = b("expand") & (B_cin % 8 == 0) & (B_hid % 8 == 0) & (hin_win <= mfma_max_px) & mfma_late
    exp = np.where(hblock, VB_HBLOCK, np.where(sblock, VB_SBLOCK, np.where(mblock, VB_MBLOCK, np.where(mfma3, VB_PW_MFMA3, VB_VALU))))
    bad = np.flatnonzero(r["path"] != exp)
    assert len(bad) == 0, (len(bad), {k: int(r[k][bad[0]]) for k in B_IN}, int(r["path"][bad[0]]), int(exp[bad[0]]))
    assert set(np.unique(exp)) == {VB_HBLOCK, VB_SBLOCK, VB_MBLOCK, VB_PW_MFMA3, VB_VALU}
    # every input decides some row (the fp32 VALU form exists for every block of a fusable table: nothing asks for it)
    dims = (2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 8)
    path = r["path"].reshape(dims)
    for axis, n in enumerate(B_IN):
        assert bool((path != path.take([0], axis=axis)).any()) == (n != "blob"), n


def test_every_handle_level_choice_matches_the_parents(pin):
    r = _table(pin, "handles", H_IN + H_OUT, 2 ** 3 * 10 * 4 * 2 * 2 * 3 * 2 ** 5)
    b = lambda n: r[n] != 0
    S_cout, S_stride, B0_cin, B0_hid, B0_cout, B0_stride, B0_expand, B0_res = SHAPES[r["shape"]].T
    blocks_empty = B0_cin == 0
    K, out_dim, n_in = KS[r["K"]], OUT_DIMS[r["out_dim"]], KS[r["K"]] * DMS[r["Dm"]]
    shape = (S_cout == 16) & (S_stride == 2) & (B0_expand == 0) & (B0_res == 0) & (B0_cin == 16) & (B0_hid == 16) & (B0_cout == 8) & (B0_stride == 1)
    # omni_vlad_create
    fused = b("fusable") & ~b("UNFUSED")
    v_sblock = b("SBLOCK")
    fc_mfma = b("FC_MFMA") & fused & (out_dim % 32 == 0) & (n_in % 256 == 0)
    # vlad_plan_mask_skip (600 x 480: a rectangle exists for stem + block 0)
    mskip = fused & v_sblock & b("MASK_SKIP") & b("STEM_FUSE") & ~blocks_empty & shape
    # vlad_backbone_fused
    stem_b0 = b("STEM_FUSE") & ~blocks_empty & shape
    # vlad_forward
    skip = b("mask") & mskip & v_sblock & (r["prec"] != F16)
    skip_mode = np.where(b("calibrating"), 1, np.where(fused & skip, 2, 0))            # vlad_calibrate_mask_skip passes 1
    exp = {"fused": fused, "head": np.where(fused & (K <= 32), ASSIGN2_AGG8, ASSIGN_AGG), "fc": np.where(fc_mfma, FC_MFMA, np.where(fused, FC4, FC_VALU)),
           "has_skip": mskip, "own": (skip_mode != 0) & mskip, "leave_out": (skip_mode == 2) & mskip}
    for n, e in exp.items():
        bad = np.flatnonzero(r[n] != e.astype(np.int64))
        assert len(bad) == 0, (n, len(bad), {k: int(r[k][bad[0]]) for k in H_IN}, int(r[n][bad[0]]), int(e[bad[0]]))
    bad = np.flatnonzero(fused & (r["stem"] != np.where(stem_b0, STEM_B0, STEM4)))      # (the layer-by-layer path has one stem kernel)
    assert len(bad) == 0, {k: int(r[k][bad[0]]) for k in H_IN}
    assert not (mskip & (r["stem"] != STEM_B0)).any()                                   # a masked pass never reads the rectangle of a stem that did not run
    for n in ("fused", "head", "fc", "has_skip", "own", "leave_out"):
        assert len(np.unique(r[n])) == len(np.unique(exp[n].astype(np.int64))) > 1, n


def _oracle_blocks():
    """oracle/mobilenetvlad_ref.py layer_specs() grouped as omni_vlad_create groups it: (cin, hid, cout, stride, expand, res, forms).  Every block with an
    expansion has all four packed forms for this table, block 0 the fp32 VALU form only.  The mblob condition is restated below; whether a split-fp16 / fp16
    form exists is vlad_sblock_supported / vlad_hblock_supported in the .hip files, which this CPU test cannot call: a block that lost its sblob would drop out
    of the mask's constant region and change omni_vlad_mask_skip_layers (tests/test_gpu_vlad_detector.py::test_masked_passes_skip_the_constant_region_bit_identically
    asserts the layers exist), one without an hblob would move test_fp16_operand_mode_error_and_batch_invariance's error out of its (1e-4, 1e-2) band."""
    specs = V.layer_specs()
    assert specs[0][1:] == ("conv3x3", 3, 16, 2)
    blocks, i = [], 1
    while i < len(specs):
        e = specs[i] if specs[i][1] == "pw_relu6" else None
        i += e is not None
        (_, kd, hid, _, stride), (_, kp, _, cout, _) = specs[i], specs[i + 1]
        assert kd == "dw3x3_relu6" and kp in ("pw_linear", "pw_linear_res")
        blocks.append((e[2] if e else hid, hid, cout, stride, int(e is not None), int(kp == "pw_linear_res"), 15 if e else 1))
        if e:                                                    # omni_vlad_create's mblob condition: cin % 4, cop <= 128, vlad_mblock_smem <= 160 KB
            cin, cop, rp = e[2], -(-cout // 32) * 32, -(-(7 * stride + 3) ** 2 // 32) * 32
            assert cin % 4 == 0 and cop <= 128 and (rp * (cin + 1) + rp * 33 + 64 * 33 + 32 * (cin + 11 + cop) + rp) * 4 <= 160 * 1024
            assert hid % 48 == 0 and cout % 4 == 0               # (vlad_sblock_supported's first conditions)
        i += 2
    return blocks


def _plan(pin, h, w, prec, **switches):
    args = [pin, "plan", str(h), str(w), str(prec), "16", "2"] + ["%s=%d" % kv for kv in switches.items()] + [",".join(map(str, b)) for b in _oracle_blocks()]
    p = {"rects": [], "skip": {}}
    for line in subprocess.run(args, capture_output=True, check=True, text=True).stdout.splitlines():
        key, *v = line.split()
        if key == "plan":
            p["fused"], p["stem"], p["head"], p["fc"] = map(int, v)
        elif key == "blocks":
            p["blocks"] = [int(x) for x in v]
        elif key == "rect":
            p["rects"].append(tuple(int(x) for x in v[:11]) + (float(v[11]),))
        else:
            p["skip"][(int(v[0]), int(v[1]))] = (int(v[2]), int(v[3]))
    return p


def test_the_production_rows(pin):
    p = _plan(pin, 480, 600, F32)
    assert (p["fused"], p["stem"], p["head"], p["fc"]) == (1, STEM_B0, ASSIGN2_AGG8, FC_MFMA)
    assert len(p["blocks"]) == 17 and p["blocks"][1:] == [VB_SBLOCK] * 16
    n = len(p["rects"])
    assert n == 5
    # (fisheye_mask, calibrating) -> (layers with their own buffer, rectangles left out): masked fp32 passes skip, the calibration runs every tile
    assert p["skip"] == {(0, 0): (0, 0), (1, 0): (n, 1), (0, 1): (n, 0), (1, 1): (n, 0)}
    h = _plan(pin, 480, 600, F16)                                    # after set_precision(F16): every block with an fp16 form
    assert (h["fused"], h["stem"], h["head"], h["fc"]) == (1, STEM_B0, ASSIGN2_AGG8, FC_MFMA) and h["blocks"][1:] == [VB_HBLOCK] * 16
    assert h["rects"] == p["rects"]                                  # (the buffers are allocated once)
    assert h["skip"][(1, 0)] == (0, 0) and h["skip"][(0, 0)] == (0, 0)       # masked fp16 passes do not skip
    # the switches of the fallback paths, on the same table
    assert _plan(pin, 480, 600, F32, MASK_SKIP=0)["rects"] == [] and _plan(pin, 480, 600, F32, STEM_FUSE=0)["rects"] == []
    assert _plan(pin, 480, 600, F32, STEM_FUSE=0)["stem"] == STEM4
    q = _plan(pin, 480, 600, F32, SBLOCK=0)                          # the exact-f32 kernels: fp32 VALU down to 75 x 60, the fused MFMA kernel from 38 x 30
    assert q["rects"] == [] and q["skip"][(1, 0)] == (0, 0)
    assert q["blocks"][1:] == [VB_VALU] * 6 + [VB_MBLOCK] * 10
    assert _plan(pin, 480, 600, F32, SBLOCK=0, MBLOCK_PX=0)["blocks"][1:] == [VB_VALU] * 6 + [VB_PW_MFMA3] * 10
    assert _plan(pin, 480, 600, F32, SBLOCK=0, MBLOCK_PX=0, MFMA=0)["blocks"][1:] == [VB_VALU] * 16
    assert _plan(pin, 480, 600, F32, SBLOCK=0, MFMA_PX=400)["blocks"][1:] == [VB_VALU] * 6 + [VB_MBLOCK] * 10
    assert _plan(pin, 480, 600, F32, SBLOCK=0, MBLOCK_PX=0, MFMA_PX=400)["blocks"][1:] == [VB_VALU] * 13 + [VB_PW_MFMA3] * 3
    assert _plan(pin, 480, 600, F32, FC_MFMA=0)["fc"] == FC4
    u = _plan(pin, 480, 600, F32, UNFUSED=1)
    assert (u["fused"], u["head"], u["fc"], u["rects"]) == (0, ASSIGN_AGG, FC_VALU, []) and u["skip"][(1, 0)] == (0, 0)


def _mblock(pin, hid, cout, hout, wout, px, mblock_px, cpw, batch, scratch):
    out = subprocess.run([pin, "mblock"] + [str(v) for v in (hid, cout, hout, wout, px, mblock_px, cpw, batch, scratch)], capture_output=True, check=True, text=True).stdout
    return {line.split()[0]: tuple(int(v) for v in line.split()[1:]) for line in out.splitlines()}


def test_the_hidden_layer_split_of_the_mfma_block_kernel(pin):
    """vlad_mblock_split / vlad_mblock_scratch_bytes against the parent's arithmetic (omni_vlad_create's `need`, vlad_backbone_fused's cpw / n_groups) on a
    38 x 30 block 24 -> 144 -> 24 at 4 images: n_chunks = 5, cop = 32, tiles = 5 x 4 x 4 = 80, a partial tile = 64 x cop floats."""
    tile = 64 * 32 * 4
    # OMNI_VLAD_MBLOCK_CPW = 0: all chunks in one workgroup, one group; the handle still keeps a tile of scratch per workgroup, as the parent did
    assert _mblock(pin, 144, 24, 30, 38, 1140, 2048, 0, 4, 80 * tile) == {"split": (5, 1, 80 * tile), "pass": (5, 1), "scratch": (80 * tile,)}
    # 2 chunks per workgroup: ceil(5 / 2) = 3 groups, kept when the scratch holds 3 partial tiles per output tile ...
    assert _mblock(pin, 144, 24, 30, 38, 1140, 2048, 2, 4, 240 * tile) == {"split": (2, 3, 240 * tile), "pass": (2, 3), "scratch": (240 * tile,)}
    # ... and dropped (cpw = n_chunks, one group) when it holds one byte less
    assert _mblock(pin, 144, 24, 30, 38, 1140, 2048, 2, 4, 240 * tile - 1)["pass"] == (5, 1)
    # cout = 40 pads to cop = 64; a block above OMNI_VLAD_MBLOCK_PX gets no scratch
    assert _mblock(pin, 144, 40, 30, 38, 1140, 2048, 2, 4, 0)["split"] == (2, 3, 480 * tile)
    assert _mblock(pin, 144, 24, 30, 38, 1140, 1139, 2, 4, 0)["scratch"] == (0,)
    # more than 1 GB of partial sums: none is allocated, so the pass runs without the split
    big = _mblock(pin, 144, 24, 1000, 1000, 1140, 2048, 2, 4, 0)
    assert big["split"][2] == 125 * 125 * 4 * 3 * tile > 1 << 30 and big["scratch"] == (0,) and big["pass"] == (5, 1)
    assert _mblock(pin, 144, 24, 1000, 1000, 1140, 2048, 0, 4, 0)["scratch"] == (125 * 125 * 4 * tile,)      # (512 000 000 bytes: under the cap)


def _conv3(const, s):
    """the constant set behind a 3x3, padding-1, stride-s layer: an output pixel is constant only if all nine taps lie inside the map and inside `const`"""
    h, w = const.shape
    out = np.zeros(((h - 1) // s + 1, (w - 1) // s + 1), bool)
    for r in range(out.shape[0]):
        for c in range(out.shape[1]):
            y, x = s * r - 1, s * c - 1
            out[r, c] = y >= 0 and x >= 0 and y + 3 <= h and x + 3 <= w and const[y:y + 3, x:x + 3].all()
    return out


def _whole_tiles(const, th, tw):
    """the tiles of a th x tw grid that lie inside the map and inside `const`, pixel by pixel"""
    h, w = const.shape
    return {(ty, tx) for ty in range(-(-h // th)) for tx in range(-(-w // tw))
            if (ty + 1) * th <= h and (tx + 1) * tw <= w and const[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].all()}


@pytest.mark.parametrize("h,w", [(480, 600), (480, 640), (360, 488), (240, 320), (104, 136)])
def test_the_rectangles_are_the_whole_tiles_of_the_propagated_constant_region(pin, h, w):
    blocks = _oracle_blocks()
    const = np.zeros((h, w), bool)
    const[h * 3 // 4:h * 3 // 4 + h // 4] = True                       # omni_fisheye_mask_rows
    const = _conv3(_conv3(const, 2), 1)                                # the stem, block 0's depthwise convolution
    expected = []
    tiles = _whole_tiles(const, 8, 16)                                 # vlad_stem_b0_kernel
    for k in range(len(blocks)):
        if k > 0:
            const = _conv3(const, blocks[k][3])
            tiles = _whole_tiles(const, 8 if blocks[k][3] == 1 else 4, 8)      # vlad_sblock_kernel
        if not tiles:
            break
        expected.append((tiles, const.shape + (blocks[k][2],), (8, 16) if k == 0 else (8 if blocks[k][3] == 1 else 4, 8)))
    rects = _plan(pin, h, w, F32)["rects"]
    assert len(rects) == len(expected)
    for (ty0, ty1, tx0, tx1, oy0, oy1, ox0, ox1, oh, ow, oc, frac), (tiles, shape, (th, tw)) in zip(rects, expected):
        assert {(ty, tx) for ty in range(ty0, ty1) for tx in range(tx0, tx1)} == tiles
        assert (oy0, oy1, ox0, ox1) == (ty0 * th, ty1 * th, tx0 * tw, tx1 * tw) and (oh, ow, oc) == shape
        assert frac == len(tiles) / (-(-oh // th) * -(-ow // tw))
    if (h, w) == (104, 136):
        assert rects == []
    if (h, w) == (480, 600):
        assert [round(100 * r[11]) for r in rects] == [18, 18, 12, 11, 10]             # docs/kernels.md


def _body(src, name):
    """the definition of the static function `name` (a line that starts with its signature and opens a brace) up to the closing brace in column 0"""
    m = re.search(r"^static [^\n;]*\b%s\([^;{]*\{\n.*?^\}\n" % name, src, re.S | re.M)
    assert m, name
    return m.group(0)


def test_the_host_code_decides_nothing_next_to_the_plan():
    src = open(os.path.join(CSRC, "vlad.hip")).read()
    for fn in ("vlad_backbone_fused", "vlad_forward", "vlad_calibrate_mask_skip", "vlad_fc", "vlad_block_mfma3"):
        body = _body(src, fn)
        for word in ("v->cfg[", "OMNI_PREC_", "v->sblock", "v->mfma_late", "_max_px", "v->fc_mfma", "v->fused"):
            assert word not in body, (fn, word)
    assert "vlad_pass_skip(plan, v->prec, fisheye_mask != 0, false)" in _body(src, "vlad_forward")
    assert "switch (plan.blocks[bi])" in _body(src, "vlad_backbone_fused")
    # one owner of the device memory (common.h: DevMem, tests/test_sp_plan_cpu.py)
    assert "hipMalloc(" not in src and "hipFree" not in src
    # plain host C++: nothing of HIP in the plan's header
    plan = open(os.path.join(CSRC, "vlad_plan.h")).read()
    assert "hip/" not in plan and "__device__" not in plan and "common.h" not in plan
