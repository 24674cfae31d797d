"""CPU checks of the plan of a SuperPoint pass (csrc/sp_plan.h, compiled with g++ into tests/cpp/sp_plan_pin.cpp): which kernels a pass runs for every
combination of the precision, the variant switches, the image's divisibility and the pass's own inputs, restated here independently -- in the terms
superpoint.hip's sp_forward used before the plan existed (fuse1a, w1b .. w3a, sparse, sparse32, sparse_da32, ...) -- and compared row by row; the
rows the production paths take, by name; the state of the fisheye mask's constant region over sequences of passes; and that the host code of
superpoint.hip decides nothing next to the plan (no precision / switch expression inside sp_forward, sp_make_dense, sp_calibrate_mask_skip; one owner
of the device memory; one place that makes a ConvArgs)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omni-swarm_amd", "csrc")
F32, F16, SPLIT = 0, 1, 2                                   # include/omni_hip.h
SIZES = np.array([(480, 600), (72, 104), (68, 100), (66, 98)])     # divisible by 8 / by 8 / by 4 only / by 2 only
INPUTS = ["prec", "cv", "det16", "fused_cand", "sparse_desc", "sparse_da", "split_fuse1a", "split_db", "wino_req", "size", "mask_skip", "aligned4", "mask",
          "run_post", "calibrating"]
OUTPUTS = ["wino", "conv1a", "conv1b", "raw_1b", "w2a", "cvt2a", "raw_2a", "w2b", "cvt2b", "raw_2b", "w3a", "cvt3a", "raw_3a", "use_skip", "heads_sparse_da",
           "tails_f32", "det", "cand_fused", "desc", "desc_split_db", "dense_valid", "heads_full", "run_post_out", "calibrating_out"]
C1A_DIRECT, C1A_SPLIT, C1A_FUSED = 0, 1, 2
C1B_CONV, C1B_FUSED_F16, C1B_FUSED_SPLIT, C1B_FUSED_WINO = 0, 1, 2, 3
DET_VALU, DET_MFMA16_F16, DET_MFMA16_F32, DET_MFMA_F32 = 0, 1, 2, 3
DESC_DENSE_GENERIC, DESC_DENSE_F16, DESC_SPARSE_F16, DESC_SPARSE_DA_F16, DESC_GATHER_F32, DESC_SPARSE_DA_SPLIT = 0, 1, 2, 3, 4, 5
STALE, READY_FUSED, READY_UNFUSED = 0, 1, 2


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sp_plan") / "sp_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sp_plan_pin.cpp")])
    return exe


@pytest.fixture(scope="module")
def rows(pin):
    raw = np.frombuffer(subprocess.run([pin, "plans"], capture_output=True, check=True).stdout, np.uint8)
    t = raw.reshape(-1, len(INPUTS) + len(OUTPUTS))
    assert len(t) == 3 * 4 * 2 ** 6 * 16 * 4 * 2 * 2 ** 4
    return {n: t[:, i].astype(np.int64) for i, n in enumerate(INPUTS + OUTPUTS)}


def _expected(r):
    """the parent's sp_forward / sp_init, variable by variable"""
    b = lambda n: r[n] != 0
    P, cv = r["prec"], r["cv"]
    f16, split = P == F16, P == SPLIT
    H, W = SIZES[r["size"], 0], SIZES[r["size"], 1]
    # sp_init: OMNI_SPLIT_WINO clamped by the image's divisibility and by the conv1a fusion
    wino = r["wino_req"].copy()
    wino[(H % 8 != 0) | (W % 8 != 0)] &= 7
    wino[(H % 4 != 0) | (W % 4 != 0)] &= 1
    wino[(H % 2 != 0) | (W % 2 != 0) | ~b("split_fuse1a")] &= ~1
    wino[~split] = 0
    fuse1a = ((f16 & (cv == 0)) | (split & b("split_fuse1a"))) & b("aligned4")
    use_skip = b("mask_skip") & b("mask") & (fuse1a | split) & ~b("calibrating")
    w1b, w2a, w2b, w3a = split & (wino & 1 != 0) & fuse1a, split & (wino & 2 != 0), split & (wino & 4 != 0), split & (wino & 8 != 0)
    raw_1b, raw_2a, raw_2b = w1b & w2a, w2a & w2b, w2b & w3a
    sparse = f16 & (cv == 0) & b("sparse_desc") & b("run_post")
    sparse32 = ~f16 & (cv == 0) & b("sparse_desc") & b("run_post")
    sparse_da_handle = b("sparse_desc") & b("sparse_da")
    sparse_da32 = sparse32 & split & sparse_da_handle
    sparse_da = (sparse & sparse_da_handle) | sparse_da32
    e = {"wino": wino}
    e["conv1a"] = np.where(fuse1a, C1A_FUSED, np.where(split, C1A_SPLIT, C1A_DIRECT))
    e["conv1b"] = np.where(~fuse1a, C1B_CONV, np.where(w1b, C1B_FUSED_WINO, np.where(split, C1B_FUSED_SPLIT, C1B_FUSED_F16)))
    e["raw_1b"] = raw_1b                                            # conv1ab_wino_fused(out_split = !w2a)
    e["w2a"], e["cvt2a"], e["raw_2a"] = w2a, w2a & ~raw_1b, raw_2a      # wino_layer(L2A, in_raw = raw_1b, out_split = !w2b)
    e["w2b"], e["cvt2b"], e["raw_2b"] = w2b, w2b & ~raw_2a, raw_2b
    e["w3a"], e["cvt3a"], e["raw_3a"] = w3a, w3a & ~raw_2b, np.zeros_like(w3a)      # conv3a always writes split-64
    e["use_skip"] = use_skip
    e["heads_sparse_da"] = sparse_da
    e["tails_f32"] = ~f16                                           # PH
    e["det"] = np.where(cv == 1, DET_VALU, np.where((f16 | split) & b("det16"), np.where(f16, DET_MFMA16_F16, DET_MFMA16_F32), DET_MFMA_F32))
    e["cand_fused"] = b("run_post") & b("fused_cand") & (cv != 1)
    e["desc"] = np.where(sparse & sparse_da, DESC_SPARSE_DA_F16, np.where(sparse, DESC_SPARSE_F16, np.where(sparse_da32, DESC_SPARSE_DA_SPLIT, np.where(
        sparse32, DESC_GATHER_F32, np.where(f16 & (cv == 0), DESC_DENSE_F16, DESC_DENSE_GENERIC)))))
    e["desc_split_db"] = sparse_da32 & b("split_db")                # wDbFragHi exists
    e["dense_valid"] = ~sparse & ~sparse32
    e["heads_full"] = ~sparse_da32
    e["run_post_out"], e["calibrating_out"] = b("run_post"), b("calibrating")
    return e


def test_every_combination_matches_the_rules_restated(rows):
    exp = _expected(rows)
    assert sorted(exp) == sorted(OUTPUTS)
    for n in OUTPUTS:
        bad = np.flatnonzero(rows[n] != exp[n].astype(np.int64))
        assert len(bad) == 0, (n, len(bad), {k: int(rows[k][bad[0]]) for k in INPUTS}, int(rows[n][bad[0]]), int(exp[n][bad[0]]))
    # every switch is read under every precision that can read it: flipping it changes some row's plan there
    reads = {F16: ["cv", "det16", "fused_cand", "sparse_desc", "sparse_da", "mask_skip", "aligned4", "mask", "run_post", "calibrating"],
             SPLIT: ["cv", "det16", "fused_cand", "sparse_desc", "sparse_da", "split_fuse1a", "split_db", "wino_req", "size", "mask_skip", "aligned4", "mask", "run_post",
                     "calibrating"],
             F32: ["cv", "fused_cand", "sparse_desc", "run_post"]}
    dims = (3, 4, 2, 2, 2, 2, 2, 2, 16, 4, 2, 2, 2, 2, 2)                 # the rows are the full product, INPUTS[0] slowest
    for i, n in enumerate(INPUTS):
        assert np.array_equal(rows[n], np.broadcast_to(np.arange(dims[i]).reshape([-1 if j == i else 1 for j in range(len(dims))]), dims).ravel()), n
    plan = np.stack([rows[n] for n in OUTPUTS[:-2]], 1).reshape(dims + (-1,))       # (without the two inputs the plan carries along)
    for prec, names in reads.items():
        for axis, n in enumerate(INPUTS[1:]):
            a = plan[prec]
            differs = bool((a != a.take([0], axis=axis)).any())
            assert differs == (n in names), (prec, n, differs)


def _row(rows, **kw):
    d = dict(cv=0, det16=1, fused_cand=1, sparse_desc=1, sparse_da=1, split_fuse1a=1, split_db=1, wino_req=7, size=0, mask_skip=1, aligned4=1, mask=1, run_post=1,
             calibrating=0)
    d.update(kw)
    sel = np.ones(len(rows["prec"]), bool)
    for k, v in d.items():
        sel &= rows[k] == v
    i, = np.flatnonzero(sel)
    return {n: int(rows[n][i]) for n in OUTPUTS}


def test_pinned_rows(rows):
    p = _row(rows, prec=F16)                                        # production fp16
    assert (p["conv1a"], p["conv1b"], p["use_skip"]) == (C1A_FUSED, C1B_FUSED_F16, 1)
    assert (p["heads_sparse_da"], p["tails_f32"], p["det"], p["cand_fused"], p["desc"], p["dense_valid"]) == (1, 0, DET_MFMA16_F16, 1, DESC_SPARSE_DA_F16, 0)
    assert (p["w2a"], p["w2b"], p["w3a"]) == (0, 0, 0)
    p = _row(rows, prec=SPLIT)                                      # production split
    assert (p["wino"], p["conv1a"], p["conv1b"], p["raw_1b"]) == (7, C1A_FUSED, C1B_FUSED_WINO, 1)
    assert (p["w2a"], p["cvt2a"], p["raw_2a"]) == (1, 0, 1) and (p["w2b"], p["cvt2b"], p["raw_2b"]) == (1, 0, 0) and (p["w3a"], p["cvt3a"]) == (0, 0)
    assert (p["heads_sparse_da"], p["tails_f32"], p["det"], p["desc"], p["desc_split_db"], p["heads_full"], p["use_skip"]) == (
        1, 1, DET_MFMA16_F32, DESC_SPARSE_DA_SPLIT, 1, 0, 1)
    p = _row(rows, prec=SPLIT, aligned4=0)                          # split, unaligned pointer
    assert (p["conv1a"], p["conv1b"], p["raw_1b"]) == (C1A_SPLIT, C1B_CONV, 0) and (p["w2a"], p["cvt2a"], p["raw_2a"]) == (1, 1, 1) and p["use_skip"] == 1
    p = _row(rows, prec=F32, mask_skip=0)                           # fp32
    assert (p["conv1a"], p["conv1b"], p["w2a"], p["w2b"], p["w3a"], p["use_skip"]) == (C1A_DIRECT, C1B_CONV, 0, 0, 0, 0)
    assert (p["heads_sparse_da"], p["tails_f32"], p["det"], p["desc"], p["dense_valid"], p["heads_full"]) == (0, 1, DET_MFMA_F32, DESC_GATHER_F32, 0, 1)
    for prec in (F16, SPLIT, F32):                                  # OMNI_CONV_V1 = 1 (no mask-skip plan is made for it)
        p = _row(rows, prec=prec, cv=1, mask_skip=0)
        assert (p["det"], p["cand_fused"], p["heads_sparse_da"], p["dense_valid"], p["use_skip"]) == (DET_VALU, 0, 0, 1, 0)
        assert p["desc"] == DESC_DENSE_GENERIC and (prec == SPLIT or p["conv1b"] == C1B_CONV)


def _skip(pin, prec, passes, split_fuse1a=1):
    """passes (aligned4, mask, stride) -> per pass (calibrates, zero image offset, state afterwards, skips)"""
    out = subprocess.run([pin, "skip", str(prec), str(split_fuse1a)] + [str(v) for p in passes for v in p], capture_output=True, check=True, text=True).stdout
    return [tuple(int(v) for v in line.split()) for line in out.splitlines()]


def test_mask_skip_state_over_sequences_of_passes(pin):
    for prec in (F16, SPLIT):
        # masked aligned twice: one calibration
        assert _skip(pin, prec, [(1, 1, 600), (1, 1, 600)]) == [(1, 0, READY_FUSED, 1), (0, 0, READY_FUSED, 1)]
        # an unmasked pass overwrites the rectangles
        assert _skip(pin, prec, [(1, 1, 600), (1, 0, 600), (1, 1, 600)]) == [(1, 0, READY_FUSED, 1), (0, 0, STALE, 0), (1, 0, READY_FUSED, 1)]
    # split: the unaligned pass skips too, with conv1a's own rectangle: calibrates again, one byte into the zero image when the stride alone would allow the fusion
    assert _skip(pin, SPLIT, [(1, 1, 600), (0, 1, 600)]) == [(1, 0, READY_FUSED, 1), (1, 1, READY_UNFUSED, 1)]
    assert _skip(pin, SPLIT, [(1, 1, 600), (0, 1, 602)]) == [(1, 0, READY_FUSED, 1), (1, 0, READY_UNFUSED, 1)]
    assert _skip(pin, SPLIT, [(0, 1, 600), (0, 1, 602), (1, 1, 600)]) == [(1, 1, READY_UNFUSED, 1), (0, 0, READY_UNFUSED, 1), (1, 0, READY_FUSED, 1)]
    assert _skip(pin, SPLIT, [(1, 1, 600), (1, 1, 600)], split_fuse1a=0) == [(1, 1, READY_UNFUSED, 1), (0, 0, READY_UNFUSED, 1)]
    # fp16: the unaligned pass does not skip, and invalidates
    assert _skip(pin, F16, [(1, 1, 600), (0, 1, 600), (1, 1, 600)]) == [(1, 0, READY_FUSED, 1), (0, 0, STALE, 0), (1, 0, READY_FUSED, 1)]


def _body(src, name):
    """the definition of the static function `name` (a line that starts with its signature and opens a brace) up to the closing brace in column 0"""
    m = re.search(r"^static [^\n;]*\b%s\([^;{]*\{\n.*?^\}\n" % name, src, re.S | re.M)
    assert m, name
    return m.group(0)


def test_the_host_code_decides_nothing_next_to_the_plan():
    src = open(os.path.join(CSRC, "superpoint.hip")).read()
    for fn in ("sp_forward", "sp_make_dense", "sp_calibrate_mask_skip"):
        body = _body(src, fn)
        for word in ("s->cfg", "OMNI_PREC_", "s->wino", "s->sparse_", "s->det16", "s->conv_variant", "s->facts.", "ConvArgs a;"):
            assert word not in body, (fn, word)
    assert "sp_plan_pass(s->facts, in)" in _body(src, "sp_forward")
    owner = re.search(r"^struct DevMem \{\n.*?^\};\n", open(os.path.join(CSRC, "common.h")).read(), re.S | re.M).group(0)     # (shared with omni_vlad)
    assert owner.count("hipFree") == 1 and src.count("hipFree") == 0 and src.count("hipMalloc(") == 0 and owner.count("hipMalloc(") == 1
    assert len(re.findall(r"^\s*ConvArgs \w+;", src, re.M)) == 1 and "ConvArgs a;" in _body(src, "sp_layer_args")
    # plain host C++: nothing of HIP in the plan's header
    plan = open(os.path.join(CSRC, "sp_plan.h")).read()
    assert "hip/" not in plan and "__device__" not in plan and "common.h" not in plan
