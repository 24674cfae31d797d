"""The restart-interval path of the JPEG decoder without a GPU: the chunk plan and the CPU stand-in for the kernels of a handle whose OMNI_JPEGDEC_RESTART_WGS is
on (csrc/jpeg_dec_plan.h plan_chunks / decode_planned_host with restart_wgs = W; inside the library through omni_jpeg_decode_restart_parallel_host, and as a g++ program
of its own under -fsanitize=address,undefined) against the committed Pillow pixels (tests/golden/jpegdec_restart_cases.npz) and the sequential host decoder, for
every fixture, S in {default, 128} and W in {1, 3, 8}; the mutations and the one documented divergence (tests/jpegdec_restart_cases.py); the config entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_restart_cases as R

W_ENV, S_ENV = "OMNI_JPEGDEC_RESTART_WGS", "OMNI_JPEGDEC_SUBSEQ_BITS"


@pytest.fixture(scope="module")
def sequential(omni):
    """name -> pixels of the sequential host decoder (HOST, Pillow's pixels); computed once"""
    out = {}
    for name in R.names():
        st, pix = omni.capi.jpeg_decode_host(R.file_of(name))
        assert st == R.HOST and np.array_equal(pix, R.pixels_of(name)), name
        out[name] = pix
    return out


@pytest.mark.parametrize("name", R.names())
def test_stand_in_equals_pillow_and_the_sequential_decoder_pixel_for_pixel(omni, sequential, name):
    c = omni.capi
    data, n_int = R.file_of(name), R.SPECS[name][4]
    assert c.jpegdec_classify(data)[0] == R.HOST                                               # parse() is as it was
    default = [o for o in c.config_table() if o["env"] == S_ENV][0]["default"]
    for S in (default, 128):
        for W in R.WGS:
            st, pix, stats = c.jpeg_decode_restart_parallel_host(data, S, W)
            assert np.array_equal(pix, R.pixels_of(name)) and np.array_equal(pix, sequential[name]), (name, S, W)
            if not R.plannable(name, W):
                assert st == R.HOST and stats == dict(n_sub=0, subseq_bits=0, chunks=0, rounds=0), (name, S, W, st, stats)
                continue
            assert st == R.OK and 1 <= stats["chunks"] <= min(W, n_int) and stats["n_sub"] >= n_int, (name, S, W, st, stats)
            assert stats["subseq_bits"] >= S and stats["subseq_bits"] & (stats["subseq_bits"] - 1) == 0 and stats["n_sub"] <= stats["chunks"] * R.MAX_SUBSEQ
            if R.SPECS[name][0] < 640:                                                         # (the small files fit any chunk at any S)
                assert stats["subseq_bits"] == S
    if name == "rows_noise_96x64_q100":
        assert c.jpeg_decode_restart_parallel_host(data, 128, 1)[2]["rounds"] > 0              # intervals of dozens of subsequences: relaxation runs
    if name == "rows_gray_640x480_q75":
        assert c.jpeg_decode_restart_parallel_host(data, default, 8)[2]["chunks"] > 1


def test_a_small_workgroup_doubles_the_subsequence_length_or_leaves_the_file_to_the_host(omni):
    """max_subseq below the kernels' 4096: S is doubled until every chunk fits; more intervals in a chunk than max_subseq cannot be planned"""
    c = omni.capi
    name = "rows_noise_96x64_q100"
    data = R.file_of(name)
    st, pix, stats = c.jpeg_decode_restart_parallel_host(data, 128, 1, 64)
    assert st == R.OK and np.array_equal(pix, R.pixels_of(name)) and stats["subseq_bits"] > 128 and stats["n_sub"] <= 64, stats
    st, pix, stats = c.jpeg_decode_restart_parallel_host(data, 128, 1, 7)                      # 8 intervals
    assert st == R.HOST and np.array_equal(pix, R.pixels_of(name)) and stats["chunks"] == 0
    st, pix, stats = c.jpeg_decode_restart_parallel_host(data, 128, 8, 7)
    assert st == R.OK and np.array_equal(pix, R.pixels_of(name)) and stats["chunks"] > 1 and stats["n_sub"] <= 7 * stats["chunks"]


def test_files_without_a_restart_interval_go_the_way_of_the_parallel_stand_in(omni):
    c = omni.capi
    for name in ("gray_96x64_q75", "color_80x48_420", "rst_96x64_q75", "rst_color_80x48_420"):
        data = J.file_of(name)
        st, pix, stats = c.jpeg_decode_restart_parallel_host(data, 128, 3)
        st_p, pix_p, stats_p = c.jpeg_decode_parallel_host(data, 128)
        assert np.array_equal(pix, J.pixels_of(name)), name
        if name.startswith("rst_"):                                                            # the existing restart fixtures: planned as well
            assert st == R.OK and st_p == R.HOST and stats["chunks"] >= 1
        else:
            assert st == st_p == R.OK and (stats["n_sub"], stats["subseq_bits"], stats["chunks"], stats["rounds"]) == (stats_p["n_sub"], 128, 1, stats_p["rounds"])


def test_mutations_and_the_documented_divergence(omni):
    c = omni.capi
    for what, data, st_host, st_restart in R.mutations():
        st, pix = c.jpeg_decode_host(data)
        assert st == st_host and (st != R.CORRUPT or not pix.any()), (what, st)
        for S in (128, 1024):
            for W in R.WGS:
                st, pix, _ = c.jpeg_decode_restart_parallel_host(data, S, W)
                assert st == st_restart == R.CORRUPT and pix.shape == (64, 96) and not pix.any(), (what, S, W, st)


def test_planner_and_stand_in_run_clean_under_the_sanitizers(tmp_path):
    """a g++ program of its own (tests/cpp/jpegdec_restart_pin.cpp) with -fsanitize=address,undefined: every fixture and mutation, planner invariants checked there"""
    exe = R.build_pin(tmp_path, sanitize=True)
    jobs, want = [], []
    for name in R.names():
        for S in (1024, 128):
            for W in R.WGS:
                if name.endswith("640x480_q75") and (S, W) not in ((1024, 1), (128, 3), (1024, 8)):
                    continue                                                                   # (the large pictures: three of the six combinations)
                jobs.append((R.file_of(name), S, W, R.MAX_SUBSEQ))
                want.append((R.OK if R.plannable(name, W) else R.HOST, R.pixels_of(name)))
    for what, data, _, st_restart in R.mutations():
        for W in R.WGS:
            jobs.append((data, 128, W, R.MAX_SUBSEQ))
            want.append((st_restart, np.zeros((64, 96), np.uint8)))
    jobs.append((R.file_of("rows_noise_96x64_q100"), 128, 1, 64))
    want.append((R.OK, R.pixels_of("rows_noise_96x64_q100")))
    jobs.append((J.file_of("gray_96x64_q75"), 128, 3, R.MAX_SUBSEQ))                           # no restart interval: the planner is not asked
    want.append((R.OK, J.pixels_of("gray_96x64_q75")))
    got = R.run_pin(exe, jobs, tmp_path)
    for k, (g, (st, pix)) in enumerate(zip(got, want)):
        assert g["status"] == st and np.array_equal(g["pixels"], pix), (k, g["status"], st)
        assert (g["plan"] == -1) == (k == len(jobs) - 1) and (g["plan"] != R.OK or (g["status"] in (R.OK, R.CORRUPT) and 1 <= g["chunks"] <= jobs[k][2]))


def test_the_switch_is_a_per_handle_tuning_entry_off_by_default(omni, monkeypatch):
    c = omni.capi
    table = c.config_table()
    o, = [o for o in table if o["env"] == W_ENV]
    CFG_TUNING = 1                                                                             # csrc/config.h CfgClass
    assert (o["default"], o["lo"], o["hi"], o["cls"]) == (0, 0, 64, CFG_TUNING)
    assert not c.lib().omni_config_is_process_wide(table.index(o))                             # a handle's snapshot
    assert c.config_value(W_ENV) == 0
    monkeypatch.setenv(W_ENV, "8")
    assert c.config_value(W_ENV) == 8
    for bad in ("65", "-1", "two"):
        monkeypatch.setenv(W_ENV, bad)
        with pytest.raises(c.OmniError, match=W_ENV):
            c.config_value(W_ENV)


def test_abi_version_header_and_bindings(omni):
    c = omni.capi
    assert c.lib().omni_abi_version() == 2 == c.ABI_VERSION
    header = open(os.path.join(J.ROOT, "include", "omni_hip.h")).read()
    for s in ("omni_jpeg_decode_restart_parallel_host", "omni_jpegdec_last_chunks"):
        assert re.search(rf"\b{s}\(", header) and s in c.SYMBOLS and hasattr(c.lib(), s), s
    assert W_ENV in header and "#define OMNI_ABI_VERSION 2" in header
    L = c.lib()
    data = R.file_of("blk1_gray_17x13_q75")
    out = np.empty((13, 17), np.uint8)
    w, h, st = C.c_int(), C.c_int(), C.c_int()
    stats = (C.c_int * 4)()
    for S, W, M, word in ((100, 1, 4096, b"power of two"), (128, 0, 4096, b"workgroups"), (128, 65, 4096, b"workgroups"), (128, 1, 0, b"workgroups")):
        assert L.omni_jpeg_decode_restart_parallel_host(data, len(data), S, W, M, out.ctypes.data, 17, C.byref(w), C.byref(h), C.byref(st), stats) == c.ERR_INVALID
        assert word in L.omni_last_error(), (S, W, M)
