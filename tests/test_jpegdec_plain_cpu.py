"""Files without a restart interval over several workgroups, without a GPU: the partition, the S rule and the CPU stand-in for the kernels of a handle whose
OMNI_JPEGDEC_PLAIN_WGS is W >= 2 (csrc/jpeg_dec_plan.h plain_chunks / plain_subseq_bits / decode_planned_host with plain_wgs = W; inside the library through
omni_jpeg_decode_plain_parallel_host, and as a g++ program of its own under -fsanitize=address,undefined) against the committed Pillow pixels
(tests/golden/jpegdec_cases.npz), the sequential host decoder and the same stand-in with the switch off (one chunk), for every OK fixture, S in {default, 128} and W in {2, 3, 8};
the three ends of the relaxation; the chunk cap; the 40 mutations; the config entry and the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_plain_cases as P


def default_S(c) -> int:
    return [o for o in c.config_table() if o["env"] == P.S_ENV][0]["default"]


@pytest.mark.parametrize("name", J.names(J.OK))
def test_stand_in_equals_pillow_the_sequential_decoder_and_the_one_chunk_stand_in(omni, name):
    c = omni.capi
    data, want = J.file_of(name), J.pixels_of(name)
    st_h, pix_h = c.jpeg_decode_host(data)
    assert st_h == P.OK and np.array_equal(pix_h, want)
    for S in (default_S(c), 128):
        st_1, pix_1, one = c.jpeg_decode_parallel_host(data, S)                                # the stand-in with the switch off: one chunk
        assert st_1 == P.OK and np.array_equal(pix_1, want)
        for W in P.WGS:
            st, pix, stats = c.jpeg_decode_plain_parallel_host(data, S, W)
            assert st == P.OK and P.differing(pix, want) == 0 and P.differing(pix, pix_h) == 0 and P.differing(pix, pix_1) == 0, (name, S, W, st)
            assert stats["subseq_bits"] == S and stats["n_sub"] == one["n_sub"], (name, S, W, stats)      # (no fixture needs a longer subsequence)
            assert stats["chunks"] == max(1, min(W, stats["n_sub"])) and stats["seam_changed"] >= stats["seam_chunks"] and stats["seam_chunks"] < stats["chunks"]
            assert (stats["seam_rounds"] == 0) == (stats["seam_changed"] == 0)


def test_the_three_ends_of_the_relaxation(omni):
    c = omni.capi
    st, _, s = c.jpeg_decode_plain_parallel_host(J.file_of("gray_160x120_q75"), 1024, 2)      # the seam's guess is wrong, the exit state behind it already right
    assert st == P.OK and s["chunks"] == 2 and s["seam_changed"] == 0 and s["seam_rounds"] == 0, s
    st, _, s = c.jpeg_decode_plain_parallel_host(J.file_of("noise_96x64_q100"), 128, 8)      # a repair that runs through the later chunks
    assert st == P.OK and s["chunks"] == 8 and s["seam_rounds"] >= 2 and s["seam_chunks"] >= 2, s
    print("noise_96x64_q100 S=128 W=8:", s)
    st, _, s = c.jpeg_decode_plain_parallel_host(J.file_of("gray_8x8_q100"), 128, 8)         # chunks of one subsequence: the seam relaxation does all of it
    assert st == P.OK and s["n_sub"] == 4 and s["chunks"] == 4 and s["chunk_rounds"] == 0, s
    assert s["seam_rounds"] == c.jpeg_decode_parallel_host(J.file_of("gray_8x8_q100"), 128)[2]["rounds"]
    for W in (2, 8, 64):
        st, _, s = c.jpeg_decode_plain_parallel_host(J.file_of("gray_8x8_q5"), 128, W)       # one subsequence, one chunk
        assert st == P.OK and (s["n_sub"], s["chunks"], s["rounds"], s["seam_changed"]) == (1, 1, 0, 0), s


def test_a_small_workgroup_doubles_the_subsequence_length_only_until_the_chunks_hold_the_picture(omni):
    c = omni.capi
    data, want = J.file_of("gray_96x64_q75"), J.pixels_of("gray_96x64_q75")
    assert c.jpeg_decode_parallel_host(data, 128)[2]["n_sub"] == 110
    st, pix, s = c.jpeg_decode_plain_parallel_host(data, 128, 2, 8)                            # 55 per chunk: S doubles until a chunk holds <= 8
    assert st == P.OK and np.array_equal(pix, want) and s["subseq_bits"] > 128 and s["chunks"] == 2 and 8 < s["n_sub"] <= 16, s
    assert c.jpeg_decode_parallel_host(data, s["subseq_bits"] // 2)[2]["n_sub"] > 16           # ... and no further
    st, pix, s = c.jpeg_decode_plain_parallel_host(data, 128, 16, 8)                           # 16 chunks of 6 or 7: nothing to double
    assert st == P.OK and np.array_equal(pix, want) and (s["subseq_bits"], s["n_sub"], s["chunks"]) == (128, 110, 16), s


def test_the_mutations_equal_the_one_chunk_stand_in(omni):
    """the stand-in with the switch off (one chunk) is the yardstick for corrupt input: same status, same pixels under either switch value"""
    c = omni.capi
    seen = set()
    for what, data in J.mutations():
        st_1, pix_1, _ = c.jpeg_decode_parallel_host(data, 128)
        st, pix, _ = c.jpeg_decode_plain_parallel_host(data, 128, 3)
        assert st == st_1 and P.differing(pix, pix_1) == 0 and (st != P.CORRUPT or not pix.any()), (what, st, st_1)
        seen.add(st)
    assert seen == {P.OK, P.CORRUPT}                                                           # the program holds both ends


def test_files_the_kernels_do_not_spread_go_the_way_they_went(omni):
    c = omni.capi
    for name in ("rst_96x64_q75", "rst_color_80x48_420"):                                      # a restart interval: the sequential decoder, HOST
        st, pix, s = c.jpeg_decode_plain_parallel_host(J.file_of(name), 128, 8)
        assert st == P.HOST and np.array_equal(pix, J.pixels_of(name)) and not any(s.values()), (name, s)
    assert c.jpeg_decode_plain_parallel_host(J.file_of("prog_96x64_q75"), 128, 8)[0] == P.UNSUPPORTED


def test_planner_and_stand_in_run_clean_under_the_sanitizers(omni, tmp_path):
    """a g++ program of its own (tests/cpp/jpegdec_plain_pin.cpp) with -fsanitize=address,undefined: every OK fixture and the mutations; the partition's invariants
    -- chunks cover [0, n_sub) without gap or overlap, none empty, none above max_sub -- are checked there, for these cases and for a sweep of sizes"""
    c = omni.capi
    exe = P.build_pin(tmp_path, sanitize=True)
    jobs = []
    for name in J.names(J.OK):
        for S in (1024, 128):
            for W in P.WGS:
                if name == "gray_640x480_q75" and (S, W) not in ((1024, 8), (128, 3)):
                    continue                                                                   # (the large picture: two of the six combinations)
                jobs.append((name, J.file_of(name), S, W, P.MAX_SUBSEQ))
    jobs += [("gray_96x64_q75", J.file_of("gray_96x64_q75"), 128, W, 8) for W in (2, 16)]
    jobs += [("rst_96x64_q75", J.file_of("rst_96x64_q75"), 128, 3, P.MAX_SUBSEQ)]
    jobs += [(None, data, 128, 3, P.MAX_SUBSEQ) for _, data in J.mutations()]
    got = P.run_pin(exe, [j[1:] for j in jobs], tmp_path)
    for (name, data, S, W, max_sub), g in zip(jobs, got):
        st, pix, s = c.jpeg_decode_plain_parallel_host(data, S, W, max_sub)                    # the same header inside the library
        assert g["status"] == st and np.array_equal(g["pixels"], pix), (name, S, W)
        assert (g["n_sub"], g["S"], g["chunks"], g["chunk_rounds"], g["seam_rounds"], g["seam_changed"], g["seam_chunks"]) == \
            (s["n_sub"], s["subseq_bits"], s["chunks"], s["chunk_rounds"], s["seam_rounds"], s["seam_changed"], s["seam_chunks"]), (name, S, W)
        if name:
            assert np.array_equal(g["pixels"], J.pixels_of(name)), (name, S, W)


def test_the_switch_is_a_per_handle_tuning_entry_off_by_default(omni, monkeypatch):
    c = omni.capi
    table = c.config_table()
    o, = [o for o in table if o["env"] == P.W_ENV]
    CFG_TUNING = 1                                                                             # csrc/config.h CfgClass
    assert (o["default"], o["lo"], o["hi"], o["cls"]) == (0, 0, 64, CFG_TUNING)
    assert not c.lib().omni_config_is_process_wide(table.index(o))                             # a handle's snapshot
    monkeypatch.delenv(P.W_ENV, raising=False)
    assert c.config_value(P.W_ENV) == 0
    monkeypatch.setenv(P.W_ENV, "8")
    assert c.config_value(P.W_ENV) == 8
    for bad in ("65", "-1", "two"):                                                            # what a handle's creation resolves, and refuses
        monkeypatch.setenv(P.W_ENV, bad)
        with pytest.raises(c.OmniError, match=P.W_ENV):
            c.config_value(P.W_ENV)


def test_abi_version_header_and_bindings(omni):
    c = omni.capi
    assert c.lib().omni_abi_version() == 2 == c.ABI_VERSION
    header = open(os.path.join(J.ROOT, "include", "omni_hip.h")).read()
    for s in ("omni_jpeg_decode_plain_parallel_host", "omni_jpegdec_last_seam", "omni_jpegdec_debug_state_buffer"):
        assert re.search(rf"\b{s}\(", header) and s in c.SYMBOLS and hasattr(c.lib(), s), s
    assert P.W_ENV in header and "#define OMNI_ABI_VERSION 2" in header
    L = c.lib()
    data = J.file_of("gray_17x13_q75")
    out = np.empty((13, 17), np.uint8)
    w, h, st = C.c_int(), C.c_int(), C.c_int()
    stats = (C.c_int * 7)()
    for S, W, M, word in ((100, 2, 4096, b"power of two"), (128, 0, 4096, b"workgroups"), (128, 65, 4096, b"workgroups"), (128, 2, 0, b"workgroups")):
        assert L.omni_jpeg_decode_plain_parallel_host(data, len(data), S, W, M, out.ctypes.data, 17, C.byref(w), C.byref(h), C.byref(st), stats) == c.ERR_INVALID
        assert word in L.omni_last_error(), (S, W, M)
    assert L.omni_jpeg_decode_plain_parallel_host(data, len(data), 128, 2, 4096, out.ctypes.data, 17, C.byref(w), C.byref(h), C.byref(st), stats) == 0
    assert (w.value, h.value, st.value) == (17, 13, P.OK) and np.array_equal(out, J.pixels_of("gray_17x13_q75"))
