"""The JPEG decoder's host entries inside the library (csrc/jpeg_dec_host.cpp: csrc/jpeg_dec_plan.h compiled by g++ into libomni_hip.so) through ctypes, no GPU:
omni_jpegdec_classify, omni_jpeg_decode_host, omni_jpeg_decode_parallel_host against the committed Pillow pixels (tests/golden/jpegdec_cases.npz), the round trip
omni_jpeg_encode_host -> omni_jpeg_decode_host against Pillow's decode of the same bytes, the refusals, the config entry, and that the headers and capi.py name
every new entry."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

from tests import jpegdec_cases as J

ROOT = J.ROOT


def test_classification_and_pixels_of_every_fixture(omni):
    c = omni.capi
    assert (c.JPEGDEC_OK, c.JPEGDEC_HOST, c.JPEGDEC_UNSUPPORTED, c.JPEGDEC_CORRUPT) == (J.OK, J.HOST, J.UNSUPPORTED, J.CORRUPT)
    for name, (w, h, _, _, cls) in J.SPECS.items():
        data = J.file_of(name)
        st, ww, hh = c.jpegdec_classify(data)
        assert st == cls, name
        if cls == J.UNSUPPORTED:
            before = np.full((64, 96), 0xA5, np.uint8)
            status, wv, hv = C.c_int(-1), C.c_int(), C.c_int()
            assert c.lib().omni_jpeg_decode_host(data, len(data), before.ctypes.data, 96, C.byref(wv), C.byref(hv), C.byref(status)) == c.OK
            assert status.value == J.UNSUPPORTED and (before == 0xA5).all()
            continue
        assert (ww, hh) == (w, h), name
        status, pix = c.jpeg_decode_host(data)
        assert status == cls and np.array_equal(pix, J.pixels_of(name)), name
        for S in (128, 1024):
            status, pix, stats = c.jpeg_decode_parallel_host(data, S)
            assert status == cls and np.array_equal(pix, J.pixels_of(name)), (name, S)
            assert (stats["n_sub"] >= 1 and stats["subseq_bits"] == S) == (cls == J.OK)


def test_stride_above_width_leaves_the_bytes_between_rows(omni):
    c = omni.capi
    for name in ("gray_17x13_q75", "color_72x40_422", "rst_96x64_q75"):
        w = J.SPECS[name][0]
        status, pix = c.jpeg_decode_host(J.file_of(name), stride=w + 5)
        assert np.array_equal(pix[:, :w], J.pixels_of(name)) and (pix[:, w:] == 0xA5).all(), name


def test_round_trip_through_the_projects_encoder_equals_pillows_decode(omni):
    """omni_jpeg_encode_host -> omni_jpeg_decode_host == Pillow's decode of the same bytes"""
    from PIL import Image
    c = omni.capi
    n = 0
    for name in ("gray_8x8_q75", "gray_17x13_q100", "noise_96x64_q100", "gray_160x120_q75"):
        g = np.ascontiguousarray(J.pixels_of(name))
        for q in (10, 75, 100):
            st, data = c.jpeg_encode_host(g, q)
            assert st == c.JPEG_OK
            assert c.jpegdec_classify(data) == (J.OK, g.shape[1], g.shape[0])
            status, pix = c.jpeg_decode_host(data)
            ref = np.asarray(Image.open(io.BytesIO(data)))
            assert status == J.OK and np.array_equal(pix, ref), (name, q)
            assert np.array_equal(c.jpeg_decode_parallel_host(data, 128)[1], ref), (name, q)
            n += 1
    print(f"{n} round trips equal Pillow's decode")


def test_mutated_scans_same_status_and_pixels_from_both_entries(omni):
    c = omni.capi
    for what, data in J.mutations():
        st, pix = c.jpeg_decode_host(data)
        st_p, pix_p, _ = c.jpeg_decode_parallel_host(data, 128)
        assert st == st_p and st in (J.OK, J.CORRUPT) and np.array_equal(pix, pix_p), what
        assert st == J.OK or not pix.any(), what


def test_refusals(omni):
    c = omni.capi
    L = c.lib()
    data = J.file_of("gray_17x13_q75")
    out = np.empty((13, 32), np.uint8)
    w, h, st = C.c_int(), C.c_int(), C.c_int()
    args = (C.byref(w), C.byref(h), C.byref(st))
    assert L.omni_jpeg_decode_host(data, len(data), out.ctypes.data, 17, *args) == c.OK and (w.value, h.value, st.value) == (17, 13, J.OK)
    assert L.omni_jpeg_decode_host(data, len(data), out.ctypes.data, 16, *args) == c.ERR_INVALID and b"stride" in L.omni_last_error()
    assert L.omni_jpeg_decode_host(None, 0, out.ctypes.data, 17, *args) == c.ERR_INVALID
    assert L.omni_jpeg_decode_host(data, len(data), None, 17, *args) == c.ERR_INVALID
    stats = (C.c_int * 4)()
    for S in (64, 100, 131072):
        assert L.omni_jpeg_decode_parallel_host(data, len(data), S, out.ctypes.data, 17, *args, stats) == c.ERR_INVALID and b"power of two" in L.omni_last_error()
    assert c.jpegdec_classify(b"") == (J.CORRUPT, 0, 0)


def test_the_subsequence_length_is_a_config_entry(omni):
    c = omni.capi
    o, = [o for o in c.config_table() if o["env"] == "OMNI_JPEGDEC_SUBSEQ_BITS"]
    assert o["lo"] == 128 and o["hi"] >= 4096 and o["default"] & (o["default"] - 1) == 0 and o["lo"] <= o["default"] <= o["hi"]
    assert not c.lib().omni_config_is_process_wide(c.config_table().index(o))                 # a handle's snapshot: tests switch it per handle


def test_headers_and_bindings_name_the_new_entries(omni):
    c = omni.capi
    header = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    new = ["omni_jpegdec_create", "omni_jpegdec_destroy", "omni_jpegdec_enqueue_host", "omni_jpegdec_last_stats", "omni_jpegdec_last_ms", "omni_jpegdec_debug_buffers",
           "omni_jpegdec_classify", "omni_jpeg_decode_host", "omni_jpeg_decode_parallel_host", "omni_cam_enqueue_jpeg_host", "omni_cam_jpegdec_status"]
    for s in new:
        assert re.search(rf"\b{s}\(", header) and s in c.SYMBOLS and hasattr(c.lib(), s), s
    for word in ("OMNI_JPEGDEC_OK", "OMNI_JPEGDEC_HOST", "OMNI_JPEGDEC_UNSUPPORTED", "OMNI_JPEGDEC_CORRUPT", "UNPINNED"):
        assert word in header
    assert "enqueue_jpeg_async" in open(os.path.join(ROOT, "omni-swarm_amd", "host", "omni_swarm.hpp")).read()
    assert hasattr(c.Cam, "enqueue_jpeg_host") and hasattr(c.Cam, "jpegdec_status")


def test_the_pipeline_library_and_the_settings_file_key(omni):
    """lib/libomni_host_jpegdec.so exports what include/omni_host_jpegdec.h declares, and the VINS settings file's is_compressed_images is read (no GPU)"""
    from omni_swarm_amd import pipeline
    L = pipeline.jpegdec_lib()
    header = open(os.path.join(ROOT, "include", "omni_host_jpegdec.h")).read()
    for s in pipeline.JPEGDEC_SYMBOLS:
        assert hasattr(L, s) and re.search(rf"\b{s}\(", header), s
    present = C.c_int(-1)
    for text, want, found in (("%YAML:1.0\nimu: 1\nis_compressed_images: 1\nimage_width: 640\n", 1, 1), ("is_compressed_images : 0\n", 0, 1), ("  is_compressed_images: 2 # yes\n", 1, 1),
                              ("#is_compressed_images: 1\nnum_of_cam: 2\n", 0, 0), ("", 0, 0)):
        assert L.omni_swarm_vins_is_compressed_images(text.encode(), C.byref(present)) == want and present.value == found, text
    assert L.omni_pipeline_set_compressed_images(None, 1) == 1 and b"null pipeline" in L.omni_jpegdec_host_last_error()
    src = open(os.path.join(ROOT, "omni-swarm_amd", "host", "keyframe_pipeline.hpp")).read()
    assert "bool compressed_images = false;" in src and "jpeg_corrupt()" in src                 # off by default
    import inspect
    assert inspect.signature(pipeline.KeyframePipeline.__init__).parameters["compressed_images"].default is False
