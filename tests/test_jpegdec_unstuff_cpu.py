"""Unstuffing by tiles, without a GPU: csrc/jpeg_dec_plan.h's unstuff_keep / survey / unstuff_tiled_host (the CPU stand-in for jpegdec_unstuff_kernel of a handle whose
OMNI_JPEGDEC_UNSTUFF_DEV is 1) against the byte-wise pass (jd::unstuff) and the byte-wise rules written out in tests/jpegdec_unstuff_cases.py -- equality
everywhere: clean bytes, count, the 16 bytes of padding, restart offsets, raw_end, the tile table -- on seeded strings, patterns across a tile seam and a lane seam,
every committed fixture scan, the 40 mutations and files with fill bytes; the memchr scan_end; the config entry; the bindings; and the same header as a g++ program
of its own under -fsanitize=address,undefined."""
import os
import re

import numpy as np
import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_restart_cases as R
from tests import jpegdec_unstuff_cases as U


def test_tiles_equal_the_byte_wise_pass_on_seeded_strings_and_seam_patterns(omni):
    c = omni.capi
    T = c.jpeg_unstuff_tile_bytes()
    assert T == 4096
    seen_end, seen_whole = 0, 0
    for what, s in U.strings(T):
        assert len(s) < 20 * 1024
        (_, n, _), t = U.check_tiled(c, s, what)
        seen_end += t["raw_end"] < len(s)
        seen_whole += t["raw_end"] == len(s) > T
    assert seen_end >= 10 and seen_whole >= 4                                                   # strings that end at a marker, and strings of several tiles that do not


def test_the_named_runs(omni):
    """FF FF 00 is one 0xFF; FF 00 00 an 0xFF and a zero; FF FF Dn a restart marker with a fill byte; a terminator ends the scan at its run's first 0xFF"""
    c = omni.capi
    for s, want, rst, raw_end in ((b"\x41\xff\xff\x00\x42", b"\x41\xff\x42", [], 5), (b"\xff\x00\x00", b"\xff\x00", [], 3), (b"\x41\xff\xff\xd5\x42", b"\x41\x42", [1], 5),
                                  (b"\x41\xff\xff\xd9\x42", b"\x41", [], 1), (b"\x41\xff\xff", b"\x41", [], 1), (b"", b"", [], 0), (b"\xff", b"", [], 0),
                                  (b"\xff\xd0\xff\xd1", b"", [0, 0], 4), (b"\x00\xff\x00\xff\x01\x41", b"\x00\xff", [], 3)):
        (clean, n, r), t = U.check_tiled(c, s, s)
        assert bytes(clean[:n]) == want and r == rst and t["raw_end"] == raw_end, (s, bytes(clean[:n]), r, t["raw_end"])


def test_tiles_equal_the_byte_wise_pass_on_every_fixture_scan_and_mutation(omni):
    c = omni.capi
    stuffed, markers = [], []
    for name, s in U.fixture_scans() + U.mutation_scans():
        (_, n, rst), t = U.check_tiled(c, s, name)
        stuffed.append(t["raw_end"] - n - 2 * len(rst))
        markers.append(len(rst))
    print(f"stuffed zeros per scan {min(stuffed)}..{max(stuffed)}, restart markers up to {max(markers)}")
    assert min(stuffed) == 0 and max(stuffed) >= 100 and max(markers) == 4799                  # (no fixture holds a fill byte: raw - clean = zeros + 2 per marker)


@pytest.mark.parametrize("extra", [1, 3])
def test_fill_bytes_in_front_of_every_restart_marker(omni, extra):
    c = omni.capi
    data = U.fill_file(extra)
    assert len(data) == len(R.file_of(U.FILL)) + 7 * extra
    lo, hi = J.scan_range(data)
    (_, n, rst), t = U.check_tiled(c, data[lo:hi], extra)
    lo0, hi0 = J.scan_range(R.file_of(U.FILL))
    clean0, n0, rst0 = c.jpeg_unstuff_host(R.file_of(U.FILL)[lo0:hi0])
    assert n == n0 and rst == rst0 and len(rst) == 7 and np.array_equal(t["out"], clean0)       # the fill bytes leave no trace
    assert t["raw_end"] == hi - lo == hi0 - lo0 + 7 * extra
    st, pix = c.jpeg_decode_host(data)
    assert st == U.R.HOST and np.array_equal(pix, R.pixels_of(U.FILL))
    st, pix, _ = c.jpeg_decode_restart_parallel_host(data, 128, 3)
    assert st == U.R.OK and np.array_equal(pix, R.pixels_of(U.FILL))


def test_the_memchr_scan_end_equals_the_byte_wise_rule(omni):
    c = omni.capi
    T = c.jpeg_unstuff_tile_bytes()
    n = 0
    for what, s in U.strings(T) + U.fixture_scans() + U.mutation_scans():
        for p in sorted({0, 1, 2, len(s) // 2, max(len(s) - 2, 0), len(s)}):
            if p <= len(s):
                assert c.jpeg_scan_end(s, p) == U.scan_end_rule(s, p), (what, p)
                n += 1
    assert n > 500 and c.jpeg_scan_end(b"\x41", 2) == -1
    for name in J.names():                                                                     # ... and the parser that uses it still classifies every fixture
        assert c.jpegdec_classify(J.file_of(name))[0] == J.SPECS[name][4], name


def test_the_header_runs_clean_under_the_sanitizers(omni, tmp_path):
    """tests/cpp/jpegdec_unstuff_pin.cpp with -fsanitize=address,undefined, a process of its own: its own patterns, then the strings of the tests above in buffers
    of exactly the promised size; what it reports equals the library's build of the same header"""
    c = omni.capi
    exe = U.build_pin(tmp_path, sanitize=True)
    T = c.jpeg_unstuff_tile_bytes()
    jobs = U.strings(T) + U.fixture_scans() + U.mutation_scans() + [(f"fill {k}", U.fill_file(k)) for k in (1, 3)]
    got = U.run_pin(exe, [s for _, s in jobs], tmp_path)
    for (what, s), g in zip(jobs, got):
        t = c.jpeg_unstuff_tiled_host(s)
        assert (g["n_clean"], g["raw_end"], g["n_rst"], g["n_tiles"], g["scan_end"]) == \
            (t["n_clean"], t["raw_end"], len(t["rst"]), len(t["tile_off"]), U.scan_end_rule(s)), (what, g)


def test_the_switch_is_a_per_handle_tuning_entry_off_by_default(omni, monkeypatch):
    c = omni.capi
    table = c.config_table()
    o, = [o for o in table if o["env"] == U.U_ENV]
    CFG_TUNING = 1                                                                             # csrc/config.h CfgClass
    assert (o["default"], o["lo"], o["hi"], o["cls"]) == (0, 0, 1, CFG_TUNING)
    assert not c.lib().omni_config_is_process_wide(table.index(o))                             # a handle's snapshot
    monkeypatch.delenv(U.U_ENV, raising=False)
    assert c.config_value(U.U_ENV) == 0
    monkeypatch.setenv(U.U_ENV, "1")
    assert c.config_value(U.U_ENV) == 1
    for bad in ("2", "-1", "on"):
        monkeypatch.setenv(U.U_ENV, bad)
        with pytest.raises(c.OmniError, match=U.U_ENV):
            c.config_value(U.U_ENV)


def test_header_and_bindings(omni):
    c = omni.capi
    assert c.lib().omni_abi_version() == c.ABI_VERSION
    header = open(os.path.join(J.ROOT, "include", "omni_hip.h")).read()
    for s in ("omni_jpegdec_last_unstuff", "omni_jpegdec_debug_in_buffer", "omni_jpegdec_unstuff_dev", "omni_jpeg_unstuff_tile_bytes", "omni_jpeg_unstuff_host",
              "omni_jpeg_unstuff_tiled_host", "omni_jpeg_scan_end"):
        assert re.search(rf"\b{s}\(", header) and s in c.SYMBOLS and hasattr(c.lib(), s), s
    assert U.U_ENV in header and hasattr(c.JpegDec, "last_unstuff") and hasattr(c.JpegDec, "unstuff_guard_ok")
    import ctypes as C
    out = np.zeros(8, np.uint8)
    k, nr = C.c_int64(), C.c_int64()
    assert c.lib().omni_jpeg_unstuff_host(b"\x41\x42", 2, out.ctypes.data, 8, C.byref(k), None, 0, C.byref(nr)) == c.ERR_INVALID      # room for 2 + 16
    assert b"room" in c.lib().omni_last_error()
