"""The cases of the JPEG decoder's restart-interval path (OMNI_JPEGDEC_RESTART_WGS; csrc/jpeg_dec_plan.h plan_chunks / decode_planned_host,
csrc/jpeg_dec.hip), shared by the CPU and the GPU tier: files with restart markers as Pillow writes them and Pillow's pixels for them, from the committed fixture
tests/golden/jpegdec_restart_cases.npz (written by tools/gen_jpegdec_restart_golden.py; the tests never import Pillow), the mutations derived from one of them,
and the g++ pin program around the header (tests/cpp/jpegdec_restart_pin.cpp).

DIVERGENCE, asserted as such by both tiers: a file whose interval lost its last bytes while the marker behind it stayed.  The sequential host decoder
(decode_sequential) reads on into the next interval's bits and returns a decoded picture (HOST); the restart path bounds every interval to its own bits and says
CORRUPT, the picture all zeros.  libjpeg's own resynchronisation is unpinned either way."""
import os
import struct
import subprocess

import numpy as np

from tests import jpegdec_cases as J

ROOT, PKG = J.ROOT, J.PKG
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpegdec_restart_cases.npz")
OK, HOST, UNSUPPORTED, CORRUPT = J.OK, J.HOST, J.UNSUPPORTED, J.CORRUPT
MAX_SUBSEQ = 4096                                              # csrc/jpeg_dec_plan.h JD_MAX_SUBSEQ

# name -> (w, h, content, Pillow's save arguments, restart intervals, the fixture's pixel array)
SPECS = {
    "blk1_gray_96x64_q75": (96, 64, "scene", dict(quality=75, restart_marker_blocks=1), 96, None),                 # every block its own interval
    "rows_gray_96x64_q75": (96, 64, "scene", dict(quality=75, restart_marker_rows=1), 8, None),                    # restart = 12
    "rows_noise_96x64_q100": (96, 64, "noise", dict(quality=100, restart_marker_rows=1), 8, None),                 # ~10 kB: dozens of subsequences per interval at S = 128
    "blk1_gray_17x13_q75": (17, 13, "scene", dict(quality=75, restart_marker_blocks=1), 6, None),                  # no multiple of 8
    "blk3_color_72x40_422": (72, 40, "color", dict(quality=75, subsampling="4:2:2", restart_marker_blocks=3), 9, None),      # bpm 4; 25 MCUs: the last interval is short
    "rows_color_80x48_420_q90_opt": (80, 48, "color", dict(quality=90, subsampling="4:2:0", optimize=True, restart_marker_rows=1), 3, None),      # bpm 6
    "rows_gray_640x480_q75": (640, 480, "scene", dict(quality=75, restart_marker_rows=1), 60, "gray_640x480_q75"),
    "blk1_gray_640x480_q75": (640, 480, "scene", dict(quality=75, restart_marker_blocks=1), 4800, "gray_640x480_q75"),       # more intervals than MAX_SUBSEQ
}
# the key-frame unit's frames (network size): the same pictures as files without and with restart markers, cam_plain_<k> / cam_rows_<k>
CAM_W, CAM_H, CAM_FRAMES = 128, 96, 3
CAM_SAVE = (dict(quality=75), dict(quality=85), dict(quality=60))                    # every file below the unit decoder's capacity, CAM_W * CAM_H / 2 bytes


def cam_image(k: int) -> np.ndarray:
    return np.ascontiguousarray(np.roll(J.make_image("scene", CAM_W, CAM_H), 7 * k, axis=1))


MANY = "blk1_gray_640x480_q75"                                 # W = 1 cannot plan it (HOST); W >= 2 can
MUTATED = "rows_gray_96x64_q75"
WGS = (1, 3, 8)

_fix = None


def fixture():
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as z:
            _fix = {k: z[k] for k in z.files}
    return _fix


def file_of(name: str) -> bytes:
    return fixture()["jpg_" + name].tobytes()


def pixels_of(name: str) -> np.ndarray:
    return fixture()["pix_" + (SPECS[name][5] or name)]


def names():
    return list(SPECS)


def plannable(name: str, W: int) -> bool:
    return name != MANY or W >= 2


def markers(data: bytes):
    """the offsets of the restart markers in the file's scan (0xFF 0xD0..0xD7: entropy-coded data holds no other 0xFF that is not followed by 0x00)"""
    lo, hi = J.scan_range(data)
    return [p for p in range(lo, hi - 1) if data[p] == 0xFF and 0xD0 <= data[p + 1] <= 0xD7]


def mutations():
    """[(what, bytes, status of the host decoder, status of the restart path)] of the 96 x 64 rows = 1 file (7 markers)"""
    data = file_of(MUTATED)
    m = markers(data)
    assert len(m) == 7
    return [("cut 40 bytes behind the 4th marker", data[:m[3] + 2 + 40], CORRUPT, CORRUPT),
            ("the 3rd marker removed", data[:m[2]] + data[m[2] + 2:], CORRUPT, CORRUPT),
            ("the last 30 bytes of the 3rd interval removed, its marker kept", data[:m[2] - 30] + data[m[2]:], HOST, CORRUPT)]      # the DIVERGENCE (above)


# ---- the pin program -------------------------------------------------------------------------------------------------------------------------------------
def build_pin(tmp, sanitize: bool = True) -> str:
    exe = os.path.join(str(tmp), "jpegdec_restart_pin" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "jpegdec_restart_pin.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe: str, jobs, tmp) -> list:
    """jobs: [(file bytes, S, W, max_sub)] -> [dict(status, w, h, n_sub, S, chunks, rounds, plan -- the planner's own verdict --, pixels [h][w] or None)]"""
    fin, fout = os.path.join(str(tmp), "rpin_in.bin"), os.path.join(str(tmp), "rpin_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for data, S, W, max_sub in jobs:
            f.write(struct.pack("4i", len(data), S, W, max_sub))
            f.write(data)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    d, p, out = open(fout, "rb").read(), 0, []
    for _ in jobs:
        st, w, h, n_sub, S, chunks, rounds, plan, has = struct.unpack_from("9i", d, p)
        p += 36
        pix = None
        if has:
            pix = np.frombuffer(d, np.uint8, w * h, p).reshape(h, w)
            p += w * h
        out.append(dict(status=st, w=w, h=h, n_sub=n_sub, S=S, chunks=chunks, rounds=rounds, plan=plan, pixels=pix))
    assert p == len(d)
    return out
