"""The cases of the JPEG decoder (csrc/jpeg_dec_plan.h, csrc/jpeg_dec.hip), shared by the CPU and the GPU tier: the files and Pillow's pixels for them from the
committed fixture tests/golden/jpegdec_cases.npz (written by tools/gen_jpegdec_golden.py; the GPU tier never imports Pillow), the g++ pin program around the
header, and the fixed mutation program (truncated and byte-flipped scans)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpegdec_cases.npz")
OK, HOST, UNSUPPORTED, CORRUPT = 0, 1, 2, 3

# name -> (w, h, content, Pillow's save arguments, classification)
GRAY_SIZES = [(8, 8), (17, 13), (96, 64)]
SPECS = {}
for _w, _h in GRAY_SIZES:
    for _q in (5, 75, 100):
        SPECS[f"gray_{_w}x{_h}_q{_q}"] = (_w, _h, "scene", dict(quality=_q), OK)
SPECS["noise_96x64_q100"] = (96, 64, "noise", dict(quality=100), OK)                        # 16-bit codes, ZRL
SPECS["opt_96x64_q75"] = (96, 64, "scene", dict(quality=75, optimize=True), OK)             # a DHT that is not Annex K's
SPECS["gray_160x120_q75"] = (160, 120, "scene", dict(quality=75), OK)
SPECS["color_80x48_420"] = (80, 48, "color", dict(quality=75, subsampling="4:2:0"), OK)
SPECS["color_72x40_422"] = (72, 40, "color", dict(quality=75, subsampling="4:2:2"), OK)     # 72 is no multiple of the MCU's 16 columns (40 is one of its 8 rows)
SPECS["color_80x48_444"] = (80, 48, "color", dict(quality=75, subsampling="4:4:4"), OK)
SPECS["gray_640x480_q75"] = (640, 480, "frame", dict(quality=75), OK)                       # the camera's own size
SPECS["rst_96x64_q75"] = (96, 64, "scene", dict(quality=75, restart_marker_blocks=5), HOST)
SPECS["rst_color_80x48_420"] = (80, 48, "color", dict(quality=75, subsampling="4:2:0", restart_marker_blocks=2), HOST)
SPECS["prog_96x64_q75"] = (96, 64, "scene", dict(quality=75, progressive=True), UNSUPPORTED)

PARALLEL_S = [128, 256, 1024, 4096]
MUTATED = "gray_96x64_q75"
N_MUTATIONS = 40


def make_image(content: str, w: int, h: int) -> np.ndarray:
    """gray [h][w] u8, or RGB [h][w][3] u8 for "color" """
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rng = np.random.default_rng(4000 + 131 * w + h)
    if content == "noise":                                     # noise (long codes); the right third the DCT's (7, 7) basis function (long zero runs: ZRL)
        a = rng.integers(0, 256, (h, w)).astype(np.float64)
        basis = 128 + (40 + 3 * (x // 8) + 11 * (y // 8)) * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16)
        a[:, 2 * w // 3:] = np.rint(basis)[:, 2 * w // 3:]
        return a.astype(np.uint8)
    if content == "frame":                                     # a camera-like frame: smooth shading, a few edges, little texture
        a = 120 + 70 * np.sin(x / 53.0) * np.cos(y / 41.0) + 30 * ((x // 80 + y // 60) % 2) + 25 * (np.hypot(x - 400, y - 200) < 90)
        a += rng.normal(0, 1.5, (h, w))
        return np.clip(a, 0, 255).astype(np.uint8)
    a = 128 + 90 * np.sin(x / 5.0 + 0.3) * np.cos(y / 3.5) + 40 * ((x // 7 + y // 5) % 2) + rng.normal(0, 6, (h, w))
    g = np.clip(a, 0, 255).astype(np.uint8)
    if content == "scene":
        return g
    r = np.clip(128 + 100 * np.sin(x / 11.0), 0, 255).astype(np.uint8)
    b = np.clip(128 + 100 * np.cos(y / 6.0) + rng.normal(0, 10, (h, w)), 0, 255).astype(np.uint8)
    return np.stack([r, g, b], axis=-1)


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
    return fixture()["pix_" + name]


def names(status=None):
    return [n for n, s in SPECS.items() if status is None or s[4] == status]


def scan_range(data: bytes):
    """(first byte of the entropy-coded data of the first scan, the EOI's offset) of a baseline file"""
    p = 2
    while True:
        assert data[p] == 0xFF
        m, ln = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        p += 2 + ln
        if m == 0xDA:
            return p, data.rindex(b"\xff\xd9")


def mutations(name: str = MUTATED, n: int = N_MUTATIONS, seed: int = 20240607):
    """[(what, bytes)]: truncated and byte-flipped scans of one fixture, a fixed program"""
    data = file_of(name)
    lo, hi = scan_range(data)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        at = int(rng.integers(lo, hi))
        b = bytearray(data)
        kind = k % 5
        if kind == 0:                                          # the file ends inside the scan
            b = b[:at]
            what = f"cut at {at}"
        elif kind == 1:                                        # the scan ends early, the EOI follows
            b = b[:at] + b"\xff\xd9"
            what = f"cut at {at} + EOI"
        elif kind == 2:
            bit = int(rng.integers(0, 8))
            b[at] ^= 1 << bit
            what = f"bit {bit} of byte {at} flipped"
        elif kind == 3:
            b[at] = int(rng.integers(0, 256))
            what = f"byte {at} = {b[at]:#x}"
        else:                                                  # a burst: 4 bytes replaced
            for j in range(4):
                if at + j < hi:
                    b[at + j] = int(rng.integers(0, 256))
            what = f"bytes {at}..{at + 3} replaced"
        out.append((what, bytes(b)))
    return out


# ---- the pin program -------------------------------------------------------------------------------------------------------------------------------------
def build_pin(tmp, sanitize: bool = False) -> str:
    exe = os.path.join(str(tmp), "jpegdec_plan_pin" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "jpegdec_plan_pin.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe: str, jobs, tmp) -> list:
    """jobs: [(file bytes, S -- 0: the sequential decoder --, max_sub)] -> [dict(status, w, h, n_sub, S, rounds, wrong, pixels [h][w] or None)]"""
    fin, fout = os.path.join(str(tmp), "pin_in.bin"), os.path.join(str(tmp), "pin_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for data, S, max_sub in jobs:
            f.write(struct.pack("3i", len(data), S, max_sub))
            f.write(data)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    d, p, out = open(fout, "rb").read(), 0, []
    for _ in jobs:
        st, w, h, n_sub, S, rounds, wrong, has = struct.unpack_from("8i", d, p)
        p += 32
        pix = None
        if has:
            pix = np.frombuffer(d, np.uint8, w * h, p).reshape(h, w)
            p += w * h
        out.append(dict(status=st, w=w, h=h, n_sub=n_sub, S=S, rounds=rounds, wrong=wrong, pixels=pix))
    assert p == len(d)
    return out
