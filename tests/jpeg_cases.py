"""The cases of the JPEG stage (csrc/jpeg_plan.h, csrc/jpeg.hip), shared by the CPU and the GPU tier: the images, Pillow's files for them from the committed
fixture tests/golden/jpeg_cases.npz (written by tools/gen_jpeg_golden.py; the GPU tier never imports Pillow), the g++ pin program around the header, and a small
reader of a baseline scan's Huffman symbols (to ASSERT that the fixtures hold a stuffed FF 00 pair and a ZRL symbol, not assume it)."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
HEADER_BYTES = 328
OK, TRUNCATED = 0, 1

SHAPES = [(8, 8), (16, 8), (24, 16), (13, 11), (64, 48)]        # (w, h): one block; DC prediction across two; two block rows; edge replication both ways
CONTENTS = ["noise", "smooth", "zeros", "white", "pattern"]
QUALITIES = [10, 50, 75, 100]
BATCH = 5                                                      # 5 different 64 x 48 images in one call: no state leaks between images
STRIDE_CASE = ((24, 16), 40)                                   # 24 x 16 with 40 bytes between rows


def make_image(content: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    y, x = np.mgrid[0:h, 0:w]
    if content == "noise":                                     # long codes, ZRL
        a = np.random.default_rng(1000 + 97 * w + h + seed).integers(0, 256, (h, w))
    elif content == "smooth":                                  # EOB, long zero runs
        a = 128 + 100 * np.sin((x + 3 * seed) / 9.0) * np.cos((y + seed) / 7.0)
    elif content == "zeros":
        a = np.zeros((h, w))
    elif content == "white":
        a = np.full((h, w), 255)
    else:                                                      # black / white
        a = 255 * (((x // 3) + (y // 5) + seed) % 2)
    return np.ascontiguousarray(a, dtype=np.float64).astype(np.uint8)


def image_sets() -> dict:
    """name -> [k][h][w] u8: what the fixture stores next to Pillow's files"""
    out = {f"{c}_{w}x{h}": make_image(c, w, h)[None] for (w, h) in SHAPES for c in CONTENTS}
    out["batch_64x48"] = np.stack([make_image(CONTENTS[i % len(CONTENTS)], 64, 48, seed=i + 1) for i in range(BATCH)])
    return out


_fix = None


def fixture():
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as z:
            _fix = {k: z[k] for k in z.files}
    return _fix


def cases():
    """[(id, images [k][h][w], quality, [Pillow's file per image])] from the fixture: every shape x content x quality, and the batch at every quality"""
    f = fixture()
    out = []
    for name in sorted(k[4:] for k in f if k.startswith("img_")):
        imgs = f["img_" + name]
        for q in QUALITIES:
            out.append((f"{name}_q{q}", imgs, q, [f[f"jpg_{name}_q{q}_{i}"].tobytes() for i in range(imgs.shape[0])]))
    return out


def build_pin(tmp) -> str:
    exe = os.path.join(str(tmp), "jpeg_plan_pin")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "jpeg_plan_pin.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe: str, jobs, tmp) -> list:
    """jobs: [(gray [h][stride] u8, width, quality, zero_from_row, capacity)] -> [(status, size, buffer of capacity + 16 bytes, 0xA5 where nothing was written)]"""
    fin, fout = os.path.join(str(tmp), "pin_in.bin"), os.path.join(str(tmp), "pin_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for g, w, q, zfr, cap in jobs:
            g = np.ascontiguousarray(g, np.uint8)
            f.write(struct.pack("6i", w, g.shape[0], g.shape[1], q, zfr, cap))
            f.write(g.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    d, p, out = open(fout, "rb").read(), 0, []
    for g, w, q, zfr, cap in jobs:
        st, sz = struct.unpack_from("2i", d, p)
        out.append((st, sz, np.frombuffer(d, np.uint8, cap + 16, p + 8)))
        p += 8 + cap + 16
    assert p == len(d)
    return out


def roomy(w: int, h: int) -> int:
    """a capacity no file of this size exceeds: 63 x 26 + 20 bits per block, every byte stuffed"""
    return HEADER_BYTES + 2 + ((w + 7) // 8) * ((h + 7) // 8) * 416 + 8


def pin_file(exe, tmp, gray, quality, zero_from_row=None, width=0) -> bytes:
    g = np.ascontiguousarray(gray, np.uint8)
    w = width or g.shape[1]
    (st, sz, buf), = run_pin(exe, [(g, w, quality, g.shape[0] if zero_from_row is None else zero_from_row, roomy(w, g.shape[0]))], tmp)
    assert st == OK
    return buf[:sz].tobytes()


# ---- reading a scan back: the Huffman symbols of a baseline one-component file with the standard tables -----------------------------------------------------
def _huff_tables(data: bytes):
    tabs, p = {}, 2
    while data[p:p + 2] != b"\xff\xda":
        marker, ln = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        if marker == 0xC4:
            cls_id, bits, vals = data[p + 4], data[p + 5:p + 21], data[p + 21:p + 2 + ln]
            code, k, t = 0, 0, {}
            for ln_ in range(1, 17):
                for _ in range(bits[ln_ - 1]):
                    t[(ln_, code)] = vals[k]
                    code, k = code + 1, k + 1
                code <<= 1
            tabs[cls_id] = t
        p += 2 + ln
    return tabs, p + 2 + int.from_bytes(data[p + 2:p + 4], "big")


def scan_symbols(data: bytes, w: int, h: int):
    """-> (AC symbols of every block in order, number of stuffed FF 00 pairs in the scan); asserts that the scan holds exactly the picture's blocks"""
    tabs, start = _huff_tables(data)
    assert data[-2:] == b"\xff\xd9"
    scan = data[start:-2]
    stuffed = scan.count(b"\xff\x00")
    assert scan.count(b"\xff") == stuffed                       # no other marker inside the scan
    bits = "".join(f"{b:08b}" for b in scan.replace(b"\xff\x00", b"\xff"))
    pos, syms = 0, []

    def symbol(t):
        nonlocal pos
        code = 0
        for ln in range(1, 17):
            code = code << 1 | int(bits[pos + ln - 1])
            if (ln, code) in t:
                pos += ln
                return t[(ln, code)]
        raise AssertionError("no such code")
    for _ in range(((w + 7) // 8) * ((h + 7) // 8)):
        n = symbol(tabs[0x00])                                  # (the DC difference's category = its value bits)
        pos += n
        k = 1
        while k < 64:
            s = symbol(tabs[0x10])
            syms.append(s)
            if s == 0x00:
                break
            k += (s >> 4) + 1
            pos += s & 15
        assert k <= 64
    assert len(bits) - pos < 8 and set(bits[pos:]) <= {"1"}     # the 1-padding of the last byte
    return syms, stuffed
