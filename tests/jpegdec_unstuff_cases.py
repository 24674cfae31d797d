"""The cases of the JPEG decoder's unstuffing by tiles (OMNI_JPEGDEC_UNSTUFF_DEV; csrc/jpeg_dec_plan.h unstuff_keep / survey / unstuff_tiled_host, csrc/jpeg_dec.hip
jpegdec_unstuff_kernel), shared by the CPU and the GPU tier: seeded byte strings, patterns laid across a tile seam and a 16-byte lane seam, the scans of the
committed fixtures and of the mutations, files with fill bytes in front of their restart markers; the byte-wise rules written out in Python; the g++ pin
program around the header (tests/cpp/jpegdec_unstuff_pin.cpp)."""
import os
import struct
import subprocess

import numpy as np

from tests import jpegdec_cases as J
from tests import jpegdec_restart_cases as R

ROOT, PKG = J.ROOT, J.PKG
U_ENV, W_ENV, S_ENV, R_ENV = "OMNI_JPEGDEC_UNSTUFF_DEV", "OMNI_JPEGDEC_PLAIN_WGS", "OMNI_JPEGDEC_SUBSEQ_BITS", "OMNI_JPEGDEC_RESTART_WGS"
PAD = 16                                                       # csrc/jpeg_dec_plan.h JD_SCAN_PAD
LANE = 16                                                      # raw bytes per lane of jpegdec_unstuff_kernel
FILL = "rows_gray_96x64_q75"                                   # the restart file that gets fill bytes


def lengths(T: int):
    return [0, 1, 2, 15, 16, 17, T - 1, T, T + 1, 3 * T + 5]


def seeded(n: int, seed: int) -> bytes:
    """every byte drawn from {0xFF (about 1/4), 0x00, 0xD0..0xD7, 0xD9, any other}"""
    rng = np.random.default_rng(seed)
    kind = rng.choice(5, n, p=[0.25, 0.2, 0.15, 0.05, 0.35])
    other = rng.integers(1, 0xD0, n)
    vals = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0xFF, 0x00, 0xD0 + rng.integers(0, 8, n), 0xD9], other)
    return vals.astype(np.uint8).tobytes()


def seam_patterns(T: int):
    """[(what, bytes)]: FF|00, FF FF|00, FF|FF 00, FF|D3, FF|D9 and a lone FF as the last byte, `|` at a tile seam and at a lane seam inside a tile"""
    out = []
    for seam in (T, LANE, T + 3 * LANE, 2 * T):
        filler = bytes(0x20 + i % 0x50 for i in range(seam + 40))
        for name, left, right in (("FF|00", b"\xff", b"\x00"), ("FF FF|00", b"\xff\xff", b"\x00"), ("FF|FF 00", b"\xff", b"\xff\x00"), ("FF|D3", b"\xff", b"\xd3"),
                                  ("FF|D9", b"\xff", b"\xd9")):
            s = filler[:seam - len(left)] + left + right + filler[seam + len(right):]
            assert len(s) == len(filler) and s[seam - 1] == 0xFF
            out.append((f"{name} at {seam}", s))
        out.append((f"a lone FF ends the string at {seam}", filler[:seam - 1] + b"\xff"))
        out.append((f"a lone FF ends the string behind {seam}", filler[:seam] + b"\xff"))
    return out


def strings(T: int):
    """[(what, bytes)]: all of them below 20 KB"""
    out = [(f"seeded, {n} bytes", seeded(n, 1000 + k)) for k, n in enumerate(lengths(T))]
    out += [(f"seeded without an end, {n} bytes", seeded(n, 2000 + k).replace(b"\xd9", b"\x00")) for k, n in enumerate(lengths(T)[6:])]
    return out + seam_patterns(T)


# ---- the byte-wise rules, written out -----------------------------------------------------------------------------------------------------------------------
def is_rst(b: int) -> bool:
    return 0xD0 <= b <= 0xD7


def raw_end_rule(s: bytes) -> int:
    """where the byte-wise pass stops: the start of the 0xFF run that ends in a marker other than RSTn or 00, or runs off the end; len(s) without one"""
    i, n = 0, len(s)
    while i < n:
        if s[i] != 0xFF:
            i += 1
            continue
        j = i
        while i < n and s[i] == 0xFF:
            i += 1
        if i >= n or not (s[i] == 0 or is_rst(s[i])):
            return j
        i += 1
    return n


def scan_end_rule(s: bytes, p: int = 0) -> int:
    """the first marker at or behind p that is neither a stuffed 0xFF00 nor a restart marker; len(s) without one (a run of 0xFF to the end included)"""
    n = len(s)
    while p < n:
        if s[p] != 0xFF:
            p += 1
            continue
        q = p
        while q < n and s[q] == 0xFF:
            q += 1
        if q >= n:
            return n
        if not (s[q] == 0 or is_rst(s[q])):
            return p
        p = q + 1
    return n


def keep_rule(s: bytes, raw_end: int) -> np.ndarray:
    """bool [raw_end]: the neighbourhood rule of the issue -- a byte other than 0xFF is kept unless an 0xFF stands in front of it; an 0xFF is kept when a 00
    follows; a neighbour outside [0, raw_end) is neither"""
    a = np.frombuffer(s, np.uint8)[:raw_end].astype(np.int32)
    prev = np.concatenate([[1], a[:-1]]) if raw_end else a
    nxt = np.concatenate([a[1:], [1]]) if raw_end else a
    return np.where(a != 0xFF, prev != 0xFF, nxt == 0)


def check_tiled(c, s: bytes, what=""):
    """the tiled stand-in against the byte-wise pass and the rules above -> (the byte-wise pass's result, the tiled one's)"""
    T = c.jpeg_unstuff_tile_bytes()
    clean, n, rst = c.jpeg_unstuff_host(s)
    t = c.jpeg_unstuff_tiled_host(s)
    assert t["n_clean"] == n == t["surveyed_clean"] and np.array_equal(t["out"], clean) and not clean[n:].any() and len(clean) == n + PAD, (what, n, t["n_clean"])
    assert t["rst"] == rst, what
    re = raw_end_rule(s)
    assert t["raw_end"] == re, (what, t["raw_end"], re)
    keep = keep_rule(s, re)
    assert np.array_equal(np.frombuffer(s, np.uint8)[:re][keep], clean[:n]), what            # the rule alone gives the byte-wise pass's bytes
    before = np.concatenate([[0], np.cumsum(keep)])
    off = t["tile_off"]
    assert len(off) == (max(re, 1) + T - 1) // T and off[0] == 0 and all(x <= y for x, y in zip(off, off[1:])), (what, off)
    assert off == [int(before[k * T]) for k in range(len(off))] and 0 <= n - off[-1] <= T, (what, off)
    return (clean, n, rst), t


def fixture_scans():
    """[(name, the bytes from the first scan's start to the EOI)] of both committed fixtures -- a file with several scans: the other scans' headers included"""
    out = []
    for mod in (J, R):
        for name in mod.names():
            data = mod.file_of(name)
            lo, hi = J.scan_range(data)
            out.append((name, data[lo:hi]))
    return out


def mutation_scans():
    lo, _ = J.scan_range(J.file_of(J.MUTATED))
    return [(what, data[lo:]) for what, data in J.mutations()]


def fill_file(extra: int) -> bytes:
    """FILL with `extra` more 0xFF in front of every restart marker"""
    data = R.file_of(FILL)
    m = R.markers(data)
    assert len(m) == 7
    out, at = bytearray(), 0
    for p in m:
        out += data[at:p] + b"\xff" * extra
        at = p
    return bytes(out + data[at:])


# ---- the pin program -------------------------------------------------------------------------------------------------------------------------------------
def build_pin(tmp, sanitize: bool = True) -> str:
    exe = os.path.join(str(tmp), "jpegdec_unstuff_pin" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "jpegdec_unstuff_pin.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe: str, jobs, tmp) -> list:
    """jobs: [bytes] -> [dict(n_clean, raw_end, n_rst, n_tiles, scan_end)]; the program compares the tiles with the byte-wise pass itself"""
    fin, fout = os.path.join(str(tmp), "upin_in.bin"), os.path.join(str(tmp), "upin_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for data in jobs:
            f.write(struct.pack("i", len(data)))
            f.write(data)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    d = open(fout, "rb").read()
    assert len(d) == 40 * len(jobs)
    return [dict(zip(("n_clean", "raw_end", "n_rst", "n_tiles", "scan_end"), struct.unpack_from("5q", d, 40 * k))) for k in range(len(jobs))]
