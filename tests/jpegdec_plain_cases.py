"""The cases of the JPEG decoder's path that spreads a file WITHOUT a restart interval over several workgroups (OMNI_JPEGDEC_PLAIN_WGS; csrc/jpeg_dec_plan.h
plain_chunks / decode_planned_host, csrc/jpeg_dec.hip chunk, seam and write kernels), shared by the CPU and the GPU tier.  The files and Pillow's
pixels are the committed fixture of tests/jpegdec_cases.py; the one picture made here is written by the library's own host encoder.  The g++ pin program around
the header is tests/cpp/jpegdec_plain_pin.cpp."""
import os
import struct
import subprocess

import numpy as np

from tests import jpegdec_cases as J

ROOT, PKG = J.ROOT, J.PKG
OK, HOST, UNSUPPORTED, CORRUPT = J.OK, J.HOST, J.UNSUPPORTED, J.CORRUPT
W_ENV, S_ENV, R_ENV = "OMNI_JPEGDEC_PLAIN_WGS", "OMNI_JPEGDEC_SUBSEQ_BITS", "OMNI_JPEGDEC_RESTART_WGS"
MAX_SUBSEQ = 4096                                              # csrc/jpeg_dec_plan.h JD_MAX_SUBSEQ
WGS = (2, 3, 8)
STAT_KEYS = ("n_sub", "subseq_bits", "rounds", "chunks", "seam_rounds", "seam_changed")      # what a handle reports, in the stand-in's names

# more subsequences than one workgroup holds: noise at quality 100, S = 128
BIG_W, BIG_H, BIG_Q = 256, 256, 100


def big_noise_file(capi) -> bytes:
    img = np.random.default_rng(77).integers(0, 256, (BIG_H, BIG_W)).astype(np.uint8)
    st, data = capi.jpeg_encode_host(img, BIG_Q)
    assert st == 0
    return data


def differing(a, b) -> int:
    return int((np.asarray(a) != np.asarray(b)).sum()) if np.asarray(a).shape == np.asarray(b).shape else -1


# ---- the pin program -------------------------------------------------------------------------------------------------------------------------------------
def build_pin(tmp, sanitize: bool = True) -> str:
    exe = os.path.join(str(tmp), "jpegdec_plain_pin" + ("_san" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "jpegdec_plain_pin.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe: str, jobs, tmp) -> list:
    """jobs: [(file bytes, S, W, max_sub)] -> [dict(status, w, h, n_sub, S, chunks, chunk_rounds, seam_rounds, seam_changed, seam_chunks, pixels [h][w] or None)]"""
    fin, fout = os.path.join(str(tmp), "ppin_in.bin"), os.path.join(str(tmp), "ppin_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(jobs)))
        for data, S, W, max_sub in jobs:
            f.write(struct.pack("4i", len(data), S, W, max_sub))
            f.write(data)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    d, p, out = open(fout, "rb").read(), 0, []
    for _ in jobs:
        st, w, h, n_sub, S, chunks, chunk_rounds, seam_rounds, seam_changed, seam_chunks, has = struct.unpack_from("11i", d, p)
        p += 44
        pix = None
        if has:
            pix = np.frombuffer(d, np.uint8, w * h, p).reshape(h, w)
            p += w * h
        out.append(dict(status=st, w=w, h=h, n_sub=n_sub, S=S, chunks=chunks, chunk_rounds=chunk_rounds, seam_rounds=seam_rounds, seam_changed=seam_changed,
                        seam_chunks=seam_chunks, pixels=pix))
    assert p == len(d)
    return out
