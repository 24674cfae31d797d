"""What a decoder handle does with a batch of files on the host, without a GPU: csrc/jpeg_dec_pack.h (pack_room, pack_parse, pack_fill) as a g++ program of its
own under -fsanitize=address,undefined (tests/cpp/jpegdec_pack_pin.cpp).  The block is a heap buffer of exactly the handle's in_bytes; the program checks every
region the descriptors and jobs name (bounds, alignment, overlap), the bytes they point at (unstuff, survey, ChunkPlan::store, decode_sequential), every
descriptor against decode_planned_host under the same switches and the totals a launch is sized by -- an exit code each.  Inputs: the committed fixtures alone,
each under the eight combinations of OMNI_JPEGDEC_RESTART_WGS {0, 3} x OMNI_JPEGDEC_PLAIN_WGS {0, 3} x OMNI_JPEGDEC_UNSTUFF_DEV {0, 1}."""
import os
import struct
import subprocess

import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_restart_cases as R

OK, HOST, UNSUPPORTED, CORRUPT = J.OK, J.HOST, J.UNSUPPORTED, J.CORRUPT
MODE_DECODE, MODE_PIXELS, MODE_ZERO, MODE_SPREAD = 0, 1, 2, 3      # csrc/jpeg_dec_plan.h JD_MODE_*
ERR_INVALID = 1                                                    # include/omni_hip.h OMNI_ERR_INVALID
COMBOS = [(r, p, u) for r in (0, 3) for p in (0, 3) for u in (0, 1)]      # the program's order
S = 1024                                                           # OMNI_JPEGDEC_SUBSEQ_BITS' default
ROOMY = 1 << 16                                                    # a capacity above every small fixture


def build_pin(tmp) -> str:
    exe = os.path.join(str(tmp), "jpegdec_pack_pin_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                        os.path.join(J.PKG, "csrc"), os.path.join(J.ROOT, "tests", "cpp", "jpegdec_pack_pin.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_pin(exe: str, batches, tmp) -> list:
    """batches: [(w, h, capacity, [file bytes], host_idx, dev_idx)] -> per batch, per combination: dict(refusal, upload, clean_end, in_bytes, jobs,
    descs [dict(status, mode, n_sub, S, n_int, n_chunks, spread_chunks)])"""
    fin, fout = os.path.join(str(tmp), "kpin_in.bin"), os.path.join(str(tmp), "kpin_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("i", len(batches)))
        for w, h, capacity, files, host_idx, dev_idx in batches:
            f.write(struct.pack("7i", w, h, capacity, S, len(files), host_idx, dev_idx))
            for data in files:
                f.write(struct.pack("i", len(data)))
                f.write(data)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    d, p, out = open(fout, "rb").read(), 0, []
    keys = ("status", "mode", "n_sub", "S", "n_int", "n_chunks", "spread_chunks")
    for _, _, _, files, _, _ in batches:
        per = []
        for _ in COMBOS:
            refusal, upload, clean_end, in_bytes, jobs = struct.unpack_from("5i", d, p)
            p += 20
            descs = [dict(zip(keys, struct.unpack_from("7i", d, p + 28 * i))) for i in range(len(files))]
            p += 28 * len(files)
            per.append(dict(refusal=refusal, upload=upload, clean_end=clean_end, in_bytes=in_bytes, jobs=jobs, descs=descs))
        out.append(per)
    assert p == len(d)
    return out


def size_of(name: str):
    spec = J.SPECS.get(name) or R.SPECS[name]
    return spec[0], spec[1]


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    return build_pin(tmp_path_factory.mktemp("jpegdec_pack_pin"))


def test_every_fixture_alone(pin, tmp_path):
    names = [(J, n) for n in J.names()] + [(R, n) for n in R.names()]
    batches = []
    for mod, name in names:
        data = mod.file_of(name)
        w, h = size_of(name)
        batches.append((w, h, max(ROOMY, len(data)), [data], -1, -1))
    got = run_pin(pin, batches, tmp_path)
    for (mod, name), per in zip(names, got):
        for (rw, pw, dev), g in zip(COMBOS, per):
            what = (name, rw, pw, dev)
            if mod is J and J.SPECS[name][4] == UNSUPPORTED:
                assert g["refusal"] == ERR_INVALID, what
                continue
            D, = g["descs"]
            assert g["refusal"] == 0 and 0 < g["upload"] <= g["in_bytes"], what
            restart = mod is R or J.SPECS[name][4] == HOST
            if not restart:                                        # a file without a restart interval: the kernels', spread when the switch says so
                assert D["status"] == OK and D["mode"] == (MODE_SPREAD if pw and D["n_sub"] >= 2 else MODE_DECODE), what
                assert D["spread_chunks"] == (min(pw, D["n_sub"]) if D["mode"] == MODE_SPREAD else 0) and D["n_int"] == 0 == D["n_chunks"], what
            elif rw:                                               # every restart fixture can be planned over 3 workgroups
                assert D["status"] == OK and D["mode"] == MODE_DECODE and D["n_int"] >= 1 and 1 <= D["n_chunks"] <= rw and D["spread_chunks"] == 0, what
            else:
                assert D["status"] == HOST and D["mode"] == MODE_PIXELS, what
            assert g["jobs"] == (1 if dev and D["mode"] != MODE_PIXELS else 0), what
            assert (g["clean_end"] > g["upload"]) if g["jobs"] else g["clean_end"] in (0, g["upload"]), what


def mixed_batch():
    """96 x 64: OK files, restart files, files above the capacity (one of each kind), CORRUPT files (no frame header; too few restart markers; a cut scan)"""
    big, big_rst = J.file_of("noise_96x64_q100"), R.file_of("rows_noise_96x64_q100")
    capacity = min(len(big), len(big_rst)) - 1
    cut = J.mutations()[0][1]
    files = [J.file_of("gray_96x64_q75"), R.file_of("rows_gray_96x64_q75"), big, b"\xff\xd8\xff\xd9", R.file_of("blk1_gray_96x64_q75"), R.mutations()[1][1],
             J.file_of("opt_96x64_q75"), big_rst, cut, J.file_of("rst_96x64_q75"), J.file_of("gray_96x64_q5")]
    assert capacity >= 1024 and all(len(f) <= capacity for f in files if f not in (big, big_rst))
    return capacity, files


def test_a_mixed_batch_forwards_and_reversed(pin, tmp_path):
    capacity, files = mixed_batch()
    got = run_pin(pin, [(96, 64, capacity, files, 2, 0), (96, 64, capacity, files[::-1], len(files) - 3, len(files) - 1)], tmp_path)
    for (rw, pw, dev), fwd, rev in zip(COMBOS, *got):
        assert fwd["refusal"] == 0 == rev["refusal"]
        assert fwd["descs"] == rev["descs"][::-1], (rw, pw, dev)                               # a picture's plan does not depend on its place in the batch
        st = [D["status"] for D in fwd["descs"]]
        mode = [D["mode"] for D in fwd["descs"]]
        assert st[0] == OK and st[2] == HOST and mode[2] == MODE_PIXELS and st[7] == HOST and mode[7] == MODE_PIXELS      # above the capacity: pixels, both kinds
        assert st[3] == CORRUPT and mode[3] == MODE_ZERO
        assert st[8] == OK and mode[8] in (MODE_DECODE, MODE_SPREAD)                           # a cut scan is the kernels' to find
        for i in (1, 4, 9):
            assert (st[i], mode[i]) == ((OK, MODE_DECODE) if rw else (HOST, MODE_PIXELS)), (i, rw)
        assert (st[5], mode[5]) == (CORRUPT, MODE_ZERO)                                        # too few markers: the plan's verdict, or the sequential decoder's
        assert fwd["jobs"] == rev["jobs"] == (sum(m in (MODE_DECODE, MODE_SPREAD) for m in mode) if dev else 0)


def test_the_mutations_as_one_batch(pin, tmp_path):
    files = [data for _, data in J.mutations()]
    assert len(files) == 40
    got, = run_pin(pin, [(96, 64, ROOMY, files, -1, -1)], tmp_path)
    for (rw, pw, dev), g in zip(COMBOS, got):
        assert g["refusal"] == 0, (rw, pw, dev)
        assert all(D["status"] == OK and D["mode"] in (MODE_DECODE, MODE_SPREAD) for D in g["descs"])      # the header is whole: corruption is the kernels' to find
        assert g["jobs"] == (40 if dev else 0)


def test_a_capacity_of_exactly_the_largest_file_and_one_byte_less(pin, tmp_path):
    files = [J.file_of("gray_96x64_q75"), J.file_of("gray_96x64_q100"), J.file_of("opt_96x64_q75")]
    largest = max(range(3), key=lambda i: len(files[i]))
    n = len(files[largest])
    assert n >= 1024 and sum(len(f) == n for f in files) == 1
    exact, less = run_pin(pin, [(96, 64, n, files, -1, largest), (96, 64, n - 1, files, largest, -1)], tmp_path)      # (host_idx / dev_idx: the program's check 18)
    for g_exact, g_less in zip(exact, less):
        assert g_exact["refusal"] == 0 == g_less["refusal"]
        assert g_exact["descs"][largest]["status"] == OK and g_exact["descs"][largest]["mode"] != MODE_PIXELS
        assert (g_less["descs"][largest]["status"], g_less["descs"][largest]["mode"]) == (HOST, MODE_PIXELS)
        for i in range(3):
            if i != largest:
                assert g_exact["descs"][i] == g_less["descs"][i]
