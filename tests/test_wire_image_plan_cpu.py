"""CPU gate of the whole descriptor's byte layout (csrc/wire_plan.h whole_*, what wire_pack_image_kernel runs one dword per lane).

tests/cpp/wire_image_plan_pin.cpp, a stand-alone g++ program under -fsanitize=address,undefined with heap buffers of exactly the promised sizes: omni_wire_pack_image_host
plus the host's id patch == LoopNetWire's SWARM_LOOP_IMG_DES packets (host/loop_net_wire.hpp) byte for byte under send_img, send_whole_img_desc (with and without a file)
and is_pc_replay, on random frames and on the edges: every alignment of the byte tail against every residue of the file's size, no file (truncated), the smallest file,
exactly the capacity, above it (clamped), clamped key-point counts, an image without key points (no packet), NaN / inf / -0.0 payload bits; every packet decodes with
wire::decode and encodes back to itself; nothing is written behind a packet's last dword.

The library's own omni_wire_pack_image_host (the same header inside libomni_hip.so) is then compared, on every case the GPU test runs, with the packet an independent
writer puts together (tests/wire_image_cases.py: struct, big-endian), and read back by an independent reader."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import wire_image_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_image_plan") / "wire_image_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "wire_image_plan_pin.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_plan_plus_id_patch_equals_loop_net_wire_byte_for_byte(pin, seed):
    r = subprocess.run([pin, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert lines[-1] == ["OK", "60"] and not r.stderr
    case = {ln[1]: list(map(int, ln[2:])) for ln in lines if ln[0] == "CASE"}
    assert len(case) == 60
    H, smallest = 177 + 4 * 4096, 330
    for r_ in range(4):                                      # n_kps 0, 1, 2, 3, 4, 65, 200, 9999 -> 200: seven packets; all landmarks travel, with their flag bytes
        n = [1, 2, 3, 4, 65, 200, 200]
        files = sum(smallest + ((g + r_) & 3) for g in range(1, 8))
        assert case[f"tail{r_}:image"] == [8, 7, 7 * H + 29 * sum(n) + files]
        assert case[f"tail{r_}:whole+image"] == case[f"tail{r_}:replay"] == [8, 7, 7 * H + (29 + 256) * sum(n) + files]
        assert case[f"tail{r_}:whole"] == [8, 7, 7 * H + (29 + 256) * sum(n)] and case[f"tail{r_}:bare"] == [8, 7, 7 * H + 29 * sum(n)]
    assert case["clamped_counts:bare"] == [2, 1, H + 29 * 65]                                               # 9999 -> 65 key points, -3 -> none
    assert case["file_sizes:bare"][2] + 0 + 330 + 1024 + 1024 + 0 + 1 + 2 + 3 == case["file_sizes:image"][2]     # truncated: none; above the capacity: the capacity
    assert case["truncated_with_size:image"][2] == case["file_sizes:image"][2]


@pytest.fixture(scope="module")
def packed(omni):
    c = omni.capi
    return {name: (f, *c.wire_pack_image_host(*IC.args(f), **IC.kwargs(f), fill=0xA5)) for name, f in IC.cases(c).items()}


def test_library_host_function_equals_an_independent_writer(omni, packed):
    c = omni.capi
    for name, (f, out, sizes) in packed.items():
        N, M = f["flag"].shape
        cap = f["jpeg"].shape[1] if f["with_image"] else 0
        assert out.shape == (N, IC.capacity(M, cap)) == (N, c.wire_image_capacity(M, cap)) and sizes.shape == (N, 2)
        for g in range(N):
            want = IC.expected_packet(f, g)
            if want is None:
                assert sizes[g].tolist() == [0, 0] and np.all(out[g] == 0xA5), (name, g)
                continue
            off, size = sizes[g]
            end = (off + size + 3) // 4 * 4
            assert off == 3 == c.WIRE_IMAGE_OFFSET and size == len(want) and (off + 177) % 4 == 0, (name, g)
            assert out[g, off:off + size].tobytes() == want, (name, g)
            assert not out[g, :off].any() and not out[g, off + size:end].any() and np.all(out[g, end:] == 0xA5), (name, g)


def test_library_host_function_read_by_an_independent_parser(omni, packed):
    for name, (f, out, sizes) in packed.items():
        N, M = f["flag"].shape
        for g in range(N):
            n = int(np.clip(f["n_kps"][g], 0, M))
            if n == 0:
                continue
            p = IC.parse_image(out[g, sizes[g, 0]:sizes[g, 0] + sizes[g, 1]].tobytes())
            m = f["meta"][g]
            assert (p["drone_id"], p["msg_id"], p["frame_id"], p["landmark_num"], p["direction"], p["prevent"], p["width"], p["height"]) == \
                (m["drone_id"], 0, m["frame_id"], n, m["direction"], int(m["prevent_adding_db"] != 0), f["width"], f["height"]), (name, g)
            assert np.array_equal(p["image_desc_bits"], f["global_desc"][g].view(np.uint32)) and np.array_equal(p["flag"], f["flag"][g, :n])
            assert np.array_equal(p["desc_bits"], f["desc"][g, :n].view(np.uint32).reshape(-1) if f["with_features"] else np.zeros(0, np.uint32)), (name, g)
            for key, src in (("norm2d_bits", "norm2d"), ("kps_bits", "kps_xy"), ("l3d_bits", "l3d")):
                assert np.array_equal(p[key], f[src][g, :n].view(np.uint32).reshape(-1)), (name, g, key)
            assert p["image"] == f["jpeg"][g, :IC.image_size(f, g)].tobytes(), (name, g)


def test_host_refusals(omni):
    c = omni.capi
    f = IC.cases(c)["random_1x65_f1i1"]
    a = IC.args(f)
    with pytest.raises(c.OmniError, match="multiple of 4"):
        c.wire_pack_image_host(*a[:8], f["jpeg"][:, :1022], f["jpeg_sizes"], f["jpeg_status"])
    L = c.lib()
    ptr = [x.ctypes.data for x in a]
    out, sizes = np.zeros(c.wire_image_capacity(65, 1024), np.uint8), np.zeros(2, np.int32)
    call = lambda ni, mn, dd, gd, wi, jp, cap: L.omni_wire_pack_image_host(ni, mn, dd, gd, 1, wi, *ptr[:8], *jp, cap, 1, 1, out.ctypes.data, sizes.ctypes.data)
    for bad, word in (((0, 65, 64, 4096, 1, ptr[8:], 1024), b"n_images"), ((1, 1025, 64, 4096, 1, ptr[8:], 1024), b"max_num"), ((1, 65, 256, 4096, 1, ptr[8:], 1024), b"64"),
                      ((1, 65, 64, 1024, 1, ptr[8:], 1024), b"4096"), ((1, 65, 64, 4096, 0, ptr[8:], 1024), b"null exactly"), ((1, 65, 64, 4096, 1, [None] * 3, 1024), b"null exactly"),
                      ((1, 65, 64, 4096, 1, [ptr[8], None, ptr[10]], 1024), b"null exactly"), ((1, 65, 64, 4096, 1, ptr[8:], -4), b"jpeg_capacity"),
                      ((1, 65, 64, 4096, 1, ptr[8:], 2**30 + 4), b"jpeg_capacity")):
        assert call(*bad) == c.ERR_INVALID and word in L.omni_last_error(), (bad[:5], L.omni_last_error())
    assert call(1, 65, 64, 4096, 1, ptr[8:], 1024) == 0
    assert c.wire_image_capacity(0) == 0 and c.wire_image_capacity(1025) == 0 and c.wire_image_capacity(65, 6) == 0 and c.wire_image_capacity(65, -4) == 0


def test_the_layout_is_stated_once():
    """the kernel and the library's host entry only call wire_plan.h: neither restates the fingerprint, the head's size or an offset of it"""
    plan = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "wire_plan.h")).read())
    assert "0x4f4d4e49494d4731" in plan and "WP_IMAGE_HEAD_BYTES 177" in plan
    for f in ("wire_pack.hip", "wire_pack_host.cpp"):
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", f)).read())
        for word in ("0x4f4d4e49", "177", "180", "157", "165", "169", "173"):
            assert word not in text, (f, word)
        assert "whole_tail_dword" in text or f == "wire_pack_host.cpp"
