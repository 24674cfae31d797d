"""CPU gate of the LoopNet wire's byte layout (csrc/wire_plan.h, what csrc/wire_pack.hip runs one dword per lane).

tests/cpp/wire_plan_pin.cpp, a stand-alone g++ program under -fsanitize=address,undefined with heap buffers of exactly the promised size: omni_wire_pack_host plus
the host's id patch == the concatenated output of LoopNetWire::broadcast_fisheye_desc (host/loop_net_wire.hpp) byte for byte, on random frames and on the edges: an
image without key points (no packets), key points without a flag (a header with feature_num 0 alone), every landmark flagged, 63 / 64 / 65 flagged of 200,
send_all_features (feature_num still counts flags), NaN / inf / -0.0 payload bits; every packet decodes with wire::decode and encodes back to itself.

The library's own omni_wire_pack_host (the same header inside libomni_hip.so) is then read by an independent parser (tests/wire_cases.py: struct, big-endian)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import wire_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "omni-swarm_amd")


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wire_plan") / "wire_plan_pin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "wire_plan_pin.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plan_plus_id_patch_equals_loop_net_wire_byte_for_byte(pin, seed):
    r = subprocess.run([pin, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert lines[-1] == ["OK", "15"] and not r.stderr
    case = {ln[1]: ln[2:] for ln in lines if ln[0] == "CASE"}
    H, L = 16545, 324
    images, packets, nbytes, *features = map(int, case["no_keypoints"])
    assert images == 3 and len(features) == 2 and nbytes == 2 * H + (packets - 2) * L                      # the image without key points sent nothing
    images, packets, nbytes, *features = map(int, case["no_flag"])
    assert features[0] == 0 and packets == 2 + features[1]                                                  # a header alone
    assert list(map(int, case["all_flagged"]))[-1] == 200
    for c in (63, 64, 65):
        assert list(map(int, case[f"flagged{c}"])) == [1, 1 + c, H + c * L, c]
    images, packets, nbytes, *features = map(int, case["send_all"])
    assert features[0] == 40 and packets >= 2 + 150 and packets > 2 + sum(features)                        # 150 packets behind a header that announces 40
    assert list(map(int, case["payload_bits"])) == [1, 66, H + 65 * L, 65]
    assert list(map(int, case["clamped_counts"]))[:2] == [2, 1 + int(case["clamped_counts"][3])]          # 9999 -> 65 key points, -3 -> none


@pytest.fixture(scope="module")
def packed(omni):
    c = omni.capi
    return {name: (f, *c.wire_pack_host(*WC.args(f), send_all_features=f["send_all_features"], fill=0xA5)) for name, f in WC.cases(c).items()}


def test_library_host_function_read_by_an_independent_parser(omni, packed):
    c = omni.capi
    for name, (f, out, table) in packed.items():
        N, M = f["flag"].shape
        assert out.shape == (N, 3 + 16545 + 324 * M) == (N, c.wire_packet_capacity(M)) and table.shape == (N, 2 + 2 * (1 + M)) == (N, c.wire_table_ints(M))
        for g in range(N):
            n = int(np.clip(f["n_kps"][g], 0, M))
            fl = f["flag"][g, :n] > 0
            sent = np.arange(n) if f["send_all_features"] else np.flatnonzero(fl)
            pk = c.wire_packets(out[g], table[g])
            assert len(pk) == (0 if n == 0 else 1 + len(sent)), (name, g)
            assert table[g, 1] == (0 if n == 0 else 16548 + 324 * len(sent)) and np.all(out[g, table[g, 1]:] == 0xA5) and not table[g, 2 + 2 * len(pk):].any()
            if n == 0:
                continue
            m = f["meta"][g]
            assert pk[0][0] == "VIOKF_HEADER" and all(ch == "VIOKF_LANDMARKS" for ch, _ in pk[1:])
            assert (table[g, 2] + 161) % 4 == 0 and all((table[g, 2 + 2 * k] + 68) % 4 == 0 for k in range(1, len(pk)))
            h = WC.parse_header(pk[0][1])
            assert (h["drone_id"], h["msg_id"], h["frame_id"], h["feature_num"], h["direction"], h["prevent"]) == \
                (m["drone_id"], 0, m["frame_id"], int(fl.sum()), m["direction"], int(m["prevent_adding_db"] != 0)), (name, g)
            be64 = lambda b: np.frombuffer(b, ">u8")
            assert be64(h["timestamp_bits"])[0] == np.float64(m["timestamp"]).view(np.uint64)
            assert np.array_equal(be64(h["pose_bits"]), m["pose_drone"].view(np.uint64)) and np.array_equal(be64(h["extrinsic_bits"]), m["camera_extrinsic"].view(np.uint64))
            assert np.array_equal(h["image_desc_bits"], f["global_desc"][g].view(np.uint32))
            for (_, b), i in zip(pk[1:], sent):
                l = WC.parse_landmark(b)
                assert (l["msg_id"], l["header_id"], l["drone_id"], l["landmark_id"], l["flag"]) == (0, 0, m["drone_id"], i, f["flag"][g, i]), (name, g, i)
                want = np.concatenate([f["norm2d"][g, i], f["kps_xy"][g, i], f["l3d"][g, i]]).view(np.uint32)
                assert np.array_equal(l["floats_bits"], want) and np.array_equal(l["desc_bits"], f["desc"][g, i].view(np.uint32)), (name, g, i)


def test_the_layout_is_stated_once():
    """wire_plan.h is plain C++ for both compilers (no HIP header, no containers); the kernel and the library's host entry only call it"""
    plan = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", "wire_plan.h")).read())
    for word in ("hip/", "common.h", "std::vector", "<vector>", "<algorithm>"):
        assert word not in plan, word
    assert "0x4f4d4e4948445231" in plan and "0x4f4d4e494c4d4b31" in plan
    for f in ("wire_pack.hip", "wire_pack_host.cpp"):
        text = re.sub(r"//.*", "", open(os.path.join(PKG, "csrc", f)).read())
        for word in ("0x4f4d4e49", "16545", "16548", "161", "324"):                  # the fingerprints, the sizes and the placement
            assert word not in text, (f, word)
