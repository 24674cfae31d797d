"""LoopNet's other two message kinds on the wire (omni-swarm_amd/host/loop_net_wire.hpp; swarm_loop/src/loop_net.cpp:9-10, 37-41, 103-140, 174-184): the loop edge
(SWARM_LOOP_CONN) and the whole image descriptor (SWARM_LOOP_IMG_DES).  CPU only: g++ builds tests/cpp/wire_messages_check.cpp, which prints one tagged line per
check; the two packets it dumps are read by the independent struct reader of tests/wire_image_cases.py."""
import os
import subprocess

import numpy as np
import pytest

from tests import wire_image_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 8 + 8 + 4 + 8 + 8 + 4 + 4 + 1 + 2 * 56 + 4 + 4096 * 4         # the header packet
L = 8 + 8 + 8 + 4 + 4 + 4 + 7 * 4 + 4 + 64 * 4                     # a landmark packet
N_LM = (40, 25, 0, 60)                                              # the key frame's landmarks per direction; flag = i % 3
FLAGGED = sum(sum(1 for i in range(n) if i % 3) for n in N_LM)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wire_messages") / "wire_messages_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "cpp", "wire_messages_check.cpp")])
    return out


@pytest.fixture(scope="module", params=[1, 2, 3])
def lines(exe, request):
    r = subprocess.run([exe, str(request.param)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = {}
    for ln in r.stdout.strip().split("\n"):
        out.setdefault(ln.split()[0], []).append(ln.split()[1:])
    return out


def test_round_trips(lines):
    assert lines["EDGE_ROUNDTRIP"] == [["20", "0"]]                 # decode(encode(x)) == x by bits; no other size decodes (every truncation, one byte more)
    assert lines["IMAGE_ROUNDTRIP"] == [["48", "48"]]               # 1 / 2 / 3 / 4 / 40 / 200 landmarks x files of 0 / 1 / 331 / 4096 bytes x with and without descriptors


def test_edge_read_by_an_independent_parser(lines):
    e = IC.parse_edge(bytes.fromhex(lines["EDGE_HEX"][0][0]))
    want = lines["EDGE_FIELDS"][0]
    assert [e["id"], e["keyframe_id_a"], e["keyframe_id_b"], e["drone_id_a"], e["drone_id_b"], e["pnp_inlier_num"]] == list(map(int, want[:6]))
    assert [int(v) for v in e["bits"]] == [int(v, 16) for v in want[6:]] and len(want) == 6 + 29
    assert int(e["bits"][0]) == 0x7ff8000000abcdef and int(e["bits"][8]) == 0x8000000000000000                # ts_a's NaN payload, -0.0 in the relative attitude


def test_whole_descriptor_read_by_an_independent_parser(lines):
    for tag, feat in (("IMAGE_HEX_FEATURES", True), ("IMAGE_HEX_BARE", False)):
        b = bytes.fromhex(lines[tag][0][0])
        p = IC.parse_image(b)
        assert len(b) == 177 + 4 * (4096 + (320 if feat else 0) + 35) + 5 + 7
        assert (p["drone_id"], p["msg_id"], p["frame_id"], p["landmark_num"], p["direction"], p["prevent"], p["width"], p["height"]) == (2, 987654321012, 4242, 5, 3, 0, 643, 480)
        assert p["timestamp_bits"] == bytes.fromhex("7ff8000000abcdef") and len(p["image"]) == 7 and 0 not in p["image"]
        assert np.array_equal(p["kps_bits"].astype(np.uint32).view(np.float32).reshape(5, 2), [[10 * i + 3, 3 * i] for i in range(5)])
        assert p["flag"].tolist() == [0, 1, 2, 0, 1] and len(p["desc_bits"]) == (320 if feat else 0)
        assert p["image_desc_bits"][7] == 0xff800000 and p["l3d_bits"][2] == 0x80000000 and p["norm2d_bits"][0] == 1 and (not feat or p["desc_bits"][3] == 0x7fc12345)
        assert np.frombuffer(p["pose_bits"], ">f8").tolist() == [1.5, 0, 0, 0.8, 0, 0, 0.6]


def test_what_a_drone_sends_in_each_mode(lines):
    whole = lambda n, feat, img: 177 + 4 * (4096 + (64 * n if feat else 0) + 7 * n) + n + img
    assert lines["SENT_OFF"] == [[str(3 + FLAGGED), "0"]]                                                   # the switches off: header + landmark packets alone
    # send_img: the third packet behind each image's landmark packets, without descriptors; the packets in front of it are the ones sent with the switches off
    assert lines["SENT_IMAGE"] == [[str(3 + FLAGGED + 3), "3", "1", "0", "1", "1"]]
    assert lines["SENT_WHOLE"] == [[str(3 + FLAGGED + 3), "3", "1", "3", "1", "1"]]                         # send_whole_img_desc: with them
    assert lines["SENT_REPLAY"] == [["3", "3", "1"]]                                                        # is_pc_replay: one packet per image, whole, nothing else
    assert whole(5, True, 7) - whole(5, False, 7) == 4 * 320


def test_truncated_packets_are_dropped(lines):
    assert lines["TRUNCATED"] == [["0", "1", "1"]]                  # every prefix, one byte more, the wrong channel: dropped; the packets themselves: taken


def test_inconsistent_length_members_are_dropped(lines):
    r = lines["INCONSISTENT"][0]
    bar = r.index("|")
    assert r[3] == "(1)" and r[5] == "(1)"                          # the allowed neighbours: no global descriptor at all, a file of exactly the cap
    dropped = [v for k, v in enumerate(r[:bar]) if k not in (3, 5)]
    # feature size 64 n - 1 and 64 (n = 10), image_desc of 100, a file above the cap, direction 4 and -1, more landmarks than MAX_FEATURES; then each of the four
    # length members set to 2^31 - 1, 2^30, -1 and the packet's own size
    assert len(dropped) == 7 + 16 and set(dropped) == {"0"}
    assert r[bar + 1:] == ["1", "3"]                                # the packet they were made from is taken; image_callback saw the three valid ones only


def test_own_packets_and_edges_are_ignored(lines):
    assert lines["OWN"] == [["0", "0", "0", "|", "2", "2", "1", "1"]]      # the sender: no image, no edge, no frame; another drone: both edges, field for field


def test_accept_img_desc_rule(lines):
    rows = {(int(r[0]), int(r[1])): list(map(int, r[2:])) for r in lines["ACCEPT"]}
    for key, (images, bad, frames, landmarks, content) in rows.items():
        assert images == 3 and bad == 0 and content == 1            # image_callback always gets the image, with its file, as it was sent
        # the frame flow: only with the switch AND descriptors in the packet; then ALL landmarks arrive, not only the flagged ones
        assert (frames, landmarks) == ((3, sum(N_LM)) if key == (1, 1) else (0, 0)), key
    assert len(rows) == 4
    # header + landmark + whole packets of one drone, the switch on: every image enters the frame flow once
    assert lines["ACCEPT_ALL"] == [["3", "3", str(FLAGGED), str(FLAGGED), str(sum(N_LM))]]
