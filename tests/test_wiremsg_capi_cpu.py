"""What the wire's other two message kinds add to the C boundaries, without a GPU: include/omni_host_wire_messages.h is valid C99, libomni_host_wiremsg.so exports
exactly what it declares and pipeline.WIREMSG_SYMBOLS binds exactly that; a null pipeline and a null argument are a code and a message; the new entries of
include/omni_hip.h are declared, exported, listed in capi.SYMBOLS and refuse null handles; the Makefile builds the library; SwarmLoopParams::to_wire hands the three
launch parameters on to LoopNetWire, which then sends what loop_net.cpp:37-41, 103-116 send."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")
NEW = {"omni_wire_image_capacity", "omni_wire_pack_image_enqueue_dev", "omni_wire_pack_image_host", "omni_cam_set_wire_image", "omni_cam_wire_image"}
HOST = {"omni_wiremsg_last_error", "omni_pipeline_set_wire_messages", "omni_pipeline_get_wire_messages", "omni_pipeline_set_wire_accept_img_desc",
        "omni_pipeline_get_remote_edges", "omni_pipeline_remote_image_pending", "omni_pipeline_take_remote_image"}

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "omni_host_wire_messages.h"
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)
int main(void) {
    int a = 7, b = 7, c = 7, n = 7;
    int64_t nb = 7, dropped = 7;
    omni_remote_edge e[1];
    unsigned char buf[8];
    CHECK(sizeof(omni_remote_edge) == 272);
    CHECK(OMNI_WIRE_CHANNEL_IMG_DES == 2 && OMNI_WIRE_CHANNEL_LOOP_CONN == 3 && OMNI_WIRE_IMG_OFF == 0 && OMNI_WIRE_IMG_IMAGE == 1 && OMNI_WIRE_IMG_WHOLE == 2 &&
          OMNI_WIRE_IMG_PC_REPLAY == 3 && OMNI_WIRE_REMOTE_IMAGES_MAX == 64);
    CHECK(omni_pipeline_set_wire_messages(NULL, OMNI_WIRE_IMG_WHOLE, 1) == 1 && strstr(omni_wiremsg_last_error(), "omni_pipeline_set_wire_messages: null pipeline"));
    CHECK(omni_pipeline_get_wire_messages(NULL, &a, &b, &c) == 1 && a == 7 && b == 7 && c == 7 && strstr(omni_wiremsg_last_error(), "omni_pipeline_get_wire_messages"));
    CHECK(omni_pipeline_set_wire_accept_img_desc(NULL, 1) == 1 && strstr(omni_wiremsg_last_error(), "omni_pipeline_set_wire_accept_img_desc: null pipeline"));
    CHECK(omni_pipeline_get_remote_edges(NULL, e, 1, &n) == 1 && n == 7 && strstr(omni_wiremsg_last_error(), "omni_pipeline_get_remote_edges: null pipeline"));
    CHECK(omni_pipeline_remote_image_pending(NULL, &dropped) == -1 && dropped == 7);
    CHECK(omni_pipeline_take_remote_image(NULL, buf, 8, &nb, &a, &nb, &b, &c, &n) == 1 && nb == 7 && strstr(omni_wiremsg_last_error(), "omni_pipeline_take_remote_image: null pipeline"));
    printf("OK\n");
    return 0;
}
"""

TO_WIRE = r"""
#include <cstdio>
#include "../../omni-swarm_amd/host/swarm_loop_params.hpp"
#include "../../omni-swarm_amd/host/loop_net_wire.hpp"
using namespace omni;
int main() {
    for (int k = 0; k < 8; ++k) {
        SwarmLoopParams p;
        p.send_img = k & 1; p.send_whole_img_desc = (k & 2) != 0; p.is_pc_replay = (k & 4) != 0;
        LoopNetWire w(2);
        p.to_wire(w);
        int headers = 0, landmarks = 0, whole = 0, with_features = 0;
        w.publish = [&](const char* ch, const std::vector<uint8_t>& b) {
            headers += std::strcmp(ch, wire::CH_HEADER) == 0; landmarks += std::strcmp(ch, wire::CH_LANDMARKS) == 0;
            if (std::strcmp(ch, wire::CH_IMG_DES) == 0) { ImageDescriptor d; if (!wire::decode(b.data(), b.size(), d)) std::printf("UNDECODABLE\n"); ++whole; with_features += !d.feature_descriptor.empty(); }
        };
        ImageDescriptor im;
        im.drone_id = 2; im.landmark_num = 3; im.image_desc.assign(4096, 0.5f); im.feature_descriptor.assign(3 * 64, 0.25f);
        im.landmarks_2d.assign(3, Point2f{1, 2}); im.landmarks_2d_norm.assign(3, Point2f{0, 0}); im.landmarks_3d.assign(3, Point3f{}); im.landmarks_flag = {1, 0, 1};
        w.broadcast_img_desc(im);
        std::printf("MODE %d %d %d | %d %d %d %d\n", (int)w.send_img, (int)w.send_whole_img_desc, (int)w.is_pc_replay, headers, landmarks, whole, with_features);
    }
    return 0;
}
"""


def test_c_program_links_the_library_and_meets_every_null_refusal(tmp_path):
    src, exe = tmp_path / "wiremsg_capi.c", tmp_path / "wiremsg_capi"
    src.write_text(PROGRAM)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", LIBDIR,
                        "-lomni_host_wiremsg", "-lomni_hip", f"-Wl,-rpath,{LIBDIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr[-2000:]


def test_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_wire_messages.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_wiremsg.so")
    assert os.path.exists(lib), "libomni_host_wiremsg.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported == HOST, (sorted(declared ^ exported), sorted(declared ^ HOST))
    from omni_swarm_amd import pipeline
    assert set(pipeline.WIREMSG_SYMBOLS) == declared
    L = pipeline.wiremsg_lib()
    assert all(hasattr(L, s) for s in declared)
    assert L.omni_pipeline_set_wire_messages(None, 2, 1) == 1 and b"null pipeline" in L.omni_wiremsg_last_error()
    assert L.omni_pipeline_remote_image_pending(None, None) == -1
    assert pipeline.REMOTE_EDGE_DTYPE.itemsize == 272 and pipeline.WIRE_CHANNELS[2:] == ("SWARM_LOOP_IMG_DES", "SWARM_LOOP_CONN")
    assert (pipeline.WIRE_IMG_OFF, pipeline.WIRE_IMG_IMAGE, pipeline.WIRE_IMG_WHOLE, pipeline.WIRE_IMG_PC_REPLAY) == tuple(
        int(re.search(rf"#define OMNI_WIRE_IMG_{n} (\d+)", text).group(1)) for n in ("OFF", "IMAGE", "WHOLE", "PC_REPLAY"))
    mk = open(os.path.join(ROOT, "omni-swarm_amd", "Makefile")).read()
    assert "lib/libomni_host_wiremsg.so: host/host_wiremsg_capi.cpp $(HOST_HDRS)" in mk and "../include/omni_host_wire_messages.h" in mk


def test_new_entries_of_the_kernel_library_are_declared_exported_and_bound(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libomni_hip.so")], capture_output=True, text=True).stdout
    assert NEW <= {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert c.wire_image_capacity(200, 1024) == 180 + 4 * (4096 + 71 * 200) + 200 + 1024 and c.wire_image_capacity(65) == 180 + 4 * (4096 + 71 * 65) + 68
    assert L.omni_wire_pack_image_enqueue_dev(None, 1, 8, 64, 4096, 1, 0, *([None] * 11), 0, 1, 1, None, None) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_cam_set_wire_image(None, 1, 1) == c.ERR_INVALID and L.omni_cam_wire_image(None, None) == c.ERR_INVALID
    assert ctypes.sizeof(c._CamWireImage) == 3 * 4 + 4 + 8 + 2 * 8


def test_launch_parameters_reach_the_wire(tmp_path):
    """send_img, send_whole_img_desc and is_pc_replay as the launch files set them -> what LoopNet::broadcast_img_desc sends (loop_net.cpp:37-41, 103-116)"""
    src, exe = tmp_path / "to_wire.cpp", tmp_path / "to_wire"
    src.write_text(TO_WIRE.replace("../../", ROOT + "/"))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert len(got) == 8 and all(ln[0] == "MODE" for ln in got)
    for k, ln in enumerate(got):
        img, whole, replay = k & 1, (k >> 1) & 1, (k >> 2) & 1
        assert list(map(int, ln[1:4])) == [img, whole, replay]
        want = [0, 0, 1, 1] if replay else [1, 2, int(img or whole), whole]      # replay: the whole descriptor alone; else header + the 2 flagged landmarks (+ the third packet)
        assert list(map(int, ln[5:])) == want, ln
