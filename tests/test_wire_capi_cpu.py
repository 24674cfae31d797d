"""CPU-side checks of what the LoopNet wire adds to the C boundaries (no GPU): a gcc C99 program built against the two headers (include/omni_hip.h,
include/omni_host_wire.h) links the new entries of both libraries, checks the capacity formula and every refusal -- a code and a message before anything is
launched or dereferenced; libomni_host_wire.so exports exactly what its header declares and pipeline.py binds exactly that; capi.py binds the entries of
libomni_hip.so."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "omni-swarm_amd", "lib")
NEW = {"omni_wire_packet_capacity", "omni_wire_table_ints", "omni_wire_pack_enqueue_dev", "omni_wire_pack_host", "omni_cam_set_wire", "omni_cam_set_wire_meta", "omni_cam_wire"}

PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "omni_hip.h"
#include "omni_host_wire.h"
#define CHECK(c) do { if (!(c)) { printf("FAIL line %d: %s (last error: %s)\n", __LINE__, #c, omni_last_error()); return 1; } } while (0)
static float kps[8 * 2], desc[8 * 64], norm[8 * 2], l3d[8 * 3], global[4096];
static int n_kps[1] = {8}, table[2 + 2 * 9];
static uint8_t flag[8], out[3 + 16545 + 324 * 8 + 4];
static omni_wire_image_meta meta[1];
int main(void) {
    int m;
    long fake_ctx[64];                       /* never dereferenced: every call below is refused before the context is touched */
    omni_ctx* ctx = (omni_ctx*)fake_ctx;
    CHECK(sizeof(omni_wire_image_meta) == 144);
    CHECK(OMNI_WIRE_HEADER_BYTES == 161 + 4 * 4096 && OMNI_WIRE_LANDMARK_BYTES == 36 + 28 + 4 + 4 * 64 && (OMNI_WIRE_HEADER_OFFSET + 161) % 4 == 0);
    for (m = 1; m <= 1024; ++m) {
        CHECK(omni_wire_packet_capacity(m) == OMNI_WIRE_HEADER_OFFSET + OMNI_WIRE_HEADER_BYTES + (int64_t)OMNI_WIRE_LANDMARK_BYTES * m);
        CHECK(omni_wire_packet_capacity(m) % 4 == 0 && omni_wire_table_ints(m) == 2 + 2 * (1 + m));
    }
    CHECK(omni_wire_packet_capacity(0) == 0 && omni_wire_packet_capacity(1025) == 0 && omni_wire_packet_capacity(-1) == 0);
    CHECK(omni_wire_table_ints(0) == 0 && omni_wire_table_ints(1025) == 0);
#define DEV(c, ni, mn, dd, gd, k, o) omni_wire_pack_enqueue_dev(c, ni, mn, dd, gd, 0, k, n_kps, desc, norm, l3d, flag, global, meta, o, table)
#define HOST(ni, mn, dd, gd, k, o) omni_wire_pack_host(ni, mn, dd, gd, 0, k, n_kps, desc, norm, l3d, flag, global, meta, o, table)
    CHECK(DEV(NULL, 1, 8, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "null"));
    CHECK(DEV(ctx, 1, 8, 64, 4096, NULL, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "null"));
    CHECK(DEV(ctx, 1, 8, 64, 4096, kps, NULL) == OMNI_ERR_INVALID && strstr(omni_last_error(), "null"));
    CHECK(DEV(ctx, 1, 0, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "max_num"));
    CHECK(DEV(ctx, 1, 1025, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "max_num"));
    CHECK(DEV(ctx, 1, 8, 63, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "64"));
    CHECK(DEV(ctx, 1, 8, 256, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "64"));
    CHECK(DEV(ctx, 1, 8, 64, 4095, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "4096"));
    CHECK(DEV(ctx, 0, 8, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_images"));
    CHECK(DEV(ctx, 1, 8, 64, 4096, kps, out + 1) == OMNI_ERR_INVALID && strstr(omni_last_error(), "aligned"));
    CHECK(HOST(1, 8, 64, 4096, NULL, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "null"));
    CHECK(HOST(1, 0, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "max_num"));
    CHECK(HOST(1, 1025, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "max_num"));
    CHECK(HOST(1, 8, 65, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "64"));
    CHECK(HOST(1, 8, 64, 4097, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "4096"));
    CHECK(HOST(0, 8, 64, 4096, kps, out) == OMNI_ERR_INVALID && strstr(omni_last_error(), "n_images"));
    /* and the host entry accepts good arguments, misaligned output included */
    memset(flag, 1, sizeof flag);
    CHECK(HOST(1, 8, 64, 4096, kps, out + 1) == OMNI_OK && table[0] == 9 && table[1] == omni_wire_packet_capacity(8) && table[2] == OMNI_WIRE_HEADER_OFFSET);
    CHECK(memcmp(out + 1 + OMNI_WIRE_HEADER_OFFSET, "OMNIHDR1", 8) == 0 && memcmp(out + 1 + table[4], "OMNILMK1", 8) == 0 && table[5] == OMNI_WIRE_LANDMARK_BYTES);
    /* the pipeline's entries: a null pipeline is a code and a message, not a crash */
    {
        int a = 7, b = 7, n_packets = 0;
        int64_t n_bytes = 0;
        double ms = 0;
        CHECK(omni_pipeline_set_wire(NULL, 1, 1, 0) == 1 && strstr(omni_wire_host_last_error(), "null pipeline"));
        CHECK(omni_pipeline_get_wire(NULL, &a, &b, NULL) == 1 && a == 7 && b == 7);
        CHECK(omni_pipeline_take_packets(NULL, NULL, NULL, 0, &n_bytes, NULL, NULL, NULL, 0, &n_packets) == 1 && strstr(omni_wire_host_last_error(), "null pipeline"));
        CHECK(omni_pipeline_set_wire_recv(NULL, 0.5, 3, 0) == 1 && omni_pipeline_recv_packet(NULL, "VIOKF_HEADER", out, 4, 0.0, &a) == 1 && omni_pipeline_scan_recv(NULL, 0.0) == 1);
        CHECK(omni_pipeline_wire_pending(NULL) == -1 && omni_pipeline_remote_frames(NULL) == -1 && omni_pipeline_wire_host_ms(NULL, &ms, 0) == 1);
        CHECK(OMNI_WIRE_CHANNEL_HEADER == 0 && OMNI_WIRE_CHANNEL_LANDMARKS == 1);
    }
    printf("OK\n");
    return 0;
}
"""


def test_c_program_links_the_entries_checks_capacity_and_every_refusal(tmp_path):
    src, exe = tmp_path / "wire_capi.c", tmp_path / "wire_capi"
    src.write_text(PROGRAM)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", LIBDIR,
                        "-lomni_host_wire", "-lomni_hip", f"-Wl,-rpath,{LIBDIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr[-2000:]


def test_new_entries_are_declared_exported_and_bound(omni):
    c = omni.capi
    L = c.lib()
    hdr = open(os.path.join(ROOT, "include", "omni_hip.h")).read()
    assert NEW <= set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", hdr)) and NEW <= set(c.SYMBOLS) and all(hasattr(L, s) for s in NEW)
    assert "#define OMNI_ABI_VERSION 2 " in hdr and L.omni_abi_version() == 2                 # additions only
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libomni_hip.so")], capture_output=True, text=True).stdout
    assert NEW <= {l.split()[-1] for l in nm.splitlines() if " T " in l}
    assert ctypes.sizeof(c.WireImageMeta) == c.WIRE_META_DTYPE.itemsize == 144
    assert [(n, c.WIRE_META_DTYPE.fields[n][1]) for n in c.WIRE_META_DTYPE.names] == [(n, getattr(c.WireImageMeta, n).offset) for n, _ in c.WireImageMeta._fields_]
    assert (c.WIRE_HEADER_BYTES, c.WIRE_LANDMARK_BYTES, c.WIRE_HEADER_OFFSET) == tuple(
        int(re.search(rf"#define OMNI_WIRE_{n} (\d+)", hdr).group(1)) for n in ("HEADER_BYTES", "LANDMARK_BYTES", "HEADER_OFFSET"))
    assert c.wire_packet_capacity(200) == 3 + 16545 + 324 * 200 and c.wire_table_ints(200) == 2 + 2 * 201 and c.wire_packet_capacity(1025) == 0
    assert L.omni_wire_pack_enqueue_dev(None, 1, 8, 64, 4096, 0, *([None] * 10)) == c.ERR_INVALID and b"null" in L.omni_last_error()
    assert L.omni_cam_set_wire(None, 1, 0) == c.ERR_INVALID and L.omni_cam_set_wire_meta(None, None, 1) == c.ERR_INVALID and L.omni_cam_wire(None, None) == c.ERR_INVALID
    assert ctypes.sizeof(c._CamWire) == 4 * 4 + 8 + 2 * 8


def test_wire_host_library_exports_what_its_c_header_declares():
    hdr_path = os.path.join(ROOT, "include", "omni_host_wire.h")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr_path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = re.sub(r"/\*.*?\*/", "", open(hdr_path).read(), flags=re.S)
    declared = set(re.findall(r"\b(omni_[a-z0-9_]+)\s*\(", text))
    lib = os.path.join(LIBDIR, "libomni_host_wire.so")
    assert os.path.exists(lib), "libomni_host_wire.so missing: run __graft_entry__.build()"
    nm = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if l.split() and l.split()[-1].startswith("omni_") and " T " in l}
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    from omni_swarm_amd import pipeline
    assert set(pipeline.WIRE_SYMBOLS) == declared
    L = pipeline.wire_lib()
    assert all(hasattr(L, s) for s in declared)
    assert L.omni_pipeline_set_wire(None, 1, 0, 0) == 1 and b"null pipeline" in L.omni_wire_host_last_error()


def test_launch_parameters_hand_on_send_all_features():
    """SwarmLoopParams::to_pipeline_config: the launch files' send_all_features reaches KeyframePipeline::Config (taken up when the wire is switched on)"""
    text = open(os.path.join(ROOT, "omni-swarm_amd", "host", "swarm_loop_params.hpp")).read()
    body = text[text.index("void to_pipeline_config"):]
    assert "c.send_all_features = send_all_features;" in body[:body.index("\n    }")]
