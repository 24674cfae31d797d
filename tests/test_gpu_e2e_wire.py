"""The LoopNet wire of the key-frame pipeline (KeyframePipeline(..., wire=, device_wire=): include/omni_host_wire.h) on the rendered scenes of the existing end-to-end
tests, whose builders are imported and unchanged.

Outbound equality: STEREO_PINHOLE (raw 750 x 600 pairs), STEREO_FISHEYE (flattened views, device_landmarks) and PINHOLE_DEPTH (device_depth_landmarks) with the packets
packed on the GPU inside the key-frame unit (device_wire) and by LoopNetWire::broadcast_fisheye_desc on the calling thread: identical bytes for every key frame, and
hits, candidates, edges, geometry counters and rows identical to a run with the wire off.

Through the wire: two pipelines in one process on the STEREO_PINHOLE scene.  Drone 1 runs the whole scene; drone 2 runs the scene's second half under ids 1008..1015,
its packets (take_packets) go to drone 1 (recv_packet, scan_recv).  Against: the same drone-1 run followed by the existing hook (omni_pipeline_recv_copy_as_remote),
which hands on_remote_frame copies of drone 1's OWN stored frames 8..15 as frames 1008..1015 of drone 2 -- the same pictures through the same networks.  No tolerance:
bytes and bits."""
import numpy as np
import pytest

from tests import test_gpu_e2e_depth_device as DD
from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_scene as FE
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests import wire_cases as WC
from tests.test_gpu_e2e_landmarks import files, fisheye_scene, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the two scenes)
from tests.test_gpu_e2e_depth_device import scene as depth_scene                 # noqa: F401

pytestmark = pytest.mark.gpu
MB = LM.MB
MODES = {"off": (False, False), "host": (True, False), "device": (True, True)}


def stereo_blocks(ctx, scene, frames):
    """pinned blocks of MB key frames each, laid out as run() takes them: the up / left images of the block, then its down / right images"""
    dirs, pins = scene[0][0].shape[0] // 2, []
    for s in range(0, len(frames), MB):
        kf = [scene[frames[s + m]][0] for m in range(MB)]
        p = ctx.host_alloc((2 * dirs * MB,) + kf[0].shape[1:], np.uint8)
        p[:] = np.stack([kf[m][i] for m in range(MB) for i in range(dirs)] + [kf[m][dirs + i] for m in range(MB) for i in range(dirs)])
        pins.append(p)
    return pins


def drain(pl):
    out = []
    while pl.wire_pending:
        out.append(pl.take_packets())
    return out


def result(pl, hits):
    return hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows


def stereo_through(omni, ctx, files, scene_kind, scene, mode, streaming):
    pl = LM.make(omni, files, scene_kind, True)
    pins = []
    try:
        if MODES[mode][0]:
            pl.set_wire(*MODES[mode])
        assert pl.wire()[:2] == MODES[mode]
        if streaming:
            hits = 0
            for i, (views, pose) in enumerate(scene):
                hits += pl.push_keyframe(list(views), i, float(i), pose, False)
            hits += pl.flush()
        else:
            pins = stereo_blocks(ctx, scene, list(range(len(scene))))
            pl.set_poses(0, np.array([pose for _, pose in scene]))
            hits = pl.run(len(scene), 0, [p.ctypes.data for p in pins], 0, None, True)
        if MODES[mode][0]:
            with pytest.raises(omni.capi.OmniError, match="after the first key frame"):
                pl.set_wire(False)
        ms = pl.wire_host_ms() if MODES[mode][0] else 0.0
        return result(pl, hits), drain(pl), ms
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


def depth_through(omni, scene, mode):
    pl = DD.make(omni, scene, "distorted", True, MB)
    try:
        if MODES[mode][0]:
            pl.set_wire(*MODES[mode])
        n = len(scene["plan"])
        pl.set_poses(0, scene["poses"])
        pl.set_depth(0, np.stack([f[1] for f in scene["frames"]]))
        hits = pl.run(n, 0, [p.ctypes.data for p in scene["pins"]], 0, None, True)
        return result(pl, hits), drain(pl), pl.wire_host_ms() if MODES[mode][0] else 0.0
    finally:
        pl.close()


def check_outbound(what, n_frames, dirs, got):
    (off, none, _), (host, host_pk, host_ms), (dev, dev_pk, dev_ms) = got["off"], got["host"], got["device"]
    n_pk, n_bytes = sum(len(p) for _, p in host_pk), sum(len(b) for _, p in host_pk for _, b in p)
    print(f"{what}: {n_frames} key frames -> {n_pk} packets, {n_bytes} bytes; candidates {len(off[1])}, edges {len(off[2])}; calling thread in the wire: host path {host_ms:.2f} ms, "
          f"device_wire {dev_ms:.2f} ms")
    assert none == [] and len(off[1]) >= 4 and len(off[2]) >= 2                    # the wire off keeps nothing; the scene is not vacuous
    assert [m for m, _ in host_pk] == list(range(n_frames)) == [m for m, _ in dev_pk]      # every key frame, in order
    headers = [WC.parse_header(b) for _, p in host_pk for ch, b in p if ch == "VIOKF_HEADER"]
    assert len(headers) >= n_frames * dirs - 2 and sum(h["feature_num"] for h in headers) > 50 and n_pk == len(headers) + sum(h["feature_num"] for h in headers)
    assert len({h["msg_id"] for h in headers}) == len(headers) and all(h["msg_id"] >> 40 == 1 for h in headers)      # numbered in the wire's own sequence
    assert dev_pk == host_pk                                                      # identical bytes, channels and order for every key frame
    for r in (host, dev):                                                         # ... and nothing downstream changes
        assert r[0] == off[0] and r[3] == off[3] and r[4] == off[4] and np.array_equal(r[1], off[1])
        assert r[2].shape == off[2].shape and np.array_equal(r[2], off[2])


@pytest.mark.parametrize("scene_kind,streaming", [("pinhole", False), ("pinhole", True), ("fisheye", False)], ids=["pinhole-run", "pinhole-push_keyframe", "fisheye-run"])
def test_outbound_packets_are_identical_on_both_paths_stereo(omni, ctx, files, fisheye_scene, pinhole_scene, scene_kind, streaming):
    scene = fisheye_scene if scene_kind == "fisheye" else pinhole_scene
    got = {mode: stereo_through(omni, ctx, files, scene_kind, scene, mode, streaming) for mode in MODES}
    check_outbound(f"{scene_kind}, {'push_keyframe' if streaming else 'run'}", len(scene), scene[0][0].shape[0] // 2, got)


def test_outbound_packets_are_identical_on_both_paths_pinhole_depth(omni, ctx, depth_scene):
    got = {mode: depth_through(omni, depth_scene, mode) for mode in MODES}
    check_outbound("PINHOLE_DEPTH, run", len(depth_scene["plan"]), 1, got)


def test_refusals(omni, ctx, files, depth_scene):
    c = omni.capi
    pl = LM.make(omni, files, "pinhole", False)                                   # the landmarks on the host's geometry threads
    try:
        with pytest.raises(c.OmniError, match="device_landmarks"):
            pl.set_wire(True, True)
        with pytest.raises(c.OmniError, match="without wire"):
            pl.set_wire(False, True)
        with pytest.raises(c.OmniError, match="wire is off"):
            pl.recv_packet("VIOKF_HEADER", b"x", 0.0)
        with pytest.raises(c.OmniError, match="no key frame"):
            pl.take_packets()
        pl.set_wire(True)                                                         # the host path needs nothing of the unit
        assert pl.wire() == (True, False, False) and pl.wire_pending == 0 and pl.remote_frames == 0
        assert pl.recv_packet("VIOKF_HEADER", b"junk", 0.0) is False and pl.recv_packet("SOMETHING_ELSE", b"", 0.0) is False
        pl.set_device_landmarks(True)
        pl.set_wire(True, True, True)
        assert pl.wire() == (True, True, True)
        with pytest.raises(c.OmniError, match="device_wire packs"):
            pl.set_device_landmarks(False)
        pl.set_wire(False)
        assert pl.wire() == (False, False, False)
    finally:
        pl.close()
    pl = DD.make(omni, depth_scene, "ideal", False, MB)                           # PINHOLE_DEPTH with its landmarks read on the calling thread
    try:
        with pytest.raises(c.OmniError, match="device_depth_landmarks"):
            pl.set_wire(True, True)
    finally:
        pl.close()


def test_through_the_wire_equals_the_serial_flow(omni, ctx, files, pinhole_scene):
    scene, n = pinhole_scene, len(pinhole_scene)
    half = n // 2
    assert half % MB == 0
    poses = np.array([pose for _, pose in scene])
    sent = list(range(half, n))                                                   # drone 2 sees what drone 1 saw at its key frames 8..15
    pins = stereo_blocks(ctx, scene, list(range(n)))

    def drone1(wire):
        pl = LM.make(omni, files, "pinhole", True)
        if wire:
            pl.set_wire(True, True)
        pl.set_poses(0, poses)
        hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
        return pl, hits

    try:
        # the parent's serial flow first: the hook hands on_remote_frame copies of the stored frames
        pl, hits = drone1(False)
        try:
            n_cand, n_edges = len(pl.candidates()), len(pl.edges())
            verdicts = [pl.recv_copy_as_remote(src, 2, 1000 + src) for src in sent]
            want = result(pl, hits)
        finally:
            pl.close()
        remote_edges = want[2][n_edges:]
        print(f"serial flow: verdicts {verdicts}; candidates {n_cand} -> {len(want[1])}, edges {n_edges} -> {len(want[2])}")
        assert len(want[1]) == n_cand + len(sent) and len(remote_edges) >= 1      # a condition on the scene: at least one inter-drone edge
        assert set(remote_edges[:, 2]) | set(remote_edges[:, 3]) == {1.0, 2.0}
        # through the wire
        from omni_swarm_amd import pipeline
        c, P = omni.capi, SP.PARAMS
        tx = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 2,
                                       P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                       geometry=True, stereo_pinhole=SP.STEREO, device_landmarks=True, wire=True, device_wire=True)
        try:
            tx.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
            tx.set_poses(1000 + half, poses[half:])
            tx.run(half, 1000 + half, [p.ctypes.data for p in pins[half // MB:]], 0, None, True)
            frames = drain(tx)
            own = [(ch, b) for _, p in frames[:1] for ch, b in p]
            assert [m for m, _ in frames] == [1000 + s for s in sent]
            assert all(tx.recv_packet(ch, b, 1.0) for ch, b in own) and tx.remote_frames == 0      # a pipeline ignores its own packets (sent_message)
            tx.scan_recv(100.0)
            assert tx.remote_frames == 0
        finally:
            tx.close()
        rx, hits = drone1(True)
        try:
            drain(rx)                                                             # (its own packets are not part of this test)
            t = 10.0
            for _, packets in frames:
                for ch, b in packets:
                    assert rx.recv_packet(ch, b, t)
                    t += 0.001
            rx.scan_recv(t + 10.0)
            got = result(rx, hits)
            print(f"through the wire: {sum(len(p) for _, p in frames)} packets, {rx.remote_frames} frames completed; candidates {len(got[1])}, edges {len(got[2])}")
            assert rx.remote_frames == len(sent)
        finally:
            rx.close()
        assert np.array_equal(got[1], want[1])                                    # candidates
        assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2])  # every field of every edge
        assert got[3] == want[3]
    finally:
        for p in pins:
            ctx.host_free(p)
