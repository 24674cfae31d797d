"""LoopNet's other two message kinds through the key-frame pipeline (KeyframePipeline(..., wire_img_desc=, wire_loop_conn=): include/omni_host_wire_messages.h) on the
STEREO_PINHOLE scene and the two-pipeline arrangement of tests/test_gpu_e2e_wire.py, whose builders are imported and unchanged.
  (a) the new switches off: the outbox holds what it holds without them, byte for byte (also with send_img on: nothing sends the file by itself);
  (b) IMAGE and WHOLE (with and without send_img): the whole descriptors packed inside the key-frame unit (device_wire) equal LoopNetWire's on the calling thread for
      every key frame; hits, candidates, edges, counters and rows are those of a run with the wire off;
  (c) drone 1's packets fed to drone 2: take_remote_image hands out drone 1's frame_image bytes, one per sent image; remote_edges() is drone 1's edges() field for
      field, the doubles bit for bit; drone 1 fed its own packets lists nothing;
  (d) PC_REPLAY on the sender, accept_img_desc on the receiver: the frames complete from whole descriptors alone, and the receiver's candidates and edges are those of
      the header + landmark flow.
No tolerance: bytes and bits."""
import numpy as np
import pytest

from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests import wire_cases as WC
from tests import wire_image_cases as IC
from tests.test_gpu_e2e_landmarks import files, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the scene)
from tests.test_gpu_e2e_wire import drain, result, stereo_blocks

pytestmark = pytest.mark.gpu
MB = LM.MB
Q = 75


@pytest.fixture(scope="module")
def pins(ctx, pinhole_scene):
    p = stereo_blocks(ctx, pinhole_scene, list(range(len(pinhole_scene))))
    yield p
    for a in p:
        ctx.host_free(a)


def run(omni, files, scene, pins, wire=None, img="off", conn=False, send_img=False, keep=False):
    """drone 1 over the whole scene -> (result, outbox, wire_host_ms[, the pipeline])"""
    pl = LM.make(omni, files, "pinhole", True)
    try:
        if send_img:
            pl.set_send_img(True, Q)
        if wire is not None:
            pl.set_wire(True, wire)
            if img != "off" or conn:
                pl.set_wire_messages(img, conn)
        pl.set_poses(0, np.array([pose for _, pose in scene]))
        hits = pl.run(len(scene), 0, [p.ctypes.data for p in pins], 0, None, True)
        out = result(pl, hits), drain(pl), pl.wire_host_ms() if wire is not None else 0.0
        return out + (pl,) if keep else out
    finally:
        if not keep:
            pl.close()


@pytest.fixture(scope="module")
def baseline(omni, files, pinhole_scene, pins):
    """the wire off, and the wire as it is without the new switches (packed by the unit)"""
    return run(omni, files, pinhole_scene, pins)[0], run(omni, files, pinhole_scene, pins, wire=True)[1]


def same_result(r, off):
    assert r[0] == off[0] and r[3] == off[3] and r[4] == off[4] and np.array_equal(r[1], off[1]) and r[2].shape == off[2].shape and np.array_equal(r[2], off[2])


def test_switches_off_the_outbox_is_unchanged(omni, files, pinhole_scene, pins, baseline):
    off, today = baseline
    assert len(today) == len(pinhole_scene) and {ch for _, p in today for ch, _ in p} == {"VIOKF_HEADER", "VIOKF_LANDMARKS"}
    for kw in ({"img": "off", "conn": False}, {"send_img": True}):
        for device in (True, False):
            r, box, _ = run(omni, files, pinhole_scene, pins, wire=device, **kw)
            assert box == today, (kw, device)
            same_result(r, off)


@pytest.mark.parametrize("img,send_img", [("image", True), ("whole", True), ("whole", False)], ids=["image", "whole+file", "whole"])
def test_whole_descriptors_are_identical_on_both_paths(omni, files, pinhole_scene, pins, baseline, img, send_img):
    off, today = baseline
    (host, host_box, host_ms), (dev, dev_box, dev_ms) = (run(omni, files, pinhole_scene, pins, wire=d, img=img, send_img=send_img) for d in (False, True))
    whole = [b for _, p in host_box for ch, b in p if ch == "SWARM_LOOP_IMG_DES"]
    print(f"{img}, send_img {send_img}: {len(whole)} whole descriptors, {sum(map(len, whole))} bytes; calling thread in the wire: host path {host_ms:.2f} ms, device_wire {dev_ms:.2f} ms")
    assert dev_box == host_box                                                    # identical bytes, channels and order for every key frame
    assert [m for m, _ in host_box] == list(range(len(pinhole_scene)))
    for (_, p), (_, q) in zip(host_box, today):                                   # the third packet stands behind the packets the frame sends anyway
        assert [x for x in p if x[0] != "SWARM_LOOP_IMG_DES"] == q and [ch for ch, _ in p][-1] == "SWARM_LOOP_IMG_DES" and len(p) == len(q) + 1
        h, w = WC.parse_header(p[0][1]), IC.parse_image(p[-1][1])
        assert w["msg_id"] == h["msg_id"] and w["frame_id"] == h["frame_id"] and np.array_equal(w["image_desc_bits"], h["image_desc_bits"])
        assert w["landmark_num"] >= h["feature_num"] and int((w["flag"] > 0).sum()) == h["feature_num"]            # ALL landmarks travel, not only the flagged ones
        assert len(w["desc_bits"]) == (64 * w["landmark_num"] if img == "whole" else 0)
        assert (len(w["image"]) > 330) == send_img and (w["width"], w["height"]) == ((SP.W, SP.H) if send_img else (0, 0))
    same_result(host, off)
    same_result(dev, off)


def test_refusals(omni, files):
    c = omni.capi
    pl = LM.make(omni, files, "pinhole", True)
    try:
        with pytest.raises(c.OmniError, match="wire is off"):
            pl.set_wire_messages("whole", True)
        with pytest.raises(c.OmniError, match="wire is off"):
            pl.set_wire_accept_img_desc(True)
        assert pl.wire_messages() == (0, False, False) and pl.take_remote_image() is None and len(pl.remote_edges()) == 0
        pl.set_wire(True, True)
        with pytest.raises(c.OmniError, match="send_img is not in effect"):
            pl.set_wire_messages("image")
        with pytest.raises(c.OmniError, match="outside 0..3"):
            pl.set_wire_messages(4)
        pl.set_wire_messages("whole", True)
        pl.set_wire_accept_img_desc(True)
        assert pl.wire_messages() == (2, True, True)
        pl.set_send_img(True, Q)
        pl.set_wire_messages("image")
        assert pl.wire_messages() == (1, False, True)
        with pytest.raises(c.OmniError, match="IMAGE sends the file"):
            pl.set_send_img(False)
        pl.set_wire(False)                                                        # the wire off takes the switches with it
        assert pl.wire_messages() == (0, False, False)
    finally:
        pl.close()


def second_drone(omni, files, self_id=2, **kw):
    from omni_swarm_amd import pipeline
    c, P = omni.capi, SP.PARAMS
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, self_id,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, stereo_pinhole=SP.STEREO, device_landmarks=True, **kw)
    pl.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
    return pl


def test_images_and_edges_reach_the_other_drone(omni, files, pinhole_scene, pins, baseline):
    off, _ = baseline
    n = len(pinhole_scene)
    r, box, _, d1 = run(omni, files, pinhole_scene, pins, wire=True, img="whole", conn=True, send_img=True, keep=True)
    d2 = second_drone(omni, files, wire=True)
    try:
        same_result(r, off)
        frames = [(m, p) for m, p in box if p[0][0] != "SWARM_LOOP_CONN"]
        conns = [(m, p) for m, p in box if p[0][0] == "SWARM_LOOP_CONN"]
        edges = d1.edges()
        assert [m for m, _ in frames] == list(range(n)) and len(conns) == len(edges) >= 2 and all(len(p) == 1 for _, p in conns)      # an entry of its own per edge
        sent_images = [d1.frame_image(m, 0) for m in range(n)]
        assert all(len(b) > 330 for b in sent_images)
        t = 10.0
        for _, packets in box:
            for ch, b in packets:
                assert d2.recv_packet(ch, b, t)
                t += 0.001
        # (c) the images: one per sent image, in order, as drone 1 keeps them
        assert d2.remote_images_pending() == (n, 0)
        for m in range(n):
            im = d2.take_remote_image()
            assert (im["drone_id"], im["frame_id"], im["direction"], im["width"], im["height"]) == (1, m, 0, SP.W, SP.H) and im["bytes"] == sent_images[m], m
        assert d2.take_remote_image() is None
        # ... and the edges: every field that edges() lists, and every field of the packet, the doubles bit for bit
        got = d2.remote_edges()
        assert len(got) == len(edges)
        listed = np.column_stack([got["keyframe_id_a"], got["keyframe_id_b"], got["drone_id_a"], got["drone_id_b"], got["pnp_inlier_num"], got["relative_pose"]])
        assert np.array_equal(listed.view(np.uint64), np.ascontiguousarray(edges).view(np.uint64))
        for (m, p), e in zip(conns, got):
            w = IC.parse_edge(p[0][1])
            assert m == w["id"] == e["id"] and (w["keyframe_id_a"], w["keyframe_id_b"], w["drone_id_a"], w["drone_id_b"], w["pnp_inlier_num"]) == \
                (e["keyframe_id_a"], e["keyframe_id_b"], e["drone_id_a"], e["drone_id_b"], e["pnp_inlier_num"])
            doubles = np.concatenate([[e["ts_a"], e["ts_b"]], e["relative_pose"], e["self_pose_a"], e["self_pose_b"], e["pos_cov"], e["ang_cov"]])
            assert np.array_equal(doubles.view(np.uint64), w["bits"].astype(np.uint64))
        assert len({int(e["id"]) for e in got}) == len(got)
        # drone 1 fed its own packets lists nothing
        for _, packets in box:
            for ch, b in packets:
                assert d1.recv_packet(ch, b, t)
        d1.scan_recv(t + 100.0)
        assert d1.remote_images_pending() == (0, 0) and len(d1.remote_edges()) == 0 and d1.remote_frames == 0 and d1.take_remote_image() is None
    finally:
        d1.close()
        d2.close()


def test_pc_replay_frames_complete_from_whole_descriptors_alone(omni, files, pinhole_scene, pins):
    scene, n = pinhole_scene, len(pinhole_scene)
    half = n // 2
    poses = np.array([pose for _, pose in scene])

    def sender(**kw):
        tx = second_drone(omni, files, wire=True, device_wire=True, **kw)
        try:
            tx.set_poses(1000 + half, poses[half:])
            tx.run(half, 1000 + half, [p.ctypes.data for p in pins[half // MB:]], 0, None, True)
            return drain(tx)
        finally:
            tx.close()

    def receiver(frames, accept):
        rx = LM.make(omni, files, "pinhole", True)
        try:
            rx.set_wire(True, True)
            rx.set_wire_accept_img_desc(accept)
            rx.set_poses(0, poses)
            hits = rx.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
            drain(rx)
            t = 10.0
            for _, packets in frames:
                for ch, b in packets:
                    assert rx.recv_packet(ch, b, t)
                    t += 0.001
            rx.scan_recv(t + 10.0)
            return result(rx, hits), rx.remote_frames
        finally:
            rx.close()

    plain, replay = sender(), sender(wire_img_desc="pc_replay")
    assert [m for m, _ in replay] == [m for m, _ in plain] == list(range(1000 + half, 1000 + n))
    assert all([ch for ch, _ in p] == ["SWARM_LOOP_IMG_DES"] for _, p in replay)                      # one packet per image, nothing else
    for (_, p), (_, q) in zip(replay, plain):
        w, h = IC.parse_image(p[0][1]), WC.parse_header(q[0][1])
        assert w["msg_id"] >> 40 == 2 and len(w["desc_bits"]) == 64 * w["landmark_num"] and np.array_equal(w["image_desc_bits"], h["image_desc_bits"])
    want, want_frames = receiver(plain, False)
    ignored, ignored_frames = receiver(replay, False)                                                 # without the switch nothing enters the frame flow
    got, got_frames = receiver(replay, True)
    print(f"header + landmark flow: {want_frames} frames, candidates {len(want[1])}, edges {len(want[2])}; PC_REPLAY: {got_frames} frames, candidates {len(got[1])}, "
          f"edges {len(got[2])}; without accept_img_desc: {ignored_frames} frames")
    assert want_frames == got_frames == half and ignored_frames == 0 and len(ignored[1]) < len(want[1])
    assert np.array_equal(got[1], want[1])                                                            # candidates
    assert got[2].shape == want[2].shape and np.array_equal(got[2], want[2])                          # every field of every edge
    assert got[3] == want[3]
