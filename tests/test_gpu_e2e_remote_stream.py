"""Remote key frames joining the unit stream (KeyframePipeline(..., remote_in_stream=True): include/omni_host_remote.h, host/remote_queue.hpp) on the STEREO_PINHOLE
scene and the builders of tests/test_gpu_e2e_wire.py, imported and unchanged.  Drone 2's packets for key frames 1008..1015 are made once, as in that file's
test_through_the_wire_equals_the_serial_flow: drone 2 sees what drone 1 saw at its key frames 8..15.

With the switch off every frame the wire completes stops the pipeline (flush, then on_remote_frame): the parent's serial flow, the reference here.  With it on the
frames are queued and join the key-frame units' detector batches at their place in the serial order, their rows gathered with the unit's on the GPU
(csrc/rows_assemble.hip).  No tolerance: candidates, every field of every edge, the geometry counters, the database's rows and the returned hit total are equal.
Conditions on the scene, not measurements: it yields at least one inter-drone edge and eight remote candidates on the off run (the wire test asserts the same)."""
import numpy as np
import pytest

from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests import test_gpu_e2e_wire as WT
from tests.test_gpu_e2e_landmarks import files, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the scene)

pytestmark = pytest.mark.gpu
MB = LM.MB


@pytest.fixture(scope="module")
def packets(omni, ctx, files, pinhole_scene):
    """[(msg_id, [(channel, bytes), ...])] of drone 2's key frames 1008..1015: the scene's second half through a pipeline of its own"""
    from omni_swarm_amd import pipeline
    scene, n = pinhole_scene, len(pinhole_scene)
    half = n // 2
    assert half % MB == 0
    poses = np.array([pose for _, pose in scene])
    pins = WT.stereo_blocks(ctx, scene, list(range(half, n)))
    c, P = omni.capi, SP.PARAMS
    tx = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 2,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, stereo_pinhole=SP.STEREO, device_landmarks=True, wire=True, device_wire=True)
    try:
        tx.set_stereo_extrinsics(np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
        tx.set_poses(1000 + half, poses[half:])
        tx.run(half, 1000 + half, [p.ctypes.data for p in pins], 0, None, True)
        frames = WT.drain(tx)
    finally:
        tx.close()
        for p in pins:
            ctx.host_free(p)
    assert [m for m, _ in frames] == [1000 + s for s in range(half, n)]
    return frames


def drone1(omni, files, in_stream):
    pl = LM.make(omni, files, "pinhole", True)
    pl.set_wire(True, True)
    if in_stream:
        pl.set_remote_in_stream(True)
    assert pl.remote_in_stream() is in_stream and pl.remote_pending == 0 and pl.remote_stats() == (0, 0, 0, 0)
    return pl


class Clock:
    t = 10.0


def receive(pl, frame, clock):
    """one remote key frame's packets, then the scan that completes it (recv_period has long run out)"""
    for ch, b in frame[1]:
        assert pl.recv_packet(ch, b, clock.t)
        clock.t += 0.001
    clock.t += 10.0
    pl.scan_recv(clock.t)
    clock.t += 10.0


def check_scene(off, n_remote):
    """the off run is not vacuous: every remote frame found a candidate, at least one became an inter-drone edge"""
    remote_cand = off[1][off[1][:, 0] >= 1000]
    remote_edges = [e for e in off[2] if {e[2], e[3]} == {1.0, 2.0}]
    print(f"off run: {len(off[1])} candidates ({len(remote_cand)} remote), {len(off[2])} edges ({len(remote_edges)} inter-drone), hits {off[0]}")
    assert len(remote_cand) >= n_remote and len(remote_edges) >= 1


def assert_same(on, off):
    assert on[0] == off[0]                                                     # the returned hit total (local key frames only)
    assert np.array_equal(on[1], off[1])                                       # candidates, in the serial flow's order
    assert on[2].shape == off[2].shape and np.array_equal(on[2], off[2])       # every field of every edge
    assert on[3] == off[3] and on[4] == off[4]                                 # the geometry counters, the database's rows


def test_push_keyframe_with_remote_frames_in_between(omni, ctx, files, pinhole_scene, packets):
    """(a) key frames 0..15 through push_keyframe; after key frame 8 + j drone 2's frame 1008 + j arrives; flush() at the end"""
    scene, half = pinhole_scene, len(pinhole_scene) // 2

    def run(in_stream):
        pl, clock, hits = drone1(omni, files, in_stream), Clock(), 0
        try:
            for i, (views, pose) in enumerate(scene):
                hits += pl.push_keyframe(list(views), i, float(i), pose, False)
                if i >= half:
                    receive(pl, packets[i - half], clock)
            hits += pl.flush()
            assert pl.remote_frames == half and pl.remote_pending == 0
            return WT.result(pl, hits), pl.remote_stats()
        finally:
            pl.close()

    off, off_stats = run(False)
    on, on_stats = run(True)
    print(f"remote_stats off {off_stats}, on {on_stats}")
    check_scene(off, half)
    assert off_stats == (0, 0, 0, half)                                        # every frame forced a flush
    assert on_stats[0] == half and on_stats[3] == 0 and on_stats[1] >= 1       # none did; at least one frame joined a unit's batch
    assert_same(on, off)


def test_run_in_two_halves_with_the_remote_frames_in_between(omni, ctx, files, pinhole_scene, packets):
    """(b) run() of key frames 0..7, the eight remote frames, run() of key frames 8..15: every remote frame is seen before key frame 8 -- the first at once, in a
    batch of its own (no local key frame is around and no batch is pending), the others at the head of the second half's first batch"""
    scene, n = pinhole_scene, len(pinhole_scene)
    half = n // 2
    poses = np.array([pose for _, pose in scene])
    pins = WT.stereo_blocks(ctx, scene, list(range(n)))

    def run(in_stream):
        pl, clock = drone1(omni, files, in_stream), Clock()
        try:
            pl.set_poses(0, poses)
            ptrs = [p.ctypes.data for p in pins]
            hits = pl.run(half, 0, ptrs[:half // MB], 0, None, True)
            for frame in packets:
                receive(pl, frame, clock)
            pending = pl.remote_pending
            hits += pl.run(half, half, ptrs[half // MB:], 0, None, True)
            assert pl.remote_pending == 0
            return WT.result(pl, hits), pl.remote_stats(), pending
        finally:
            pl.close()

    try:
        off, off_stats, _ = run(False)
        on, on_stats, pending = run(True)
    finally:
        for p in pins:
            ctx.host_free(p)
    print(f"remote_stats off {off_stats}, on {on_stats}; pending before the second half: {pending}")
    check_scene(off, half)
    assert off_stats == (0, 0, 0, half) and pending == half                    # nothing was collected in between: no poll, no key frame
    assert on_stats == (half, half - 1, 1, 0)
    assert_same(on, off)


def test_remote_frames_alone_leave_through_poll(omni, ctx, files, pinhole_scene):
    """(c) after drone 1's whole run: eight copies of stored frames as drone 2's, queued, then poll() until none is pending -- no key frame, no flush()"""
    scene, n = pinhole_scene, len(pinhole_scene)
    half = n // 2
    poses = np.array([pose for _, pose in scene])
    pins = WT.stereo_blocks(ctx, scene, list(range(n)))

    def run(in_stream):
        pl = LM.make(omni, files, "pinhole", True)
        try:
            if in_stream:
                pl.set_remote_in_stream(True)
            pl.set_poses(0, poses)
            hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
            if not in_stream:
                for src in range(half, n):
                    pl.recv_copy_as_remote(src, 2, 1000 + src)
                return WT.result(pl, hits), None
            for src in range(half, n):
                pl.queue_copy_as_remote(src, 2, 1000 + src)
            assert pl.remote_pending == half
            polls = 0
            while pl.remote_pending:
                hits += pl.poll()
                polls += 1
                assert polls <= 2 * half
            return WT.result(pl, hits), pl.remote_stats()
        finally:
            pl.close()

    try:
        off, _ = run(False)
        on, on_stats = run(True)
    finally:
        for p in pins:
            ctx.host_free(p)
    print(f"remote_stats on {on_stats}")
    check_scene(off, half)
    assert on_stats[0] == half and on_stats[1] == 0 and 1 <= on_stats[2] <= half and on_stats[3] == 0
    assert_same(on, off)


def test_refusals(omni, ctx, files, pinhole_scene):
    c = omni.capi
    views, pose = pinhole_scene[0]
    pl = LM.make(omni, files, "pinhole", True)
    try:
        pl.set_remote_in_stream(True)
        pl.set_remote_in_stream(False)
        assert pl.remote_in_stream() is False
        pl.push_keyframe(list(views), 0, 0.0, pose, False)
        pl.flush()
        with pytest.raises(c.OmniError, match="after the first key frame"):
            pl.set_remote_in_stream(True)
        with pytest.raises(c.OmniError, match="remote_in_stream is off"):          # the queue's entries with the switch off
            pl.queue_copy_as_remote(0, 2, 1000)
        assert pl.remote_pending == 0 and pl.remote_stats() == (0, 0, 0, 0)
    finally:
        pl.close()
    pl = LM.make(omni, files, "pinhole", True)
    try:
        pl.set_remote_in_stream(True)
        pl.push_keyframe(list(views), 0, 0.0, pose, False)
        pl.flush()
        with pytest.raises(c.OmniError, match="own id"):
            pl.queue_copy_as_remote(0, 1, 1000)
        with pytest.raises(c.OmniError, match="not in the database"):
            pl.queue_copy_as_remote(77, 2, 1000)
        with pytest.raises(c.OmniError, match="in the database already"):
            pl.queue_copy_as_remote(0, 2, 0)
        assert pl.remote_pending == 0 and pl.remote_stats() == (0, 0, 0, 0)
    finally:
        pl.close()
