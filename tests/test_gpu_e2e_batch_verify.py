"""Inter-drone loop candidates verified with their batch (KeyframePipeline(..., batch_verify=True): include/omni_host_verify.h, host/verify_plan.hpp) on the
STEREO_PINHOLE scene, the packets and the three arrival patterns of tests/test_gpu_e2e_remote_stream.py, imported and unchanged: remote frames between
push_keyframe calls, between two run() halves, and alone through poll() -- each with remote_in_stream on and off.

With the switch off a candidate between a frame of drone 2 and a frame of drone 1 is verified on the spot, in a round trip of its own: the parent's flow, the
reference here.  With it on such candidates wait for the end of their detector batch.  No tolerance: candidates, every field of every edge (ids and order included),
the geometry and homography / PnP counters, the database's rows and the returned hit total are equal.  With the default inter_drone_init_frames = 50, which the
scene's inter-drone edges never reach, no mode ever depends on a pending verdict: zero early resolves and at most one matcher round trip per resolved batch -- and
where seven remote frames share a batch, fewer round trips than candidates, which verifying on the spot cannot do.  Once more with inter_drone_init_frames = 3
through the launch parameter: the crossing falls inside a batch, the results are again identical and the rule forces at least one early resolve.  With device_homography
(the default) every candidate's correspondences come out of the matcher's round trip (csrc/corr_assemble.hip); with the homography on the host none do."""
import numpy as np
import pytest

from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_remote_stream as RS
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests import test_gpu_e2e_wire as WT
from tests.test_gpu_e2e_landmarks import files, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the scene)
from tests.test_gpu_e2e_remote_stream import packets               # noqa: F401  (drone 2's key frames 1008..1015 as packets)

pytestmark = pytest.mark.gpu
MB = LM.MB
P = SP.PARAMS
LAUNCH = ('<launch><node pkg="swarm_loop" type="swarm_loop_node" name="swarm_loop">'
          '<param name="self_id" value="1" type="int"/><param name="camera_configuration" value="0" type="int"/>'
          f'<param name="query_thres" value="{P["inner_product_thres"]}" type="double"/><param name="init_query_thres" value="{P["init_mode_product_thres"]}" type="double"/>'
          f'<param name="match_index_dist" value="{P["match_index_dist"]}" type="int"/><param name="min_loop_feature_num" value="{P["min_loop_num"]}" type="int"/>'
          f'<param name="min_direction_loop" value="{P["min_direction_loop"]}" type="int"/><param name="inter_drone_init_frames" value="3" type="int"/>'
          '</node></launch>')


HOST_HOMOGRAPHY = False      # set by the one test that runs the homography RANSAC on the host's geometry threads


def drone1(omni, files, in_stream, batch_verify, wire, launch):
    pl = LM.make(omni, files, "pinhole", True)
    if HOST_HOMOGRAPHY:
        pl.set_device_homography(False)
    if wire:
        pl.set_wire(True, True)
    if in_stream:
        pl.set_remote_in_stream(True)
    assert pl.batch_verify() is False and pl.verify_stats() == (0, 0, 0, 0)
    if batch_verify:
        pl.set_batch_verify(True)
    assert pl.batch_verify() is batch_verify
    if launch:
        pl.apply_launch(LAUNCH)
    return pl


def full(pl, hits):
    """WT.result plus the homography / PnP counters (device, host) and the edge ids"""
    return WT.result(pl, hits) + (pl.device_homography()[1:], pl.device_pnp()[1:], pl.edge_ids())


def run_push(omni, ctx, files, scene, packets, in_stream, bv, launch=False):
    """(a) key frames 0..15 through push_keyframe; after key frame 8 + j drone 2's frame 1008 + j arrives; flush() at the end"""
    half = len(scene) // 2
    pl, clock, hits = drone1(omni, files, in_stream, bv, True, launch), RS.Clock(), 0
    try:
        for i, (views, pose) in enumerate(scene):
            hits += pl.push_keyframe(list(views), i, float(i), pose, False)
            if i >= half:
                RS.receive(pl, packets[i - half], clock)
        hits += pl.flush()
        assert pl.remote_frames == half and pl.remote_pending == 0
        return full(pl, hits), pl.verify_stats() + pl.corr_stats()
    finally:
        pl.close()


def run_halves(omni, ctx, files, scene, packets, in_stream, bv, launch=False):
    """(b) run() of key frames 0..7, the eight remote frames, run() of key frames 8..15"""
    n = len(scene)
    half = n // 2
    pins = WT.stereo_blocks(ctx, scene, list(range(n)))
    pl, clock = drone1(omni, files, in_stream, bv, True, launch), RS.Clock()
    try:
        pl.set_poses(0, np.array([pose for _, pose in scene]))
        ptrs = [p.ctypes.data for p in pins]
        hits = pl.run(half, 0, ptrs[:half // MB], 0, None, True)
        for frame in packets:
            RS.receive(pl, frame, clock)
        hits += pl.run(half, half, ptrs[half // MB:], 0, None, True)
        assert pl.remote_pending == 0
        return full(pl, hits), pl.verify_stats() + pl.corr_stats()
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


def run_alone(omni, ctx, files, scene, packets, in_stream, bv, launch=False):
    """(c) after drone 1's whole run: eight copies of stored frames as drone 2's -- handed over one by one, or queued and left to poll()"""
    n = len(scene)
    half = n // 2
    pins = WT.stereo_blocks(ctx, scene, list(range(n)))
    pl = drone1(omni, files, in_stream, bv, False, launch)
    try:
        pl.set_poses(0, np.array([pose for _, pose in scene]))
        hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
        if not in_stream:
            for src in range(half, n):
                pl.recv_copy_as_remote(src, 2, 1000 + src)
        else:
            for src in range(half, n):
                pl.queue_copy_as_remote(src, 2, 1000 + src)
            polls = 0
            while pl.remote_pending:
                hits += pl.poll()
                polls += 1
                assert polls <= 2 * half
        return full(pl, hits), pl.verify_stats() + pl.corr_stats()
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


PATTERNS = {"push": run_push, "halves": run_halves, "alone": run_alone}


def assert_same(on, off):
    RS.assert_same(on, off)
    assert on[5] == off[5] and on[6] == off[6]                                 # homography pairs and PnP candidates, device / host
    assert len(on[7]) == len(on[2]) and np.array_equal(on[7], off[7])          # the edge ids: number_edge ran in candidate order


@pytest.mark.parametrize("in_stream", [False, True], ids=["flush", "in_stream"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_batch_verify_equals_verifying_on_the_spot(omni, ctx, files, pinhole_scene, packets, pattern, in_stream):
    half = len(pinhole_scene) // 2
    off, off_stats = PATTERNS[pattern](omni, ctx, files, pinhole_scene, packets, in_stream, False)
    on, on_stats = PATTERNS[pattern](omni, ctx, files, pinhole_scene, packets, in_stream, True)
    print(f"{pattern}, remote_in_stream {in_stream}: verify_stats off {off_stats}, on {on_stats}; geometry {on[3]}, homography {on[5]}, pnp {on[6]}")
    RS.check_scene(off, half)
    assert off_stats == (0, 0, 0, 0, 0, 0)
    assert_same(on, off)
    deferred, end_resolves, early, round_trips, corr_device, corr_host = on_stats
    assert corr_device == on[3][0] and corr_host == 0          # every candidate's correspondences came from the matcher's round trip (csrc/corr_assemble.hip)
    assert deferred >= half                                    # every remote frame found a candidate against a frame of this drone
    assert early == 0                                          # init mode never ends: no mode depends on a pending verdict
    assert 1 <= round_trips <= end_resolves <= deferred        # at most one round trip per detector batch that had something to resolve
    if pattern == "halves" and in_stream:                      # seven remote frames share the second half's first batch
        assert round_trips <= deferred - (half - 2)


def test_the_crossing_inside_a_batch_forces_an_early_resolve(omni, ctx, files, pinhole_scene, packets):
    """inter_drone_init_frames = 3 through the launch parameter, the pattern whose batch holds seven remote frames"""
    off, off_stats = run_halves(omni, ctx, files, pinhole_scene, packets, True, False, launch=True)
    on, on_stats = run_halves(omni, ctx, files, pinhole_scene, packets, True, True, launch=True)
    inter = [e for e in off[2] if {e[2], e[3]} == {1.0, 2.0}]
    print(f"inter_drone_init_frames 3: verify_stats on {on_stats}; {len(off[1])} candidates, {len(off[2])} edges ({len(inter)} inter-drone)")
    assert len(inter) >= 4                                     # a condition on the scene: the counter passes 3 with remote frames still to come
    assert off_stats == (0, 0, 0, 0, 0, 0)
    assert_same(on, off)
    assert on_stats[2] >= 1 and on_stats[3] <= on_stats[1] + on_stats[2]


def test_with_the_homography_on_the_host_the_batch_takes_the_tasks_path(omni, ctx, files, pinhole_scene, packets, monkeypatch):
    """device_homography off: the round trip returns raw matches only, no correspondences are assembled on the GPU, and the results are still the same"""
    monkeypatch.setattr(__import__(__name__, fromlist=["x"]), "HOST_HOMOGRAPHY", True)
    off, off_stats = run_halves(omni, ctx, files, pinhole_scene, packets, True, False)
    on, on_stats = run_halves(omni, ctx, files, pinhole_scene, packets, True, True)
    print(f"host homography: verify_stats on {on_stats}; homography {on[5]}")
    assert_same(on, off)
    assert on[5][0] == 0 and on_stats[4:] == (0, 0) and on_stats[2] == 0 and 1 <= on_stats[3] <= on_stats[1]


def test_refusals_and_the_constructor_switch(omni, ctx, files, pinhole_scene):
    from omni_swarm_amd import pipeline
    c = omni.capi
    views, pose = pinhole_scene[0]
    pl = LM.make(omni, files, "pinhole", True)
    try:
        pl.set_batch_verify(True)
        pl.set_batch_verify(False)
        assert pl.batch_verify() is False
        pl.push_keyframe(list(views), 0, 0.0, pose, False)
        pl.flush()
        pl.set_batch_verify(True)                              # between two calls is fine: nothing is pending
        assert pl.batch_verify() is True and pl.verify_stats() == (0, 0, 0, 0)
    finally:
        pl.close()
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, stereo_pinhole=SP.STEREO, batch_verify=True)
    try:
        assert pl.batch_verify() is True
    finally:
        pl.close()
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=False, stereo_pinhole=SP.STEREO)
    try:
        with pytest.raises(c.OmniError, match="no geometry stage"):
            pl.set_batch_verify(True)
    finally:
        pl.close()
