"""Pairwise-consistency outlier rejection through the key-frame pipeline (KeyframePipeline(..., pcm=True): include/omni_host_pcm.h, host/loop_outlier_rejection.hpp)
on the STEREO_PINHOLE scene of tests/test_gpu_e2e_batch_verify.py, imported and unchanged: run() of key frames 0..7, drone 2's eight key frames through the wire,
run() of key frames 8..15.

The stage only adds an output.  With the switch on, the returned hits, candidates, every field of every edge with its id, the geometry / homography / PnP counters
and the database's rows equal the switch-off run's: no tolerance.  good_edges() equals the recomputation on the host -- LoopOutlierRejection fed the records the
stage entered (path lengths included), its rows from omni_pcm_rows_host, the g++ build of the header the kernels run -- edge by edge.  Once more with four fabricated
SWARM_LOOP_CONN packets of drone 2 behind the run: two made from the scene's true poses, two with a displaced relative pose; and one whose frames this pipeline never
saw, which stays outside the graph, is counted and passes."""
import struct

import numpy as np
import pytest

from tests import pcm_cases as PC
from tests import test_gpu_e2e_batch_verify as BV
from tests import test_gpu_e2e_landmarks as LM
from tests import test_gpu_e2e_remote_stream as RS
from tests import test_gpu_e2e_stereo_pinhole as SP
from tests import test_gpu_e2e_wire as WT
from tests import wire_image_cases as IC
from tests.test_gpu_e2e_landmarks import files, pinhole_scene      # noqa: F401  (module-scoped fixtures: weight files and the scene)
from tests.test_gpu_e2e_remote_stream import packets               # noqa: F401  (drone 2's key frames 1008..1015 as packets)

pytestmark = pytest.mark.gpu
MB = LM.MB


def loop_conn_packet(edge_id, kf_a, kf_b, drone_a, drone_b, rel, pose_a, pose_b, cov=0.05):
    return struct.pack(IC.EDGE, b"OMNILCN1", edge_id, kf_a, kf_b, drone_a, drone_b, 40, float(kf_a), float(kf_b), *rel, *pose_a, *pose_b, *([cov] * 6))


def fabricated(scene):
    """(id, packet) of drone 2's edges between a frame of drone 1 and one of its own frames 1008..1015, which carry the poses of key frames 8..15"""
    half = len(scene) // 2
    poses = [np.asarray(pose, np.float64) for _, pose in scene]
    rng, out = np.random.default_rng(77), []
    for k, (a, b, displaced) in enumerate([(1, 3, False), (5, 6, False), (2, 4, True), (6, 1, True)]):
        A, B = poses[a], poses[half + b]
        rel = PC.pmul(PC.pinv(A), B)
        if displaced:
            rel = PC.pmul(rel, np.concatenate([rng.normal(size=3) * 3, PC.rand_quat(rng)]))
        out.append((200000000 + k, loop_conn_packet(200000000 + k, a, 1000 + half + b, 1, 2, rel, A, B)))
    A, B = poses[0], poses[1]
    out.append((200000099, loop_conn_packet(200000099, 0, 4242, 1, 2, PC.pmul(PC.pinv(A), B), A, B)))      # frame 4242 of drone 2 never arrived
    return out


def run(omni, ctx, files, scene, packets, pcm, extra=()):
    n = len(scene)
    half = n // 2
    pins = WT.stereo_blocks(ctx, scene, list(range(n)))
    pl, clock = BV.drone1(omni, files, True, False, True, False), RS.Clock()
    try:
        assert pl.pcm()["on"] is False and pl.pcm_stats()["edges_entered"] == 0
        if pcm:
            pl.set_pcm(True)
            assert pl.pcm() == dict(on=True, pcm_thres=0.6, redundant=False, capacity=4096)
        pl.set_poses(0, np.array([pose for _, pose in scene]))
        ptrs = [p.ctypes.data for p in pins]
        hits = pl.run(half, 0, ptrs[:half // MB], 0, None, True)
        for frame in packets:
            RS.receive(pl, frame, clock)
        hits += pl.run(half, half, ptrs[half // MB:], 0, None, True)
        assert pl.remote_pending == 0
        for _, b in extra:
            assert pl.recv_packet("SWARM_LOOP_CONN", b, clock.t)
            clock.t += 0.001
        return BV.full(pl, hits), pl.good_edges(), pl.pcm_stats(), pl.pcm_records() if pcm else None, pl.remote_edges()
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


def check_against_the_host(omni, result, good, stats, records, remote):
    from omni_swarm_amd import pipeline
    ids_all = [int(i) for i in result[7]] + [int(i) for i in remote["id"]]
    host_good, host_stats = pipeline.pcm_filter_host(records, self_id=1)
    entered = {int(r["id"]): bool(g) for r, g in zip(records, host_good)}
    want = [i for i in ids_all if entered.get(i, True)]                      # an edge outside the graph passes
    assert [int(i) for i in good["id"]] == want
    for k in ("edges_entered", "pairs_evaluated", "consistent_pairs", "full_handles"):
        assert stats[k] == host_stats[k], k
    assert stats["edges_entered"] == len(records) and stats["unknown_frames"] == len(ids_all) - len(records) and stats["clique_runs"] >= 1
    return entered


def test_the_switch_only_adds_an_output_and_good_edges_equal_the_host(omni, ctx, files, pinhole_scene, packets):
    off, good_off, stats_off, _, remote_off = run(omni, ctx, files, pinhole_scene, packets, False)
    on, good, stats, records, remote = run(omni, ctx, files, pinhole_scene, packets, True)
    RS.check_scene(off, len(pinhole_scene) // 2)
    BV.assert_same(on, off)
    assert len(remote) == len(remote_off) == 0
    assert [int(i) for i in good_off["id"]] == [int(i) for i in off[7]] and set(stats_off.values()) == {0}      # without the stage: every edge, no work
    assert len(records) == len(on[7]) >= 2 and stats["unknown_frames"] == 0        # every frame of every edge went through this pipeline
    entered = check_against_the_host(omni, on, good, stats, records, remote)
    print(f"pcm on: {len(on[7])} edges, {len(good)} good; stats {stats}; verdicts {entered}")
    assert stats["pairs_evaluated"] >= 1


def test_fabricated_edges_of_the_other_drone(omni, ctx, files, pinhole_scene, packets):
    extra = fabricated(pinhole_scene)
    off = run(omni, ctx, files, pinhole_scene, packets, False)[0]
    on, good, stats, records, remote = run(omni, ctx, files, pinhole_scene, packets, True, extra)
    BV.assert_same(on, off)
    assert [int(i) for i in remote["id"]] == [i for i, _ in extra]
    entered = check_against_the_host(omni, on, good, stats, records, remote)
    fab = [entered[i] for i, _ in extra[:4]]
    print(f"fabricated edges: verdicts {fab} (true, true, displaced, displaced); stats {stats}")
    assert stats["unknown_frames"] == 1 and extra[4][0] not in entered and extra[4][0] in [int(i) for i in good["id"]]
    # the two true edges agree with each other at rounding level, whatever the scene's own edges say: never both rejected in favour of a displaced one
    recs = records[np.isin(records["id"], [i for i, _ in extra[:4]])]
    _, _, smd = omni.capi.pcm_rows_host(recs, with_smd=True)
    assert smd[1, 0] < 1e-20 and smd[2, 0] > 0.6 and smd[3, 0] > 0.6 and smd[3, 1] > 0.6 and smd[2, 1] > 0.6


def test_refusals_and_the_constructor_switch(omni, ctx, files, pinhole_scene):
    from omni_swarm_amd import pipeline
    c, P = omni.capi, SP.PARAMS
    views, pose = pinhole_scene[0]
    pl = LM.make(omni, files, "pinhole", True)
    try:
        for cap in (0, 100, 65536):
            with pytest.raises(c.OmniError, match="capacity"):
                pl.set_pcm(True, capacity=cap)
        with pytest.raises(c.OmniError, match="pcm_thres"):
            pl.set_pcm(True, pcm_thres=0.0)
        pl.set_pcm(True, 2.8, True, 128)
        assert pl.pcm() == dict(on=True, pcm_thres=2.8, redundant=True, capacity=128)
        pl.set_pcm(False)
        assert pl.pcm()["on"] is False
        pl.push_keyframe(list(views), 0, 0.0, pose, False)
        pl.flush()
        with pytest.raises(c.OmniError, match="after the first key frame"):
            pl.set_pcm(True)
    finally:
        pl.close()
    common = (0, files["sp"], files["comp"], files["mean"], files["vlad"], SP.W, SP.H, SP.THR, SP.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1, P["inner_product_thres"],
              P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"])
    pl = pipeline.KeyframePipeline(*common, geometry=True, stereo_pinhole=SP.STEREO, pcm=True, pcm_thres=1.5)
    try:
        assert pl.pcm() == dict(on=True, pcm_thres=1.5, redundant=False, capacity=4096)
    finally:
        pl.close()
    pl = pipeline.KeyframePipeline(*common, geometry=False, stereo_pinhole=SP.STEREO)
    try:
        with pytest.raises(c.OmniError, match="no geometry stage"):
            pl.set_pcm(True)
    finally:
        pl.close()
