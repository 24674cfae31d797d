"""End to end in the raw-fisheye mode of CameraConfig::STEREO_FISHEYE (KeyframePipeline::Config::fisheye_src_width ...): a stream of 20 key frames, each ONE up and
ONE down fisheye frame, through three C++ key-frame pipelines --
  (i)   the existing mode: the four side views of both cameras made by capi.Flatten from the frames and handed over as 8 flattened views,
  (ii)  raw_fisheye: the two frames as pixels, flattened inside every unit (omni_cam_enqueue_fisheye_host),
  (iii) raw_fisheye + compressed_images: the two frames as JPEG files, decoded and flattened inside every unit (omni_cam_enqueue_fisheye_jpeg_host),
(i) and (ii) fed the host-decoded pixels (omni_jpeg_decode_host) of (iii)'s files -- once through run() / run_jpeg() in units of 4 and once through push_keyframe /
push_keyframe_jpeg + flush() in units of 3.  All three run the same network kernels on the same bytes: database size, hits, candidates, every field of every
LoopEdge (bits) and the geometry counters are identical, and jpeg_corrupt() stays 0.  The reference has no such path (its upstream, VINS-Fisheye, decodes and
flattens): parity is against this project's own modes.  The key-frame messages and the database rows themselves are not readable from Python;
tests/test_gpu_cam_fisheye_jpeg.py holds every field of a unit's result -- the global descriptors that become the rows among them -- bit-identical.

Stream: 12 places, then 8 revisits that repeat an earlier place's fisheye pair exactly, with a drifted odometry pose.  An up frame is synth.image_u8; the down
frame shows what the up frame shows, displaced the way the rig's 10 cm baseline displaces a wall 1.25 m away: every side view of the down camera is the up
camera's side view 8 rows further down (f B / Z = 100 x 0.10 / 1.25; a multiple of the networks' 8-pixel cell, as synth.ROOM_DISPARITY), painted into the down
camera's fisheye frame through its own maps at four times the views' resolution.
Rig: the one of tests/test_gpu_cam_fisheye_jpeg.py (432 x 352 frames, 200 x 104 side views)."""
import numpy as np
import pytest

from oracle import flatten_ref as F
from oracle import geometry_ref as G
from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests.test_gpu_cam_fisheye_jpeg import FOV, SRC_H, SRC_W, VH, VW, coded, mei

pytestmark = pytest.mark.gpu
THR, MAXN, QUALITY, DIRS = 0.015, 200, 75, 4
N_PLACES, N_KF = 12, 20
DISPARITY, UPSCALE, N_SHAPES = 8, 4, 400                                                     # rows between the up and the down view of a wall point; the painting's oversampling
PARAMS = dict(inner_product_thres=0.3, init_mode_product_thres=0.2, match_index_dist=5, min_loop_num=30, min_direction_loop=3)      # tests/test_gpu_e2e_scene.py's


def schedule():
    """key frame i -> (place, reported odometry pose): 12 first visits, then 8 revisits in another order, each with a drifted pose"""
    out = [(p, G.pose([10.0 * p, 2.0 * (p % 3), 1.0], G.q_from_yaw(0.03 * p))) for p in range(N_PLACES)]
    for i in range(N_KF - N_PLACES):
        p = (5 * i + 3) % N_PLACES
        true = out[p][1]
        out.append((p, G.pose(true[0] + np.array([0.30, -0.20, 0.05]), G.qmul(G.q_from_yaw(0.02), true[1]))))
    return out


def down_frame(up, maps_up_hi, maps_down_hi):
    """the down camera's fisheye frame of a wall the up camera sees as `up`: side view v of the down camera at (x, y) = side view v of the up camera at (x, y + d)"""
    d = DISPARITY * UPSCALE
    total, hits = np.zeros(SRC_H * SRC_W), np.zeros(SRC_H * SRC_W)
    for v in range(1, 5):
        view = F.remap_linear(up, maps_up_hi[v])                              # the up camera's side view, oversampled
        m = maps_down_hi[v][:view.shape[0] - d]
        x, y = np.rint(m[..., 0]).astype(np.int64), np.rint(m[..., 1]).astype(np.int64)
        ok = (x >= 0) & (x < SRC_W) & (y >= 0) & (y < SRC_H)
        at = y[ok] * SRC_W + x[ok]                                            # a frame pixel is the mean of the view samples that land in it
        total += np.bincount(at, view[d:][ok].astype(np.float64), SRC_H * SRC_W)
        hits += np.bincount(at, None, SRC_H * SRC_W)
    return np.rint(total / np.maximum(hits, 1)).astype(np.uint8).reshape(SRC_H, SRC_W)


@pytest.fixture(scope="module")
def world(omni, ctx, tmp_path_factory):
    from omni_swarm_amd import flatten, weights
    c = omni.capi
    sp_w, vw = S.synth_weights(0), V.synth_weights()
    comp, mean = synth.pca()
    files = weights.write_pipeline_files(str(tmp_path_factory.mktemp("e2e_fisheye_raw")), sp_w, comp, mean, vw, V.layer_specs(), c.VLAD_KINDS)
    m = mei(SRC_W, SRC_H)
    hi = [flatten.generate_undist_maps(m, VW * UPSCALE, FOV, cam_id) for cam_id in (0, 1)]
    assert all(v.shape == (VH * UPSCALE, VW * UPSCALE, 2) for h in hi for v in h[1:])
    places = []                                                               # per place: [(file, pixels) of the up frame, of the down frame]
    for p in range(N_PLACES):
        up = synth.image_u8(7600 + p, SRC_H, SRC_W, n_shapes=N_SHAPES)
        pair = [coded(c, up, QUALITY), coded(c, down_frame(up, hi[0], hi[1]), QUALITY)]
        assert all(len(f) <= SRC_W * SRC_H // 2 for f, _ in pair)
        places.append(pair)
    plan = schedule()
    # mode (i)'s input: the four side views of both cameras, made by the existing flatten object from the host-decoded frames
    fl = [c.Flatten(ctx, SRC_W, SRC_H, flatten.generate_undist_maps(m, VW, FOV, cam_id)) for cam_id in (0, 1)]
    try:
        views = [[fl[cam](places[p][cam][1][None])[0][1:5] for cam in range(2)] for p in range(N_PLACES)]      # [place][cam][dir]
    finally:
        for f in fl:
            f.close()
    return {"files": files, "places": places, "views": views, "plan": plan, "poses": np.array([np.concatenate([q[1][0], q[1][1]]) for q in plan]),
            "raw_fisheye": dict(src_width=SRC_W, src_height=SRC_H, fov_deg=FOV, mei_up=m, mei_down=m)}


def make(omni, world, microbatch, **kw):
    from omni_swarm_amd import pipeline
    c, files = omni.capi, world["files"]
    return pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], VW, VH, THR, MAXN, c.PREC_F16, microbatch, 2, c.STORE_F32, 1,
                                     PARAMS["inner_product_thres"], PARAMS["init_mode_product_thres"], PARAMS["match_index_dist"], PARAMS["min_loop_num"],
                                     PARAMS["min_direction_loop"], geometry=True, **kw)


def outcome(pl, hits):
    return {"hits": hits, "cand": pl.candidates(), "edges": pl.edges(), "stats": pl.geometry_stats(), "rows": pl.db_rows, "corrupt": pl.jpeg_corrupt()}


def same_outcome(a, b):
    assert a["rows"] == b["rows"] == DIRS * N_KF and a["hits"] == b["hits"] and np.array_equal(a["cand"], b["cand"]) and a["stats"] == b["stats"]
    assert a["edges"].shape == b["edges"].shape and np.array_equal(a["edges"].view(np.uint8), b["edges"].view(np.uint8))      # every field of every LoopEdge, bit for bit
    assert a["corrupt"] == b["corrupt"] == 0


def blocks(ctx, world, mode, MB):
    """run()'s pinned blocks of MB key frames: (i) [up views, 4 per key frame | down views], (ii) [up frames | down frames]"""
    pins = []
    for s in range(0, N_KF, MB):
        kfs = [world["plan"][i][0] for i in range(s, min(s + MB, N_KF))]
        if mode == "views":
            blk = np.stack([world["views"][p][cam][d] for cam in range(2) for p in kfs for d in range(DIRS)])
        else:
            blk = np.stack([world["places"][p][cam][1] for cam in range(2) for p in kfs])
        a = ctx.host_alloc(blk.shape, np.uint8)
        a[:] = blk
        pins.append(a)
    return pins


def run_three(omni, ctx, world, MB):
    c = omni.capi
    out = {}
    for mode in ("views", "pixels"):
        pins = blocks(ctx, world, mode, MB)
        pl = make(omni, world, MB, **({} if mode == "views" else dict(raw_fisheye=world["raw_fisheye"])))
        try:
            assert pl.fisheye_raw() == ((0, 0) if mode == "views" else (SRC_W, SRC_H)) and pl.compressed_images() == (False, False)
            pl.set_poses(0, world["poses"])
            full = N_KF // MB
            hits = pl.run(N_KF, 0, [p.ctypes.data for p in pins[:full]], 0, pins[full].ctypes.data if N_KF % MB else None, True)
            out[mode] = outcome(pl, hits)
            if mode == "pixels":
                with pytest.raises(c.OmniError, match="raw-fisheye mode"):
                    pl.attach_shard(0, 1, c.shard_unique_id())
                with pytest.raises(c.OmniError, match="compressed_images is off"):
                    pl.run_jpeg([[f for f, _ in world["places"][0]]], 100)
        finally:
            pl.close()
            for p in pins:
                ctx.host_free(p)
    pl = make(omni, world, MB, raw_fisheye=world["raw_fisheye"], compressed_images=True)
    try:
        assert pl.compressed_images() == (True, True)
        pl.set_poses(0, world["poses"])
        out["files"] = outcome(pl, pl.run_jpeg([[f for f, _ in world["places"][p]] for p, _ in world["plan"]], 0))
    finally:
        pl.close()
    return out


def stream_three(omni, world, MB):
    out = {}
    for mode in ("views", "pixels", "files"):
        pl = make(omni, world, MB, **({} if mode == "views" else dict(raw_fisheye=world["raw_fisheye"], compressed_images=mode == "files")))
        try:
            pl.set_latency(-1.0, False)                                        # units leave when they are full (and at flush): the same cut in all three, whatever the timing
            hits = 0
            for i, (p, _) in enumerate(world["plan"]):
                if mode == "views":
                    hits += pl.push_keyframe([world["views"][p][cam][d] for cam in range(2) for d in range(DIRS)], i, float(i), world["poses"][i], False)
                elif mode == "pixels":
                    hits += pl.push_keyframe([world["places"][p][cam][1] for cam in range(2)], i, float(i), world["poses"][i], False)
                else:
                    hits += pl.push_keyframe_jpeg([world["places"][p][cam][0] for cam in range(2)], i, float(i), world["poses"][i], False)
            hits += pl.flush()
            out[mode] = outcome(pl, hits)
        finally:
            pl.close()
    return out


def report(name, out):
    ref = out["views"]
    print(f"{name}: {ref['rows']} rows, {ref['hits']} hits, {len(ref['cand'])} candidates, {len(ref['edges'])} edges (geometry calls, edges) {ref['stats']} in mode (i); "
          f"(ii) {out['pixels']['hits']} hits / {len(out['pixels']['edges'])} edges, (iii) {out['files']['hits']} hits / {len(out['files']['edges'])} edges; "
          f"inliers {ref['edges'][:, 4].astype(int).tolist()}")


def check(world, out):
    ref = out["views"]
    assert len(ref["cand"]) >= 3                                                                # the condition: the stream gives mode (i) its revisits
    revisit_of = {i: world["plan"][i][0] for i in range(N_PLACES, N_KF)}
    assert {(int(a), int(b)) for a, b in ref["cand"][:, :2]} >= set(revisit_of.items())         # every revisit finds its first visit
    same_outcome(out["pixels"], ref)
    same_outcome(out["files"], ref)


def test_run_three_modes_agree(omni, ctx, world):
    out = run_three(omni, ctx, world, 4)
    report("run(), units of 4", out)
    check(world, out)


def test_push_keyframe_three_modes_agree(omni, world):
    """the streaming intake, units of 3 and a last one of 2"""
    out = stream_three(omni, world, 3)
    report("push_keyframe + flush, units of 3", out)
    check(world, out)


def test_a_truncated_fisheye_file_is_counted_and_pixels_are_refused(omni, world):
    c = omni.capi
    pl = make(omni, world, 2, raw_fisheye=world["raw_fisheye"], compressed_images=True)
    try:
        up, down = (f for f, _ in world["places"][0])
        with pytest.raises(c.OmniError, match="JPEG files|no sizes|stride"):
            pl.push_keyframe([world["places"][0][cam][1] for cam in range(2)], 0, 0.0, None, False)      # pixels for a pipeline that takes files
        pl.push_keyframe_jpeg([up, down[:len(down) // 2]], 0, 0.0, None, False)
        pl.flush()
        assert pl.jpeg_corrupt() == 1 and pl.db_rows == DIRS
    finally:
        pl.close()
