"""End to end in CameraConfig::STEREO_PINHOLE (loop_defines.h:110-115; generate_stereo_image_descriptor for ONE direction, loop_cam.cpp:189-196): raw left / right
frames of the camera's size -> resized to the networks' size INSIDE the key-frame unit (csrc/resize.hip; the cv::resize of superpoint_tensorrt.cpp:123-125) ->
SuperPoint on both, MobileNetVLAD on the left image, no rows blanked -> left / right matching -> triangulation with the rig's two extrinsics -> database / query
rule on direction 0 (loop_detector.cpp:252-258) -> compute_correspond_features with MAX_DIRS = 1 -> homography mask -> PnP -> LoopEdge, through the C++ key-frame
pipeline on the GPU against the oracle chain on the frames resized by the numpy restatement of the resize (tests/resize_ref.py) and against the scene's ground truth.

Scene: direction 0 of omni_swarm_amd.synth.room_keyframe rendered at 750 x 600 -- view 0 (the up camera) is the left camera, view 4 (the down camera) the right
one, 10 cm apart, extrinsics those of tests/test_gpu_e2e_scene.extrinsic(0, up), given through set_stereo_extrinsics.  The networks run at 600 x 480 (a resize
by 0.8 on both axes: the linear mode), so the model of the network-size image is fx = fy = 300, cx = 300, cy = 240 and the wall's 16 rows of disparity become 12.8.
8 places, each visited twice; 16 key frames go through run() in micro-batches of 4 and again, one at a time, through push_keyframe + flush() in micro-batches of 3.

Pre-check (the oracle chain alone, on the CPU): one direction of this scene gives the oracle 8 edges for its 8 revisits (79 .. 109 inliers each, relative
poses within 3 cm of identity) with min_loop_num = 30 -- nothing about the scene or the thresholds had to change.

The bounds are those of tests/test_gpu_e2e_scene.py and tests/test_gpu_e2e_depth.py, for the reasons given there: OMNI_PREC_SPLIT has the fp32 graph's key points,
so the discrete decisions downstream are the oracle's except where one sits within fp32 rounding of its threshold -- at most 2 of an edge's correspondences may
differ, and the pose, a least-squares refit over all inliers, then agrees to 1e-4 instead of 1e-6."""
import math

import numpy as np
import pytest

from oracle import geometry_ref as G
from oracle import match_ref as M
from oracle import mobilenetvlad_ref as V
from oracle import postproc_ref as P
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import resize_ref as R
from tests.test_gpu_e2e_scene import extrinsic

pytestmark = pytest.mark.gpu
SRC_W, SRC_H, W, H, THR, MAXN = 750, 600, 600, 480, 0.02, 200
FX = FY = 300.0
CX, CY = 300.0, 240.0
TRIANGLE_THRES, ACCEPT_MIN = 0.006, 50
N_PLACES = 8
PARAMS = dict(inner_product_thres=0.3, init_mode_product_thres=0.2, match_index_dist=3, min_loop_num=30, min_direction_loop=1)
EXT_L, EXT_R = extrinsic(0, True), extrinsic(0, False)
STEREO = dict(fx=FX, fy=FY, cx=CX, cy=CY, src_width=SRC_W, src_height=SRC_H, triangle_thres=TRIANGLE_THRES, accept_min_3d_pts=ACCEPT_MIN)


def schedule():
    """key frame i -> (place, revisit, noise sigma, reported odometry pose).  Second visits come in another order than the first ones, with a drifted pose."""
    out = []
    for p in range(N_PLACES):
        out.append((p, 0, 0.0, G.pose([6.0 * p, 1.5 * (p % 3), 1.0], G.q_from_yaw(0.05 * p))))
    for i in range(N_PLACES):
        p = (3 * i + 2) % N_PLACES
        true = out[p][3]
        drift = G.pose(true[0] + np.array([0.25, -0.15, 0.04]), G.qmul(G.q_from_yaw(0.015), true[1]))
        out.append((p, 1, 0.0 if i % 2 == 0 else 1.5, drift))
    return out


def raw_frames(plan):
    """[(left, right)] at the camera's size: views 0 and 4 of the room's key frame"""
    out = []
    for (p, rv, sg, _) in plan:
        kf = synth.room_keyframe(p, SRC_H, SRC_W, rv, sg)
        out.append((kf[0].copy(), kf[4].copy()))
    return out


def oracle_frame(sp_w, vw, comp, mean, left, right, msg_id, pose):
    """One key frame through the oracle chain on the RESIZED pair, as a geometry_ref frame dict (+ the global descriptor of the left image)."""
    imgs = np.stack([left, right])
    semi, desc = S.forward(sp_w, S.preprocess_u8(imgs, False))
    per = []
    for b in range(2):
        xy, _, _, _ = P.get_keypoints(semi[b], THR, MAXN)
        d64, _ = P.compute_descriptors(desc[b], xy, W, H, comp, mean)
        per.append((xy.astype(np.float64), d64))
    g = V.forward(vw, imgs[:1])
    (xl, dl), (xr, dr) = per
    lift64 = lambda x: np.stack([((x[:, 0] - CX) / FX), ((x[:, 1] - CY) / FY)], 1)     # the triangulation lifts the pixels again, in double (loop_cam.cpp:403-407)
    qi, ti, _ = M.bf_match(dl, dr, 0)
    l3, fl = np.zeros((len(xl), 3)), np.zeros(len(xl), np.uint8)
    if len(xl) > ACCEPT_MIN:                                                           # loop_cam.cpp:385
        _, l3, fl, _, _ = G.stereo_landmarks(pose, EXT_L, EXT_R, lift64(xl), lift64(xr), qi, ti, TRIANGLE_THRES)
    img = {"landmark_num": len(xl), "landmarks_2d": xl, "landmarks_2d_norm": lift64(xl).astype(np.float32).astype(np.float64), "feature_descriptor": dl,
           "camera_extrinsic": EXT_L, "landmarks_3d": l3.astype(np.float32).astype(np.float64), "landmarks_flag": fl}
    return {"msg_id": msg_id, "drone_id": 1, "timestamp": float(msg_id), "pose_drone": pose, "images": [img], "landmark_num": len(xl)}, g


def oracle_chain(sp_w, vw, comp, mean, plan, resized):
    """-> (candidates [n][4], edges [(old, new, result)], database size)"""
    geo, ref_edges = {}, []
    bf = lambda a, b: M.bf_match(a, b, 0)

    def compute_loop(new, old, dn, do, init_mode):
        r = G.compute_loop(geo[new.msg_id], geo[old.msg_id], dn, do, init_mode, bf, is_4dof=True, min_loop_num=PARAMS["min_loop_num"], init_min=10,
                           max_dirs=1, min_direction_loop=1)
        if r is not None:
            ref_edges.append((old.msg_id, new.msg_id, r))
        return r is not None

    det = M.LoopDetectorRef(1, compute_loop=compute_loop, camera_configuration=M.STEREO_PINHOLE, **PARAMS)
    for i, (p, rv, sg, pose) in enumerate(plan):
        geo[i], g = oracle_frame(sp_w, vw, comp, mean, resized[i][0], resized[i][1], i, pose)
        det.on_image_recv(M.FisheyeFrameDesc(msg_id=i, drone_id=1, landmark_num=geo[i]["landmark_num"], prevent_adding_db=False,
                                             images=[M.ImageDesc(drone_id=1, landmark_num=geo[i]["images"][0]["landmark_num"], image_desc=g[0])]))
    cand = np.array([[r["msg_id"], r["old_msg_id"], r["dir_new"], r["dir_old"]] for r in det.log if r["old_msg_id"] != -1], np.int64).reshape(-1, 4)
    return cand, ref_edges, det.database_size()


@pytest.fixture(scope="module")
def world(omni, tmp_path_factory):
    from omni_swarm_amd import weights
    sp_w, vw = S.synth_weights(0), V.synth_weights()
    comp, mean = synth.pca()
    files = weights.write_pipeline_files(str(tmp_path_factory.mktemp("stereo_pinhole")), sp_w, comp, mean, vw, V.layer_specs(), omni.capi.VLAD_KINDS)
    plan = schedule()
    raw = raw_frames(plan)
    return {"weights": (sp_w, vw, comp, mean), "files": files, "plan": plan, "raw": raw, "poses": np.array([np.concatenate([q[3][0], q[3][1]]) for q in plan])}


def make_pipeline(omni, world, microbatch, **kw):
    from omni_swarm_amd import pipeline
    c, files = omni.capi, world["files"]
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, THR, MAXN, c.PREC_SPLIT, microbatch, 2, c.STORE_F32, 1,
                                   PARAMS["inner_product_thres"], PARAMS["init_mode_product_thres"], PARAMS["match_index_dist"], PARAMS["min_loop_num"],
                                   PARAMS["min_direction_loop"], geometry=True, **kw)
    return pl


@pytest.fixture(scope="module")
def product(omni, ctx, world):
    """the 16 key frames through run() in micro-batches of 4: (hits, candidates, edges, geometry stats, rows)"""
    MB, raw, n = 4, world["raw"], len(world["plan"])
    pins = []
    for s in range(0, n, MB):
        p = ctx.host_alloc((2 * MB, SRC_H, SRC_W), np.uint8)                    # the micro-batch's left frames, then its right frames, at the camera's size
        p[:] = np.stack([raw[s + m][0] for m in range(MB)] + [raw[s + m][1] for m in range(MB)])
        pins.append(p)
    pl = make_pipeline(omni, world, MB, stereo_pinhole=STEREO)
    try:
        pl.set_stereo_extrinsics(np.concatenate(EXT_L), np.concatenate(EXT_R))
        pl.set_poses(0, world["poses"])
        hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
        out = {"hits": hits, "cand": pl.candidates(), "edges": pl.edges(), "stats": pl.geometry_stats(), "rows": pl.db_rows}
        with pytest.raises(omni.capi.OmniError, match="after the first key frame"):
            pl.set_stereo_extrinsics(np.concatenate(EXT_L), np.concatenate(EXT_R))
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)
    return out


def test_run_equals_the_streaming_intake_and_a_recut_run(omni, ctx, world, product):
    """the same key frames one at a time through push_keyframe (micro-batches of 3: five full units and one of 1): the same hits, candidates and edges; and
    run() on 6 key frames with a micro-batch of 4 -- not a whole number of micro-batches: 3 + 3 from blocks of 4 + 2 through omni_cam_enqueue_raw_host_parts, or
    the blocks' own cut -- finds what the first 6 key frames of the long run found"""
    raw, plan = world["raw"], world["plan"]
    ps = make_pipeline(omni, world, 3, stereo_pinhole=STEREO)
    try:
        ps.set_stereo_extrinsics(np.concatenate(EXT_L), np.concatenate(EXT_R))
        hits_s = 0
        for i, (left, right) in enumerate(raw):
            hits_s += ps.push_keyframe([left, right], i, float(i), world["poses"][i], False)
        hits_s += ps.flush()
        cand_s, edges_s, rows_s = ps.candidates(), ps.edges(), ps.db_rows
    finally:
        ps.close()
    cand, edges = product["cand"], product["edges"]
    assert rows_s == product["rows"] and hits_s == product["hits"] and np.array_equal(cand_s, cand)
    assert np.array_equal(edges_s[:, :5], edges[:, :5]) and np.abs(edges_s[:, 5:] - edges[:, 5:]).max(initial=0) < 1e-9
    # 10 key frames, the revisits of places 2 and 5 among them, as blocks of 4 + 4 + a tail of 2
    n = 10
    blocks = []
    for s, m in ((0, 4), (4, 4), (8, 2)):
        p = ctx.host_alloc((2 * m, SRC_H, SRC_W), np.uint8)
        p[:] = np.stack([raw[s + k][0] for k in range(m)] + [raw[s + k][1] for k in range(m)])
        blocks.append(p)
    pr = make_pipeline(omni, world, 4, stereo_pinhole=STEREO)
    try:
        pr.set_stereo_extrinsics(np.concatenate(EXT_L), np.concatenate(EXT_R))
        pr.set_poses(0, world["poses"])
        hits_r = pr.run(n, 0, [blocks[0].ctypes.data, blocks[1].ctypes.data], 0, blocks[2].ctypes.data, True)
        cand_r, edges_r, rows_r = pr.candidates(), pr.edges(), pr.db_rows
    finally:
        pr.close()
        for p in blocks:
            ctx.host_free(p)
    first = cand[cand[:, 0] < n]
    e_first = edges[edges[:, 1] < n]
    assert rows_r == n and hits_r == len(first) >= 2 and np.array_equal(cand_r, first)
    assert np.array_equal(edges_r[:, :5], e_first[:, :5]) and np.abs(edges_r[:, 5:] - e_first[:, 5:]).max(initial=0) < 1e-9 and len(e_first) >= 1


def test_stereo_pinhole_frames_to_loop_edges_equal_the_oracle_chain_and_the_ground_truth(omni, world, product):
    sp_w, vw, comp, mean = world["weights"]
    plan = world["plan"]
    n = len(plan)
    resized = [(R.resize(l, W, H), R.resize(r, W, H)) for l, r in world["raw"]]
    ref_cand, ref_edges, ref_rows = oracle_chain(sp_w, vw, comp, mean, plan, resized)
    hits, cand, edges, (calls, n_edges), rows = product["hits"], product["cand"], product["edges"], product["stats"], product["rows"]
    assert rows == ref_rows == n                                              # one row per key frame
    assert hits == len(cand) and np.array_equal(cand, ref_cand), (cand, ref_cand)
    assert (cand[:, 2:] == 0).all()                                           # direction 0 on both sides
    revisit_of = {i: plan[i][0] for i in range(N_PLACES, n)}
    assert {(int(a), int(b)) for a, b in cand[:, :2]} >= {(i, p) for i, p in revisit_of.items()}          # every revisit finds its first visit
    assert calls == len(cand)
    got_list = [(int(e[0]), int(e[1]), int(e[4])) for e in edges]
    ref_list = [(a, b, r["inliers"]) for a, b, r in ref_edges]
    print("product edges (old, new, inliers):", got_list)
    print("oracle  edges (old, new, inliers):", ref_list)
    assert n_edges == len(edges) == len(ref_edges) >= N_PLACES - 1, (got_list, ref_list, cand.tolist())
    n_exact = 0
    for e, (old_id, new_id, r) in zip(edges, ref_edges):
        assert (int(e[0]), int(e[1]), int(e[2]), int(e[3])) == (old_id, new_id, 1, 1)
        assert abs(int(e[4]) - r["inliers"]) <= 2, (int(e[4]), r["inliers"])
        n_exact += int(e[4]) == r["inliers"]
        tol = 1e-6 if int(e[4]) == r["inliers"] else 1e-4
        pos, att = r["relative_pose"]
        assert np.abs(e[5:8] - pos).max() < tol, (e[5:8], pos)
        assert min(np.abs(e[8:12] - att).max(), np.abs(e[8:12] + att).max()) < tol
        assert revisit_of.get(new_id) == old_id
        assert np.linalg.norm(e[5:8]) < 0.10 and abs(G.wrap_angle(G.quat2eulers(e[8:12])[2])) < math.radians(1.0), e      # ground truth: the same physical pose
    assert n_exact >= len(edges) - 2, (n_exact, len(edges))


def test_frames_of_the_networks_size_need_no_resize_object(omni, world):
    """src_width = src_height = 0: the existing upload path; a frame of another size is then a stride error at the intake, not a silent misread"""
    pl = make_pipeline(omni, world, 2, stereo_pinhole=dict(fx=FX, fy=FY, cx=CX, cy=CY))
    try:
        small = [R.resize(f, W, H) for f in world["raw"][0]]
        assert pl.push_keyframe(small, 0, 0.0, world["poses"][0], False) == 0
        pl.flush()
        assert pl.db_rows == 1
        with pytest.raises(omni.capi.OmniError, match="stride"):
            pl.push_keyframe([f[:, :W - 8] for f in small], 1, 1.0, world["poses"][1], False)
    finally:
        pl.close()


def test_camera_configuration_3_is_still_refused(omni, world):
    """there are three camera configurations (loop_defines.h:110-115): a launch file that names a fourth is refused with a message, and so is a source size on a
    configuration that does not resize"""
    import os
    from omni_swarm_amd import pipeline
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "launch", "nodelet-sfisheye.launch")
    assert os.path.exists(path), "make -C oracle ref"
    xml = open(path).read()
    assert "camera_configuration: 1" in xml
    files = world["files"]
    with pytest.raises(omni.capi.OmniError, match="camera_configuration 3"):
        pipeline.KeyframePipeline.from_launch(0, xml.replace("camera_configuration: 1", "camera_configuration: 3"), files["sp"], files["vlad"], files["comp"], files["mean"])
    with pytest.raises(omni.capi.OmniError, match="both or neither"):
        make_pipeline(omni, world, 2, stereo_pinhole=dict(fx=FX, fy=FY, cx=CX, cy=CY, src_width=SRC_W))
