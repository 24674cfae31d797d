"""End to end with is_compressed_images (KeyframePipeline::Config::compressed_images): the STEREO_PINHOLE scene of tests/test_gpu_e2e_stereo_pinhole.py and the
PINHOLE_DEPTH scene of tests/test_gpu_e2e_depth.py, every frame encoded at test time with the project's own omni_jpeg_encode_host, through the C++ key-frame
pipeline twice: once as RAW frames that are the host decode of those files (omni_jpeg_decode_host, the g++ build of csrc/jpeg_dec_plan.h) through the existing
run(), and once as the FILES with the switch on -- run_jpeg (units of 4) and push_keyframe_jpeg + flush (units of 3; the decode kernels inside every unit, in front
of the resize).  Both sides run the same network kernels on the same bytes: database rows, hits, candidates and LoopEdges are identical (every LoopEdge field of
the two run() sides bit for bit).  The key-frame messages themselves are not readable from Python; tests/test_gpu_cam_jpegdec.py holds every field of a unit's
result bit-identical, and every LoopEdge here is computed from those fields.  A frame that cannot be decoded counts in jpeg_corrupt(); STEREO_FISHEYE ignores the
switch.  With the switch off nothing changes: the existing end-to-end tests run that side against the oracle chain, unchanged."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import test_gpu_e2e_depth as D
from tests import test_gpu_e2e_stereo_pinhole as SP

pytestmark = pytest.mark.gpu
QUALITY = 90


@pytest.fixture(scope="module")
def files(omni, tmp_path_factory):
    from omni_swarm_amd import weights
    sp_w, vw = S.synth_weights(0), V.synth_weights()
    comp, mean = synth.pca()
    return weights.write_pipeline_files(str(tmp_path_factory.mktemp("e2e_jpegdec")), sp_w, comp, mean, vw, V.layer_specs(), omni.capi.VLAD_KINDS)


def encode_decode(c, gray):
    """-> (the file, its host decode)"""
    st, data = c.jpeg_encode_host(np.ascontiguousarray(gray), QUALITY)
    assert st == c.JPEG_OK and len(data) <= gray.size // 2                      # within the unit decoder's capacity: the kernels decode it
    st, pix = c.jpeg_decode_host(data)
    assert st == c.JPEGDEC_OK and pix.shape == gray.shape
    return data, pix


def make(omni, files, params, W, H, thr, maxn, microbatch, **kw):
    from omni_swarm_amd import pipeline
    c = omni.capi
    return pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], W, H, thr, maxn, c.PREC_SPLIT, microbatch, 2, c.STORE_F32, 1,
                                     params["inner_product_thres"], params["init_mode_product_thres"], params["match_index_dist"], params["min_loop_num"],
                                     params["min_direction_loop"], geometry=True, **kw)


def outcome(pl, hits):
    return {"hits": hits, "cand": pl.candidates(), "edges": pl.edges(), "stats": pl.geometry_stats(), "rows": pl.db_rows}


def same_outcome(a, b, exact):
    assert a["rows"] == b["rows"] and a["hits"] == b["hits"] and np.array_equal(a["cand"], b["cand"]) and a["stats"] == b["stats"]
    assert a["edges"].shape == b["edges"].shape and np.array_equal(a["edges"][:, :5], b["edges"][:, :5])
    if exact:
        assert np.array_equal(a["edges"].view(np.uint8), b["edges"].view(np.uint8))
    else:                                                                       # (another cut into units: the bound the existing run-against-stream tests use)
        assert np.abs(a["edges"][:, 5:] - b["edges"][:, 5:]).max(initial=0) < 1e-9


def test_stereo_pinhole_files_equal_the_host_decoded_raw_frames(omni, ctx, files):
    c = omni.capi
    plan = SP.schedule()
    n, MB = len(plan), 4
    poses = np.array([np.concatenate([q[3][0], q[3][1]]) for q in plan])
    pairs = [[encode_decode(c, g) for g in lr] for lr in SP.raw_frames(plan)]                   # [kf][cam] -> (file, pixels)
    ext = (np.concatenate(SP.EXT_L), np.concatenate(SP.EXT_R))
    pins = []
    for s in range(0, n, MB):
        p = ctx.host_alloc((2 * MB, SP.SRC_H, SP.SRC_W), np.uint8)
        p[:] = np.stack([pairs[s + m][0][1] for m in range(MB)] + [pairs[s + m][1][1] for m in range(MB)])
        pins.append(p)
    raw = make(omni, files, SP.PARAMS, SP.W, SP.H, SP.THR, SP.MAXN, MB, stereo_pinhole=SP.STEREO)
    try:
        assert raw.compressed_images() == (False, False)
        raw.set_stereo_extrinsics(*ext)
        raw.set_poses(0, poses)
        ref = outcome(raw, raw.run(n, 0, [p.ctypes.data for p in pins], 0, None, True))
        assert raw.jpeg_corrupt() == 0
        with pytest.raises(c.OmniError, match="compressed_images is off"):
            raw.run_jpeg([[pairs[0][0][0], pairs[0][1][0]]], 100)
        with pytest.raises(c.OmniError, match="after the first key frame"):
            raw.set_compressed_images(True)
    finally:
        raw.close()
        for p in pins:
            ctx.host_free(p)
    kfs = [[pairs[i][0][0], pairs[i][1][0]] for i in range(n)]
    jr = make(omni, files, SP.PARAMS, SP.W, SP.H, SP.THR, SP.MAXN, MB, stereo_pinhole=SP.STEREO, compressed_images=True)
    try:
        assert jr.compressed_images() == (True, True)
        jr.set_stereo_extrinsics(*ext)
        jr.set_poses(0, poses)
        got = outcome(jr, jr.run_jpeg(kfs, 0))
        assert jr.jpeg_corrupt() == 0
    finally:
        jr.close()
    print(f"STEREO_PINHOLE: {ref['rows']} rows, {ref['hits']} hits, {len(ref['edges'])} edges on both sides")
    assert len(ref["cand"]) >= SP.N_PLACES and len(ref["edges"]) >= SP.N_PLACES - 1             # not vacuous
    same_outcome(got, ref, exact=True)
    js = make(omni, files, SP.PARAMS, SP.W, SP.H, SP.THR, SP.MAXN, 3, stereo_pinhole=SP.STEREO)
    try:
        js.set_compressed_images(True)
        js.set_stereo_extrinsics(*ext)
        hits = 0
        for i, kf in enumerate(kfs):
            hits += js.push_keyframe_jpeg(kf, i, float(i), poses[i], False)
        hits += js.flush()
        stream = outcome(js, hits)
        with pytest.raises(c.OmniError, match="JPEG files|no sizes|stride"):
            js.push_keyframe([pairs[0][0][1], pairs[0][1][1]], 50, 50.0, poses[0], False)       # pixels for a pipeline that takes files
        # a right frame that ends inside its scan: the unit runs, the frame is all zeros and is counted
        assert js.jpeg_corrupt() == 0
        js.push_keyframe_jpeg([kfs[0][0], kfs[0][1][:len(kfs[0][1]) // 2]], n, float(n), poses[0], False)
        js.flush()
        assert js.jpeg_corrupt() == 1
    finally:
        js.close()
    same_outcome(stream, ref, exact=False)


def test_pinhole_depth_files_equal_the_host_decoded_gray_images(omni, ctx, files):
    c = omni.capi
    plan = D.schedule()
    n, MB = len(plan), D.MB
    poses = np.array([np.concatenate([q[3][0], q[3][1]]) for q in plan])
    frames = [synth.depth_keyframe(p, D.H, D.W, rv, sg) for (p, rv, sg, _) in plan]
    coded = [encode_decode(c, f[0]) for f in frames]
    depth = np.stack([f[1] for f in frames])
    kw = dict(pinhole_depth=dict(fx=D.FX, fy=D.FY, cx=D.CX, cy=D.CY, depth_near=D.NEAR, depth_far=D.FAR, accept_min_3d_pts=D.ACCEPT_MIN))
    pins = []
    for s in range(0, n, MB):
        p = ctx.host_alloc((MB, D.H, D.W), np.uint8)
        p[:] = np.stack([coded[s + m][1] for m in range(MB)])
        pins.append(p)
    raw = make(omni, files, D.PARAMS, D.W, D.H, D.THR, D.MAXN, MB, **kw)
    try:
        raw.set_poses(0, poses)
        raw.set_depth(0, depth)
        ref = outcome(raw, raw.run(n, 0, [p.ctypes.data for p in pins], 0, None, True))
    finally:
        raw.close()
        for p in pins:
            ctx.host_free(p)
    jr = make(omni, files, D.PARAMS, D.W, D.H, D.THR, D.MAXN, MB, compressed_images=True, **kw)
    try:
        assert jr.compressed_images() == (True, True)
        jr.set_poses(0, poses)
        jr.set_depth(0, depth)
        got = outcome(jr, jr.run_jpeg([[f] for f, _ in coded], 0))
        assert jr.jpeg_corrupt() == 0
    finally:
        jr.close()
    print(f"PINHOLE_DEPTH: {ref['rows']} rows, {ref['hits']} hits, {len(ref['edges'])} edges on both sides")
    assert len(ref["cand"]) >= D.N_PLACES and len(ref["edges"]) >= D.N_PLACES - 1
    same_outcome(got, ref, exact=True)
    js = make(omni, files, D.PARAMS, D.W, D.H, D.THR, D.MAXN, 3, compressed_images=True, **kw)
    try:
        hits = 0
        for i, (f, _) in enumerate(coded):
            hits += js.push_keyframe_jpeg([f], i, float(i), poses[i], False, depth=frames[i][1])
        hits += js.flush()
        stream = outcome(js, hits)
    finally:
        js.close()
    same_outcome(stream, ref, exact=False)


def test_stereo_fisheye_ignores_the_switch_and_the_settings_file_sets_it(omni, files):
    """the reference has no compressed path for STEREO_FISHEYE: the switch is kept as set and not applied -- the pipeline goes on taking pixels"""
    from omni_swarm_amd import pipeline
    c = omni.capi
    assert pipeline.vins_is_compressed_images("%YAML:1.0\n# cameras\nnum_of_cam: 2\nis_compressed_images: 1\n") is True
    assert pipeline.vins_is_compressed_images("%YAML:1.0\nis_compressed_images: 0\n") is False and pipeline.vins_is_compressed_images("num_of_cam: 2\n") is False
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], 128, 96, 0.015, 100, c.PREC_F16, 2, 2, c.STORE_F32, 1, 0.3, 0.2, 5, 10, 3)
    try:
        pl.apply_vins_settings("is_compressed_images: 1\n")
        assert pl.compressed_images() == (True, False)
        imgs = [synth.image_u8(9900 + i, 96, 128, n_shapes=60) for i in range(8)]
        pl.push_keyframe(imgs, 0, 0.0, None, False)
        pl.flush()
        assert pl.db_rows == 4 and pl.jpeg_corrupt() == 0
    finally:
        pl.close()
