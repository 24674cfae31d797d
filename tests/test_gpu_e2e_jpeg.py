"""The key-frame pipeline with send_img (KeyframePipeline(..., send_img=True, jpg_quality=75): csrc/jpeg.hip inside every key-frame unit) on the rendered fisheye
scene of tests/test_gpu_e2e_scene.py (STEREO_FISHEYE, 600 x 480; eight places and their revisits), through run() and through push_keyframe / flush: the main image
of every direction of every key frame in the detector's database carries the bytes the g++ build of csrc/jpeg_plan.h gives for the view that went in, with the
fisheye mask's rows (360..479) black; candidates, EVERY field of every edge, the geometry counters and the database are those of the run with the switch off; no
image was truncated; with the switch off every `image` is empty."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import test_gpu_e2e_scene as FE

pytestmark = pytest.mark.gpu
MB, QUALITY, DIRS = 4, 75, 4


@pytest.fixture(scope="module")
def files(omni, tmp_path_factory):
    from omni_swarm_amd import weights
    comp, mean = synth.pca()
    return weights.write_pipeline_files(str(tmp_path_factory.mktemp("e2e_jpeg")), S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), omni.capi.VLAD_KINDS)


@pytest.fixture(scope="module")
def scene():
    plan = FE.schedule()
    first = [q for q in plan[:FE.N_PLACES] if q[0] < 8]
    again = [q for q in plan[FE.N_PLACES:] if q[0] < 8]
    return [(synth.room_keyframe(p, FE.H, FE.W, rv, sg), np.concatenate([pose[0], pose[1]])) for (p, rv, sg, pose) in first + again]


@pytest.fixture(scope="module")
def expected(omni, scene):
    """(key frame, direction) -> the file of its up view with the mask's rows black; computed once"""
    row0 = FE.H * 3 // 4
    return {(i, d): omni.capi.jpeg_encode_host(views[d], QUALITY, zero_from_row=row0, capacity=FE.W * FE.H // 2) for i, (views, _) in enumerate(scene) for d in range(DIRS)}


def through(omni, ctx, files, scene, send_img, streaming):
    """-> ((hits, candidates, edges, geometry stats, database rows), {(key frame, direction): image}, truncated, the switch as read back)"""
    from omni_swarm_amd import pipeline
    c, P, n = omni.capi, FE.PARAMS, len(scene)
    pl = pipeline.KeyframePipeline(0, files["sp"], files["comp"], files["mean"], files["vlad"], FE.W, FE.H, FE.THR, FE.MAXN, c.PREC_F16, MB, 2, c.STORE_F32, 1,
                                   P["inner_product_thres"], P["init_mode_product_thres"], P["match_index_dist"], P["min_loop_num"], P["min_direction_loop"],
                                   geometry=True, send_img=send_img, jpg_quality=QUALITY)
    pins = []
    try:
        switch = pl.send_img()
        if streaming:
            hits = 0
            for i, (views, pose) in enumerate(scene):
                hits += pl.push_keyframe(list(views), i, float(i), pose, False)
            hits += pl.flush()
        else:
            for s in range(0, n, MB):
                kf = [scene[s + m][0] for m in range(MB)]
                p = ctx.host_alloc((2 * DIRS * MB,) + kf[0].shape[1:], np.uint8)
                p[:] = np.stack([kf[m][i] for m in range(MB) for i in range(DIRS)] + [kf[m][DIRS + i] for m in range(MB) for i in range(DIRS)])
                pins.append(p)
            pl.set_poses(0, np.array([pose for _, pose in scene]))
            hits = pl.run(n, 0, [p.ctypes.data for p in pins], 0, None, True)
        pl.sync()
        images = {}
        for i in range(n):
            for d in range(DIRS):
                try:
                    images[(i, d)] = pl.frame_image(i, d)
                except c.OmniError as e:                                        # (a key frame the detector did not keep)
                    assert "not in the database" in str(e)
        with pytest.raises(c.OmniError, match="after the first key frame"):
            pl.set_send_img(not send_img, QUALITY)
        return (hits, np.array(pl.candidates()), np.array(pl.edges()), tuple(pl.geometry_stats()), pl.db_rows), images, pl.jpeg_truncated(), switch
    finally:
        pl.close()
        for p in pins:
            ctx.host_free(p)


@pytest.mark.parametrize("streaming", [False, True], ids=["run", "push_keyframe"])
def test_send_img_fills_the_main_images_and_changes_nothing_else(omni, ctx, files, scene, expected, streaming):
    c = omni.capi
    assert len(scene) % MB == 0
    off, img_off, trunc_off, sw_off = through(omni, ctx, files, scene, False, streaming)
    on, img_on, trunc_on, sw_on = through(omni, ctx, files, scene, True, streaming)
    assert sw_off == (False, 50, False) and sw_on == (True, QUALITY, True)
    differing = sum(abs(len(v) - len(expected[k][1])) + sum(a != b for a, b in zip(v, expected[k][1])) for k, v in img_on.items())
    print(f"{'push_keyframe' if streaming else 'run'}: {len(scene)} key frames, {len(img_on)} main images in the database, {sum(map(len, img_on.values())) // max(len(img_on), 1)} bytes "
          f"per image, differing bytes {differing}, truncated {trunc_on}; hits {off[0]} / {on[0]}, candidates {len(off[1])}, edges {len(off[2])} / {len(on[2])}")
    assert len(img_on) >= DIRS * len(scene) // 2 and set(img_on) == set(img_off)                  # not vacuous
    assert all(expected[k][0] == c.JPEG_OK for k in img_on)
    assert all(v == expected[k][1] for k, v in img_on.items()) and differing == 0
    assert trunc_on == 0 and trunc_off == 0
    assert all(v == b"" for v in img_off.values())                              # the switch off: every `image` is empty
    assert len(off[1]) >= 4 and len(off[2]) >= 2                                # loop candidates and accepted edges
    assert on[0] == off[0] and on[3] == off[3] and on[4] == off[4]
    assert np.array_equal(on[1], off[1])
    assert on[2].shape == off[2].shape and np.array_equal(on[2], off[2])        # every field of every edge, bit for bit
