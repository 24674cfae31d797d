"""The key-frame unit fed RAW fisheye pairs (omni_cam_enqueue_fisheye_host / _dev: flatten_unit_kernel inside the unit) against the existing path -- capi.Flatten per
camera, numpy reordering into [up views | down views], omni_cam_enqueue_host -- and against the numpy oracle of the remap.  Rig: 1280 x 1024 frames, the MEI camera
of tests/test_flatten.py at fov 235 / width 600 (five views per camera, the four side views 600 x 312), 3 key frames in a unit created for 4.
Both paths run the same network kernels on the same bytes: every comparison is exact."""
import contextlib

import numpy as np
import pytest

from oracle import flatten_ref as F
from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth

pytestmark = pytest.mark.gpu

MEI = (1.8, -0.2, 0.05, 0.001, -0.002, 1100.0, 1098.0, 640.0, 512.0)
SRC_W, SRC_H, FOV, VW, VH, DIRS, N_KF, N_KF_CAP, MAX_NUM = 1280, 1024, 235.0, 600, 312, 4, 3, 4, 200
ROW0 = 234                                                                    # omni_fisheye_mask_rows(312): rows [234, 312) are blanked
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")


@pytest.fixture(scope="module")
def rig(omni, ctx):
    from omni_swarm_amd import flatten
    c = omni.capi
    r = {"maps": [flatten.generate_undist_maps(MEI, VW, FOV, cam_id) for cam_id in (0, 1)]}
    assert all(len(m) == 5 and m[0].shape == (VW, VW, 2) and all(v.shape == (VH, VW, 2) for v in m[1:]) for m in r["maps"])
    r["fl"] = [c.Flatten(ctx, SRC_W, SRC_H, m) for m in r["maps"]]
    r["raw"] = []
    for cam in range(2):                                                      # pinned: the source of the unit's asynchronous uploads
        a = ctx.host_alloc((N_KF + 1, SRC_H, SRC_W), np.uint8)                # (the fourth pair: a second unit for the in-flight test)
        a[:] = np.stack([synth.image_u8(7000 + 10 * cam + k, SRC_H, SRC_W, n_shapes=400) for k in range(N_KF + 1)])
        r["raw"].append(a)
    # the existing path's input block: every camera's five views per frame, of which the unit takes 1..4, up cameras first
    views = [fl(raw) for fl, raw in zip(r["fl"], r["raw"])]
    r["views"] = lambda kfs: np.stack([views[cam][k][1 + d] for cam in range(2) for k in kfs for d in range(DIRS)])
    r["weights"] = (S.synth_weights(0), synth.pca(), V.synth_weights())
    yield r
    for fl in r["fl"]:
        fl.close()
    for a in r["raw"]:
        ctx.host_free(a)


@contextlib.contextmanager
def make_cam(omni, ctx, rig, prec):
    """a unit created for 4 key frames with 3 active; closed whatever the test does (a handle that outlives its context is destroyed on a dead stream)"""
    from omni_swarm_amd import frontend
    sp_w, (comp, mean), vw = rig["weights"]
    lc = frontend.LoopCam(ctx, sp_w, comp, mean, vw, V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), VW, VH, 0.015, MAX_NUM, prec, n_dirs=N_KF_CAP * DIRS)
    try:
        lc.cam.set_active(N_KF * DIRS)
        yield lc
    finally:
        lc.close()


def wait(lc):
    return {k: v.copy() for k, v in lc.cam.wait().items()}


def same(a, b):
    return [k for k in KEYS if not np.array_equal(a[k], b[k])]


def masked(views):
    """what flatten_unit_kernel leaves of these views under the fisheye mask"""
    out = views.copy()
    out[:, ROW0:] = 0
    return out


def test_unit_input_bytes_equal_the_oracle(omni, ctx, rig):
    """omni_cam_get_input after a unit of raw pairs: [up kf x dir | down kf x dir], every remapped row the oracle's bytes, the masked rows zero."""
    c = omni.capi
    up, down = (a[:N_KF] for a in rig["raw"])
    ref = np.stack([F.remap_linear(rig["raw"][cam][k], rig["maps"][cam][1 + d]) for cam in range(2) for k in range(N_KF) for d in range(DIRS)])
    assert ref.shape == (2 * N_KF * DIRS, VH, VW) and ref[:, ROW0:].std() > 5                  # the masked rows have content to lose
    with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
        for mask in (True, False):
            lc.cam.enqueue_fisheye_host(rig["fl"][0], rig["fl"][1], up, down, 1, mask)
            with pytest.raises(c.OmniError, match="in flight"):
                lc.cam.get_input()
            lc.cam.wait()
            got = lc.cam.get_input()
            rows = ROW0 if mask else VH
            diff = int((got[:, :rows] != ref[:, :rows]).sum())
            print(f"mask {mask}: {diff} of {got[:, :rows].size} remapped bytes differ from the oracle; non-zero bytes in the masked rows: {int((got[:, rows:] != 0).sum())}")
            assert got.shape == ref.shape and diff == 0
            assert not got[:, rows:].any()
        # the same bytes as the existing kernel's
        assert np.array_equal(got, rig["views"](range(N_KF)))
        # a unit that read a caller's buffer has no input block to show
        p = ctx.to_device(got)
        try:
            lc.cam.enqueue_dev(p, VW, True)
            lc.cam.wait()
            with pytest.raises(c.OmniError, match="caller"):
                lc.cam.get_input()
        finally:
            ctx.free(p)


@pytest.mark.parametrize("prec", ["PREC_F16", "PREC_SPLIT"])
def test_results_equal_the_unit_fed_flattened_views(omni, ctx, rig, prec):
    c = omni.capi
    flat = ctx.host_alloc((2 * N_KF * DIRS, VH, VW), np.uint8)
    flat[:] = rig["views"](range(N_KF))
    try:
        with make_cam(omni, ctx, rig, getattr(c, prec)) as lc:
            lc.cam.enqueue_host(flat, True)
            ref = wait(lc)
            assert np.array_equal(lc.cam.get_input(), flat)                                     # (the flattened views as uploaded: the networks mask on their own)
            lc.cam.enqueue_fisheye_host(rig["fl"][0], rig["fl"][1], rig["raw"][0][:N_KF], rig["raw"][1][:N_KF], 1, True)
            got = wait(lc)
    finally:
        ctx.host_free(flat)
    print(prec, "key points per up view:", ref["n_kps"][:N_KF * DIRS].tolist(), "matches:", ref["n_matches"].tolist())
    assert ref["n_kps"].shape == (2 * N_KF * DIRS,) and ref["global_desc"].shape == (N_KF * DIRS, V.OUT_DIM)
    assert (ref["n_kps"][:N_KF * DIRS] >= 50).all() and ref["n_matches"].sum() > 0              # not vacuous
    assert same(got, ref) == []


def test_host_entry_equals_device_entry_and_two_units_in_flight(omni, ctx, rig):
    c = omni.capi
    fu, fd = rig["fl"]
    units = [[a[:N_KF] for a in rig["raw"]], [a[1:N_KF + 1] for a in rig["raw"]]]                # two different units of three key frames
    ctx_b = c.Context(0)                                                                        # the second handle on streams of its own, as in the key-frame pipeline
    try:
        with make_cam(omni, ctx, rig, c.PREC_F16) as a, make_cam(omni, ctx_b, rig, c.PREC_F16) as b:
            one_by_one = []
            for lc, (up, down) in zip((a, b), units):
                lc.cam.enqueue_fisheye_host(fu, fd, up, down, 1, True)
                one_by_one.append(wait(lc))
            assert same(one_by_one[0], one_by_one[1]) != []                                     # different key frames, different results
            # raw frames already in HBM
            up_dev, down_dev = ctx.to_device(units[0][0]), ctx.to_device(units[0][1])
            try:
                a.cam.enqueue_fisheye_dev(fu, fd, up_dev, down_dev, SRC_W, N_KF, 1, True)
                assert same(wait(a), one_by_one[0]) == []
                assert np.array_equal(a.cam.get_input(), masked(rig["views"](range(N_KF))))
            finally:
                ctx.free(up_dev); ctx.free(down_dev)
            # both units enqueued before either is waited for
            for lc, (up, down) in zip((a, b), units):
                lc.cam.enqueue_fisheye_host(fu, fd, up, down, 1, True)
            together = [wait(b), wait(a)][::-1]
            assert same(together[0], one_by_one[0]) == [] and same(together[1], one_by_one[1]) == []
            # the blocking call of the Python frontend: one raw pair = one key frame
            a.cam.set_active(DIRS)
            kf = a.on_fisheye_images(rig["raw"][0][0], rig["raw"][1][0], fu, fd)
            v = rig["views"]([0])
            ref = a.on_flattened_images(v[:DIRS], v[DIRS:])
            assert len(kf["images"]) == DIRS and kf["landmark_num"] == ref["landmark_num"] > 0
            for x, y in zip(kf["images"], ref["images"]):
                assert all(np.array_equal(x[k], y[k]) for k in x)
    finally:
        ctx_b.close()


def test_refusals(omni, ctx, rig):
    c = omni.capi
    fu, fd = rig["fl"]
    up, down = (a[:N_KF] for a in rig["raw"])
    with make_cam(omni, ctx, rig, c.PREC_F16) as lc:
        with pytest.raises(c.OmniError, match="key frames x 4 directions for a unit of 12"):
            lc.cam.enqueue_fisheye_host(fu, fd, up[:2], down[:2], 1, True)                      # 2 x 4 views for an active size of 12
        with pytest.raises(c.OmniError, match="key frames x 5 directions"):
            lc.cam.enqueue_fisheye_host(fu, fd, up, down, 0, True)                              # with the top view: 3 x 5
        with pytest.raises(c.OmniError, match="stride"):
            lc.cam.enqueue_fisheye_dev(fu, fd, 16, 16, SRC_W - 1, N_KF, 1, True)                # (refused before the pointers are used)
        square = c.Flatten(ctx, SRC_W, SRC_H, [rig["maps"][0][0]] * 5)                          # five 600 x 600 views
        mono = c.Cam(lc.sp, lc.vlad, N_KF * DIRS, V.OUT_DIM, mono=True)
        try:
            with pytest.raises(c.OmniError, match="600x600 but the networks were created for 600x312"):
                lc.cam.enqueue_fisheye_host(fu, square, up, down, 1, True)
            with pytest.raises(c.OmniError, match="mono"):
                mono.enqueue_fisheye_host(fu, fd, up, down, 1, True)
        finally:
            mono.close(); square.close()
        with pytest.raises(c.OmniError, match="without a pending"):                             # nothing was enqueued by any of them
            lc.cam.wait()
        lc.cam.enqueue_fisheye_host(fu, fd, up, down, 1, True)                                  # and the handle still works
        assert (wait(lc)["n_kps"][:N_KF * DIRS] >= 50).all()
