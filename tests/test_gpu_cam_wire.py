"""The LoopNet wire inside the key-frame unit (omni_cam_set_wire / omni_cam_set_wire_meta / omni_cam_wire: csrc/wire_pack.hip on the unit's SuperPoint stream behind
the landmark stage and MobileNetVLAD's rows) against the same unit with the stage off: every field of omni_cam_result and omni_cam_landmarks_result bit-identical,
and the packed buffers and tables equal to omni_wire_pack_host (the g++ build of csrc/wire_plan.h) on the unit's OWN outputs.  A stereo handle (four directions,
two key frames, a stereo model: the up images are packed) and a mono handle with a depth model; networks at 128 x 96, max_num 100."""
import numpy as np
import pytest

from oracle import mobilenetvlad_ref as V
from oracle import superpoint_ref as S
from omni_swarm_amd import synth
from tests import camera_cases as CC
from tests import depth_cases as D
from tests import landmark_cases as L
from tests import wire_cases as WC

pytestmark = pytest.mark.gpu

W, H, DIRS, N_KF, N_MONO, MAX_NUM, ACCEPT_MIN = 128, 96, 4, 2, 2, 100, 3
KEYS = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")
LM_KEYS = ("norm2d", "landmarks_3d", "landmarks_flag", "count_3d")


def poses(seed, n):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-3, 3, (n, 3)), rng.standard_normal((n, 4)) * rng.uniform(0.5, 2.0, (n, 1))], 1)


def records(capi, seed, n):
    return WC.frame(capi, seed, n, 1)["meta"]


@pytest.fixture(scope="module")
def stereo(omni, ctx):
    from omni_swarm_amd import frontend
    c = omni.capi
    comp, mean = synth.pca()
    lc = frontend.LoopCam(ctx, S.synth_weights(0), comp, mean, V.synth_weights(), V.layer_specs(), (V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM), W, H, 0.015, MAX_NUM, c.PREC_F16,
                          n_dirs=DIRS * N_KF)
    unit = ctx.host_alloc((2 * DIRS * N_KF, H, W), np.uint8)
    up = np.stack([synth.image_u8(8200 + k, H, W, n_shapes=60) for k in range(DIRS * N_KF)])
    up[5] = 0                                                   # a black image (the pack stage alone covers an image without key points: tests/test_gpu_wire_pack.py)
    unit[:] = np.concatenate([up, np.roll(up, -3, axis=1)])
    rig_up, rig_down = L.rig(DIRS)
    yield {"lc": lc, "unit": unit, "model": c.stereo_model(64.0, 64.0, 63.5, 47.5, L.THRES, ACCEPT_MIN, rig_up, rig_down)}
    lc.close()
    ctx.host_free(unit)


@pytest.fixture(scope="module")
def mono(omni, ctx):
    c = omni.capi
    comp, mean = synth.pca()
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, S.synth_weights(0), comp, mean, W, H, 0.015, MAX_NUM, c.PREC_F16, N_MONO)
    vlad = c.MobileNetVLAD(vctx, V.synth_weights(), V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, W, H, N_MONO)
    cam = c.Cam(sp, vlad, N_MONO, V.OUT_DIM, mono=True)
    unit = ctx.host_alloc((N_MONO, H, W), np.uint8)
    unit[:] = np.stack([synth.image_u8(8300 + k, H, W, n_shapes=60) for k in range(N_MONO)])
    ext = np.array([0.05, -0.02, 0.1, 0.5, -0.5, 0.5, -0.5]) * 1.3
    rng = np.random.default_rng(1)
    yield {"cam": cam, "unit": unit, "model": c.depth_model(64.0, 64.0, 63.5, 47.5, D.NEAR, D.FAR, ACCEPT_MIN, W, H, ext), "camera": CC.camera(omni, "mild"),
           "depth": rng.integers(200, 12000, (N_MONO, H, W)).astype(np.uint16)}
    cam.close()
    sp.close()
    vlad.close()
    vctx.close()
    ctx.host_free(unit)


def wait(cam, with_wire):
    res = {k: v.copy() for k, v in cam.wait().items()}
    res.update({k: v.copy() for k, v in cam.landmarks().items()})
    if with_wire:
        res["packets"], res["table"] = (a.copy() for a in cam.wire())
    return res


def check_against_host(capi, got, off, meta, n_main, send_all):
    """stage on == stage off in every result field; the packed bytes == the host function on the unit's own outputs (its main images: the first n_main)"""
    assert [k for k in KEYS + LM_KEYS if not np.array_equal(got[k].view(np.uint8), off[k].view(np.uint8))] == []
    want_out, want_table = capi.wire_pack_host(got["kps_xy"][:n_main], got["n_kps"][:n_main], got["desc"][:n_main], got["norm2d"][:n_main], got["landmarks_3d"][:n_main],
                                               got["landmarks_flag"][:n_main], got["global_desc"][:n_main], meta, send_all_features=send_all)
    table, out = got["table"], got["packets"]
    print("key points:", got["n_kps"][:n_main].tolist(), "count_3d:", got["count_3d"].tolist(), "packets:", table[:, 0].tolist(), "bytes used:", table[:, 1].tolist())
    assert out.shape == want_out.shape and np.array_equal(table, want_table)
    for g in range(n_main):                                     # (bytes behind an image's last packet are nobody's)
        assert np.array_equal(out[g, :table[g, 1]], want_out[g, :table[g, 1]]), g
    return table


@pytest.mark.parametrize("send_all", [False, True])
def test_stereo_unit_packs_its_up_images(omni, ctx, stereo, send_all):
    c = omni.capi
    cam, unit, n = stereo["lc"].cam, stereo["unit"], DIRS * N_KF
    p7, meta = poses(1, N_KF), records(c, 21, n)
    cam.set_active(n)
    cam.set_stereo_model(stereo["model"])
    try:
        cam.set_wire(False)
        cam.set_poses(p7)
        cam.enqueue_host(unit, True)
        off = wait(cam, False)
        with pytest.raises(c.OmniError, match="stage off"):
            cam.wire()
        cam.set_wire(True, send_all)
        cam.set_poses(p7)
        cam.set_wire_meta(meta)
        cam.enqueue_host(unit, True)
        got = wait(cam, True)
        table = check_against_host(c, got, off, meta, n, send_all)
        flagged = [int(got["landmarks_flag"][g, :got["n_kps"][g]].sum()) for g in range(n)]
        assert sum(flagged) > 0 and (got["n_kps"][:n] > 0).sum() >= n - 1                           # not vacuous: key points and 3-D points to send
        assert [int(t) for t in table[:, 0]] == [0 if got["n_kps"][g] == 0 else 1 + (int(got["n_kps"][g]) if send_all else flagged[g]) for g in range(n)]
        for g in range(n):                                      # and the header announces the flagged ones either way
            if table[g, 0]:
                assert WC.parse_header(c.wire_packets(got["packets"][g], table[g])[0][1])["feature_num"] == flagged[g]
        # a partly filled unit: one key frame in a handle made for two
        cam.set_active(DIRS)
        small = np.ascontiguousarray(np.concatenate([unit[:DIRS], unit[n:n + DIRS]]))
        dev = ctx.to_device(small)
        try:
            cam.set_poses(p7[:1])
            cam.set_wire_meta(meta[:DIRS])
            cam.enqueue_dev(dev, W, True)
            one = wait(cam, True)
        finally:
            ctx.free(dev)
        assert one["table"].shape[0] == DIRS and one["table"][:, 0].sum() > DIRS
        check_against_host(c, one, one, meta[:DIRS], DIRS, send_all)
    finally:
        cam.set_active(n)
        cam.set_wire(False)
        cam.set_stereo_model(None)


def test_mono_unit_with_a_depth_model(omni, ctx, mono):
    c = omni.capi
    cam, unit, depth = mono["cam"], mono["unit"], mono["depth"]
    p7, meta = poses(2, N_MONO), records(c, 22, N_MONO)
    cam.set_depth_model(mono["model"], mono["camera"])
    try:
        def run(on):
            cam.set_wire(on)
            cam.set_poses(p7)
            cam.set_depth_host(list(depth))
            if on:
                cam.set_wire_meta(meta)
            cam.enqueue_host(unit, False)
            return wait(cam, on)
        off, got = run(False), run(True)
        table = check_against_host(c, got, off, meta, N_MONO, False)
        assert (got["count_3d"] > 5).all() and (table[:, 0] == 1 + got["count_3d"]).all()          # not vacuous: a packet per depth landmark
    finally:
        cam.set_wire(False)
        cam.set_depth_model(None)


def test_refusals(omni, ctx, stereo, mono):
    """each before anything is enqueued; the handle stays usable"""
    c = omni.capi
    cam, unit, n = stereo["lc"].cam, stereo["unit"], DIRS * N_KF
    meta = records(c, 23, n)
    cam.set_active(n)
    cam.set_stereo_model(None)
    with pytest.raises(c.OmniError, match="no landmark model"):                 # the stage packs landmarks the device made
        cam.set_wire(True)
    with pytest.raises(c.OmniError, match="no landmark model"):
        mono["cam"].set_wire(True)
    with pytest.raises(c.OmniError, match="stage off"):
        cam.set_wire_meta(meta)
    cam.set_stereo_model(stereo["model"])
    try:
        cam.set_wire(True)
        with pytest.raises(c.OmniError, match="images, the handle holds"):
            cam.set_wire_meta(np.concatenate([meta, meta]))
        cam.set_poses(poses(3, N_KF))
        with pytest.raises(c.OmniError, match="records are not set"):
            cam.enqueue_host(unit, True)
        cam.set_wire_meta(meta[:DIRS])                                          # four images' records for a unit of eight
        with pytest.raises(c.OmniError, match="records of 4 images for a unit of 8"):
            cam.enqueue_host(unit, True)
        with pytest.raises(c.OmniError, match="records of 4 images"):
            cam.enqueue_dev(16, W, True)                                        # (refused before the pointer is used)
        with pytest.raises(c.OmniError, match="without a pending"):             # nothing was enqueued by any of them
            cam.wait()
        cam.set_stereo_model(None)                                              # the model taken away behind the switch: refused at enqueue
        cam.set_wire_meta(meta)
        with pytest.raises(c.OmniError, match="no landmark model"):
            cam.enqueue_host(unit, True)
        cam.set_stereo_model(stereo["model"])
        cam.set_poses(poses(3, N_KF))
        cam.enqueue_host(unit, True)
        for call in (lambda: cam.set_wire(False), lambda: cam.set_wire_meta(meta), lambda: cam.wire()):
            with pytest.raises(c.OmniError, match="in flight"):
                call()
        first = wait(cam, True)
        cam.set_poses(poses(3, N_KF))
        with pytest.raises(c.OmniError, match="records are not set"):           # the records were that unit's: the next one needs its own
            cam.enqueue_host(unit, True)
        cam.set_wire_meta(meta)
        cam.enqueue_host(unit, True)                                            # and the handle still works
        again = wait(cam, True)
        assert np.array_equal(first["table"], again["table"]) and first["table"][:, 0].sum() > n
        for g in range(n):
            assert np.array_equal(first["packets"][g, :first["table"][g, 1]], again["packets"][g, :again["table"][g, 1]])
    finally:
        cam.set_wire(False)
        cam.set_stereo_model(None)
