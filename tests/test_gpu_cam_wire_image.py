"""The whole descriptor inside the key-frame unit (omni_cam_set_wire_image / omni_cam_wire_image: wire_pack_image_kernel on the unit's SuperPoint stream behind
wire_pack_kernel and, with the file, behind the JPEG stage of the MobileNetVLAD stream) on the shapes of tests/test_gpu_cam_wire.py: the unit's packets equal
omni_wire_pack_image_host (the g++ build of csrc/wire_plan.h) fed the unit's OWN outputs -- omni_cam_result, omni_cam_landmarks, omni_cam_jpeg -- byte for byte; a
stereo and a mono handle; a unit whose files do not fit (tiny capacity_per_image: image_size 0); with the stage off, every field of omni_cam_result, the landmarks,
the existing wire result and the JPEG files identical to a handle that never had it; the refusals."""
import numpy as np
import pytest

from tests import wire_image_cases as IC
from tests.test_gpu_cam_wire import DIRS, H, KEYS, LM_KEYS, N_KF, N_MONO, W, mono, poses, records, stereo      # noqa: F401  (the fixtures and shapes of that test)

pytestmark = pytest.mark.gpu


def wait(cam, image):
    res = {k: v.copy() for k, v in cam.wait().items()}
    res.update({k: v.copy() for k, v in cam.landmarks().items()})
    res["packets"], res["table"] = (a.copy() for a in cam.wire())
    res["jpeg"], res["jpeg_sizes"], res["jpeg_status"] = (a.copy() for a in cam.jpeg_arrays())
    if image:
        res["whole"], res["whole_sizes"] = (a.copy() for a in cam.wire_image())
    return res


def same_unit(a, b, n):
    """every field of the result, the landmarks, the header + landmark packets and the files"""
    bad = [k for k in KEYS + LM_KEYS + ("table", "jpeg_sizes", "jpeg_status") if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]
    bad += [f"packets[{g}]" for g in range(n) if not np.array_equal(a["packets"][g, :a["table"][g, 1]], b["packets"][g, :b["table"][g, 1]])]
    bad += [f"jpeg[{g}]" for g in range(n) if not np.array_equal(a["jpeg"][g, :a["jpeg_sizes"][g]], b["jpeg"][g, :b["jpeg_sizes"][g]])]
    return bad


def check_against_host(capi, got, meta, n, wf, wi):
    jp = (got["jpeg"][:n], got["jpeg_sizes"][:n], got["jpeg_status"][:n]) if wi else (None, None, None)
    want, want_sizes = capi.wire_pack_image_host(got["kps_xy"][:n], got["n_kps"][:n], got["desc"][:n], got["norm2d"][:n], got["landmarks_3d"][:n], got["landmarks_flag"][:n],
                                                 got["global_desc"][:n], meta, *jp, width=W if wi else 0, height=H if wi else 0, with_features=wf)      # (the size travels with the file)
    out, sizes = got["whole"], got["whole_sizes"]
    print(f"with_features {wf} with_image {wi}: key points {got['n_kps'][:n].tolist()}, files {got['jpeg_sizes'][:n].tolist()} status {got['jpeg_status'][:n].tolist()}, "
          f"packet sizes {sizes[:, 1].tolist()}")
    assert out.shape == want.shape == (n, capi.wire_image_capacity(got["kps_xy"].shape[1], got["jpeg"].shape[1] if wi else 0)) and np.array_equal(sizes, want_sizes)
    for g in range(n):                                          # (bytes behind an image's packet are nobody's: the pinned block keeps what earlier units left)
        end = (sizes[g, 0] + sizes[g, 1] + 3) // 4 * 4 if sizes[g, 1] else 0
        assert np.array_equal(out[g, :end], want[g, :end]), g
    return sizes


def test_stereo_unit_packs_the_whole_descriptor_of_its_up_images(omni, ctx, stereo):
    c = omni.capi
    cam, unit, n = stereo["lc"].cam, stereo["unit"], DIRS * N_KF
    p7, meta = poses(1, N_KF), records(c, 21, n)
    cam.set_active(n)
    cam.set_stereo_model(stereo["model"])

    def run(flags):
        if flags is not None:
            cam.set_wire_image(*flags)
        cam.set_poses(p7)
        cam.set_wire_meta(meta)
        cam.enqueue_host(unit, True)
        return wait(cam, bool(flags and any(flags)))
    try:
        cam.set_jpeg(75)
        cam.set_wire(True)
        never = run(None)
        with pytest.raises(c.OmniError, match="stage off"):
            cam.wire_image()
        for wf, wi in ((False, True), (True, True), (True, False)):
            got = run((wf, wi))
            assert same_unit(got, never, n) == []
            sizes = check_against_host(c, got, meta, n, wf, wi)
            assert (got["jpeg_status"][:n] == c.JPEG_OK).all() and (got["n_kps"][:n] > 0).sum() >= n - 1          # not vacuous: files and key points to send
            for g in range(n):
                if got["n_kps"][g] == 0:
                    assert sizes[g].tolist() == [0, 0]
                    continue
                p = IC.parse_image(got["whole"][g, sizes[g, 0]:sizes[g, 0] + sizes[g, 1]].tobytes())
                assert p["image"] == (got["jpeg"][g, :got["jpeg_sizes"][g]].tobytes() if wi else b"") and len(p["desc_bits"]) == (64 * got["n_kps"][g] if wf else 0)
                assert (p["landmark_num"], p["width"], p["height"], p["frame_id"]) == (got["n_kps"][g], W if wi else 0, H if wi else 0, meta["frame_id"][g])
        again = run((False, False))                             # switched off again: as if it had never been on
        assert same_unit(again, never, n) == []
        with pytest.raises(c.OmniError, match="stage off"):
            cam.wire_image()
        # a partly filled unit: one key frame in a handle made for two
        cam.set_active(DIRS)
        cam.set_wire_image(True, True)
        cam.set_poses(p7[:1])
        cam.set_wire_meta(meta[:DIRS])
        cam.enqueue_host(np.ascontiguousarray(np.concatenate([unit[:DIRS], unit[n:n + DIRS]])), True)
        one = wait(cam, True)
        assert one["whole_sizes"].shape == (DIRS, 2)
        check_against_host(c, one, meta[:DIRS], DIRS, True, True)
    finally:
        cam.set_active(n)
        cam.set_wire(False)
        cam.set_jpeg(0)
        cam.set_stereo_model(None)


@pytest.mark.parametrize("capacity", [332, 800])
def test_unit_with_files_that_do_not_fit(omni, ctx, stereo, capacity):
    """a tiny capacity_per_image: every textured image is TRUNCATED (image_size 0, no file bytes); at 800 bytes the black image's file still fits"""
    c = omni.capi
    cam, unit, n = stereo["lc"].cam, stereo["unit"], DIRS * N_KF
    meta = records(c, 24, n)
    cam.set_active(n)
    cam.set_stereo_model(stereo["model"])
    try:
        cam.set_jpeg(75, capacity)
        cam.set_wire(True)
        cam.set_wire_image(False, True)
        cam.set_poses(poses(1, N_KF))
        cam.set_wire_meta(meta)
        cam.enqueue_host(unit, True)
        got = wait(cam, True)
        sizes = check_against_host(c, got, meta, n, False, True)
        trunc = got["jpeg_status"][:n] == c.JPEG_TRUNCATED
        assert trunc.sum() >= n - 1 and (capacity == 332 or not trunc[5])
        for g in range(n):
            if sizes[g, 1]:
                assert len(IC.parse_image(got["whole"][g, 3:3 + sizes[g, 1]].tobytes())["image"]) == (0 if trunc[g] else got["jpeg_sizes"][g])
    finally:
        cam.set_wire(False)
        cam.set_jpeg(0)
        cam.set_stereo_model(None)


def test_mono_unit_with_a_depth_model(omni, ctx, mono):
    c = omni.capi
    cam, unit, depth = mono["cam"], mono["unit"], mono["depth"]
    p7, meta = poses(2, N_MONO), records(c, 22, N_MONO)
    cam.set_depth_model(mono["model"], mono["camera"])
    try:
        cam.set_jpeg(75)
        cam.set_wire(True)

        def run(flags):
            cam.set_wire_image(*flags)
            cam.set_poses(p7)
            cam.set_depth_host(list(depth))
            cam.set_wire_meta(meta)
            cam.enqueue_host(unit, False)
            return wait(cam, any(flags))
        off, got = run((False, False)), run((True, True))
        assert same_unit(got, off, N_MONO) == []
        sizes = check_against_host(c, got, meta, N_MONO, True, True)
        assert (sizes[:, 1] > 177 + 4 * 4096 + 330).all() and (got["jpeg_status"] == c.JPEG_OK).all()
    finally:
        cam.set_wire(False)
        cam.set_jpeg(0)
        cam.set_depth_model(None)


def test_refusals(omni, ctx, stereo):
    """each before anything is enqueued; the handle stays usable"""
    c = omni.capi
    cam, unit, n = stereo["lc"].cam, stereo["unit"], DIRS * N_KF
    meta = records(c, 23, n)
    cam.set_active(n)
    cam.set_stereo_model(stereo["model"])
    try:
        cam.set_wire(False)
        cam.set_jpeg(75)
        with pytest.raises(c.OmniError, match="wire stage off"):
            cam.set_wire_image(True, True)
        cam.set_wire_image(False, False)                                        # (switching off what is off: fine)
        cam.set_wire(True)
        cam.set_jpeg(0)
        with pytest.raises(c.OmniError, match="encodes no JPEG"):
            cam.set_wire_image(False, True)
        cam.set_wire_image(True, False)                                         # (without the file: no JPEG stage needed)
        cam.set_jpeg(75, 1022)
        with pytest.raises(c.OmniError, match="multiple of 4"):
            cam.set_wire_image(True, True)
        cam.set_jpeg(75, 4096)
        cam.set_wire_image(True, True)
        cam.set_jpeg(0)                                                         # the JPEG stage taken away behind the switch: refused at enqueue
        cam.set_poses(poses(3, N_KF))
        cam.set_wire_meta(meta)
        with pytest.raises(c.OmniError, match="JPEG stage is off"):
            cam.enqueue_host(unit, True)
        cam.set_jpeg(75, 8192)                                                  # ... or given another capacity
        with pytest.raises(c.OmniError, match="another capacity"):
            cam.enqueue_host(unit, True)
        with pytest.raises(c.OmniError, match="without a pending"):             # nothing was enqueued by any of them
            cam.wait()
        cam.set_wire_image(True, True)
        cam.enqueue_host(unit, True)
        for call in (lambda: cam.set_wire_image(False, False), lambda: cam.wire_image()):
            with pytest.raises(c.OmniError, match="in flight"):
                call()
        got = wait(cam, True)                                                   # and the handle still works
        check_against_host(c, got, meta, n, True, True)
        cam.set_wire(False)                                                     # the wire stage off switches the whole descriptor off with it
        cam.set_poses(poses(3, N_KF))
        cam.enqueue_host(unit, True)
        cam.wait()
        with pytest.raises(c.OmniError, match="stage off"):
            cam.wire_image()
    finally:
        cam.set_wire(False)
        cam.set_jpeg(0)
        cam.set_stereo_model(None)
