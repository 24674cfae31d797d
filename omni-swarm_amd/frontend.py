"""LoopCam: the per-keyframe CNN frontend (host-side mirror over the C ABI).

Mirrors /root/reference/swarm_loop/src/loop_cam.cpp:
    on_flattened_images                :178-229   loop over the camera directions of one fisheye key frame
    generate_stereo_image_descriptor   :341-523   SuperPoint(up), SuperPoint(down), MobileNetVLAD(up), BF up<->down
    extractor_img_desc_deepnet         :525-585   fisheye mask (rows [3H/4,H) zeroed), the two CNN calls
    match_HFNet_local_features         :141-174   cv::BFMatcher(NORM_L2, crossCheck) on the 64-d descriptors
The reference runs these 8 + 4 engine calls and 4 matches strictly one after another, each with its own H2D/D2H and
stream sync; here one key frame is three batched enqueues on one HIP stream (8 SuperPoint images, 4
MobileNetVLAD images on a second stream, 4 descriptor-set pairs) with every intermediate resident in HBM and one small
D2H at the end.
Camera geometry (liftProjective, SVD triangulation, loop_cam.cpp:73-106,405-454,558-576): a capi.StereoModel
(stereo_model=) moves it into the unit -- f64 on the GPU (csrc/landmarks.hip), the lens a capi.CameraModel
(camera_model=: camodocal's PINHOLE with distortion or MEI; the ideal pinhole without one), the key frame's
pose_drone set with set_poses() before every key frame; without a model it is left to the caller, for whom the 2-D key
points, descriptors, global descriptors and the up/down match lists are everything those steps consume.
CameraConfig::PINHOLE_DEPTH (generate_gray_depth_image_descriptor, :231-339): a capi.DepthModel (depth_model=) makes the
object a MONO unit -- n_dirs images of one camera each, no down camera, no rows blanked -- whose lifted key points and
depth landmarks (:260-304) come out of the unit too (csrc/depth_landmarks.hip); set_poses() and set_depth() before every unit.
"""
from __future__ import annotations

import numpy as np

from . import capi


class LoopCam:
    def __init__(self, ctx: capi.Context, sp_weights: dict, pca_comp, pca_mean, vlad_weights: dict, vlad_specs,
                 vlad_shape=(32, 112, 4096), width: int = 600, height: int = 480, thres: float = 0.015,
                 max_num: int = 200, precision: int = capi.PREC_F16, n_dirs: int = 4, fisheye: bool = True,
                 accept_min_3d_pts: int = 0, stereo_model: capi.StereoModel = None, camera_model: capi.CameraModel = None,
                 depth_model: capi.DepthModel = None, pca_fit: capi.PcaFit = None):
        if depth_model is not None and stereo_model is not None:
            raise ValueError("LoopCam: depth_model (PINHOLE_DEPTH, one camera per image) and stereo_model (an up / down pair per direction) are two camera configurations")
        self.mono = depth_model is not None
        if self.mono:
            fisheye = False                        # loop_cam.cpp:536 blanks rows for STEREO_FISHEYE only
        self.ctx, self.W, self.H, self.n_dirs, self.max_num, self.fisheye = ctx, width, height, n_dirs, max_num, fisheye
        self.accept_min_3d_pts = accept_min_3d_pts
        self.sp = capi.SuperPoint(ctx, sp_weights, pca_comp, pca_mean, width, height, thres, max_num, precision, (1 if self.mono else 2) * n_dirs)
        k, d, o = vlad_shape
        # MobileNetVLAD is ~50 small launches: on its own HIP stream they overlap SuperPoint's large convolutions
        import os
        self._own_vctx = os.environ.get("OMNI_VLAD_SAME_STREAM", "0") != "1"
        self.vctx = capi.Context(ctx.device_id) if self._own_vctx else ctx
        self.vlad = capi.MobileNetVLAD(self.vctx, vlad_weights, vlad_specs, k, d, o, width, height, n_dirs)
        self.out_dim = o
        self.dim = self.sp.desc_dim
        # OUTPUT_RAW_SUPERPOINT_DESC (loop_cam.cpp:51-53, 577-582) without the dump: every unit adds its key points' 256-d descriptors to the fit's moments on the GPU
        self.pca_fit = pca_fit
        if pca_fit is not None:
            self.sp.set_pcafit(pca_fit)
        # the whole key frame as one asynchronous unit with a single pinned result block (csrc/cam.hip)
        self.cam = capi.Cam(self.sp, self.vlad, n_dirs, o, capi.BF_OPENCV, mono=self.mono)
        self.stereo_model = stereo_model
        if stereo_model is not None:
            self.cam.set_stereo_model(stereo_model)
        self.camera_model = camera_model
        self.depth_model = depth_model
        if depth_model is not None:
            self.cam.set_depth_model(depth_model, camera_model)      # (the lens travels with the depth model: a mono handle takes no set_camera_model)
        elif camera_model is not None:
            self.cam.set_camera_model(camera_model)

    def set_poses(self, poses7):
        """pose_drone (xyz + quaternion wxyz) of the key frames of the NEXT unit, [n_keyframes][7]: needed before every key frame when a stereo_model is set"""
        self.cam.set_poses(poses7)

    def set_depth(self, frames, stride: int = 0):
        """depth_model: the depth frames ([H][W] u16 millimetres; None: no depth image, no landmarks) of the NEXT unit's images, copied before the call returns"""
        self.cam.set_depth_host(frames, stride)

    def close(self):
        self.cam.close()
        self.sp.close()
        self.vlad.close()
        if self._own_vctx:
            self.vctx.close()

    def enqueue_dev(self, gray_dev: int, stride: int):
        """gray_dev: [2*n_dirs][H][W] u8 in HBM -- images 0..n_dirs-1 are the 'up' (main) camera of each direction,
        n_dirs..2*n_dirs-1 the 'down' camera.  Asynchronous: SuperPoint + BF matching on the context's stream,
        MobileNetVLAD on a second stream, all D2H copies included (loop_cam.cpp:350-351, 553-556, 147-150)."""
        self.cam.enqueue_dev(gray_dev, stride, self.fisheye)

    def enqueue_host(self, gray_host: np.ndarray):
        """Same with the images in (pinned) host memory, [2*n_dirs][H][W] u8: one asynchronous upload in front of the kernels
        (omni_cam_enqueue_host).  The array must stay untouched until fetch() returns."""
        self.cam.enqueue_host(gray_host, self.fisheye)

    def fetch(self) -> dict:
        """Waits for the key frame and returns one FisheyeFrameDescriptor_t's worth of CNN outputs (copies: the pinned
        block is reused by the next enqueue)."""
        r = self.cam.wait()
        n = r["global_desc"].shape[0]          # the unit's directions: n_dirs, or fewer after Cam.set_active
        nk = r["n_kps"]
        images = []
        if self.mono:                            # one camera per image; the lifted key points and the depth landmarks computed inside the unit
            lm = self.cam.landmarks()
            for d in range(n):
                nu = int(nk[d])
                images.append({"landmarks_2d": r["kps_xy"][d, :nu].copy(), "feature_descriptor": r["desc"][d, :nu].copy(), "scores": r["scores"][d, :nu].copy(),
                               "landmark_num": nu, "image_desc": r["global_desc"][d].copy(), "direction": 0, "landmarks_2d_norm": lm["norm2d"][d, :nu].copy(),
                               "landmarks_3d": lm["landmarks_3d"][d, :nu].copy(), "landmarks_flag": lm["landmarks_flag"][d, :nu].copy(), "count_3d": int(lm["count_3d"][d])})
            return {"images": images, "landmark_num": int(sum(i["landmark_num"] for i in images))}
        for d in range(n):
            nu, nd = int(nk[d]), int(nk[n + d])
            k = int(r["n_matches"][d]) if nu > self.accept_min_3d_pts else 0    # :388 `if (pts_up.size() > ACCEPT_MIN_3D_PTS)`
            images.append({"landmarks_2d": r["kps_xy"][d, :nu].copy(), "feature_descriptor": r["desc"][d, :nu].copy(),
                           "scores": r["scores"][d, :nu].copy(), "landmark_num": nu, "image_desc": r["global_desc"][d].copy(),
                           "landmarks_2d_down": r["kps_xy"][n + d, :nd].copy(), "feature_descriptor_down": r["desc"][n + d, :nd].copy(),
                           "ids_up": r["match_up"][d, :k].copy(), "ids_down": r["match_down"][d, :k].copy(), "direction": d})
        if self.stereo_model is not None:        # generate_stereo_image_descriptor's landmarks (:397-444), computed inside the unit
            lm = self.cam.landmarks()
            for d, im in enumerate(images):
                nu, nd = int(nk[d]), int(nk[n + d])
                im.update({"landmarks_2d_norm": lm["norm2d"][d, :nu].copy(), "landmarks_3d": lm["landmarks_3d"][d, :nu].copy(),
                           "landmarks_flag": lm["landmarks_flag"][d, :nu].copy(), "landmarks_2d_norm_down": lm["norm2d"][n + d, :nd].copy(),
                           "landmarks_3d_down": lm["landmarks_3d"][n + d, :nd].copy(), "landmarks_flag_down": lm["landmarks_flag"][n + d, :nd].copy(),
                           "count_3d": int(lm["count_3d"][d])})
        return {"images": images, "landmark_num": int(sum(i["landmark_num"] for i in images))}

    def on_fisheye_images(self, up_raw: np.ndarray, down_raw: np.ndarray, undist_up, undist_down) -> dict:
        """The blocking call from the two RAW fisheye frames [src_h][src_w] uint8 of a key frame: undist_up / undist_down are the cameras'
        flatten.FisheyeUndist (or capi.Flatten) objects, whose last views -- as many as the unit has directions: 1..4 of five, the top view
        is never read (loop_cam.h:64-73) -- are flattened inside the unit (omni_cam_enqueue_fisheye_host).  Returns what
        on_flattened_images returns for the same views."""
        fl = [getattr(u, "flatten", u) for u in (undist_up, undist_down)]
        raw = [np.ascontiguousarray(r, np.uint8)[None] for r in (up_raw, down_raw)]
        self.cam.enqueue_fisheye_host(fl[0], fl[1], raw[0], raw[1], len(fl[0].shapes) - self.cam.n_active, self.fisheye)
        return self.fetch()

    def on_fisheye_jpeg(self, up_file: bytes, down_file: bytes, undist_up, undist_down) -> dict:
        """on_fisheye_images with the key frame's two RAW fisheye frames as JPEG files (bytes): decoded and flattened inside the unit
        (omni_cam_enqueue_fisheye_jpeg_host).  Returns what on_fisheye_images returns for the decoded frames; self.cam.jpegdec_status() holds the two statuses."""
        fl = [getattr(u, "flatten", u) for u in (undist_up, undist_down)]
        self.cam.enqueue_fisheye_jpeg_host(fl[0], fl[1], [bytes(up_file)], [bytes(down_file)], len(fl[0].shapes) - self.cam.n_active, self.fisheye)
        return self.fetch()

    def on_stereo_images(self, left_raw: np.ndarray, right_raw: np.ndarray, resize: capi.Resize) -> dict:
        """The blocking call for a STEREO_PINHOLE key frame (generate_stereo_image_descriptor for one direction, loop_cam.cpp:189-196): the two RAW frames
        [src_h][src_w] uint8 of the camera's size -- or [k][src_h][src_w] for the k key frames of the unit's active size -- are resized to the networks' size
        inside the unit (omni_cam_enqueue_raw_host), left = up, right = down, no rows blanked.  Returns what on_flattened_images returns for the resized images
        on a LoopCam made with fisheye=False."""
        raw = [np.ascontiguousarray(r, np.uint8) for r in (left_raw, right_raw)]
        raw = [r[None] if r.ndim == 2 else r for r in raw]
        self.cam.enqueue_raw_host(resize, raw[0], raw[1])
        return self.fetch()

    def on_flattened_images(self, up: np.ndarray, down: np.ndarray) -> dict:
        """Host-pointer convenience (the reference's blocking call): up/down [n_dirs][H][W] uint8."""
        g = np.ascontiguousarray(np.concatenate([up, down]), np.uint8)
        p = self.ctx.to_device(g)
        try:
            self.enqueue_dev(p, self.W)
            return self.fetch()
        finally:
            self.ctx.free(p)
