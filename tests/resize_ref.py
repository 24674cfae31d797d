"""numpy restatement of the resize spec of csrc/resize_plan.h: cv::resize(src, dst, cv::Size(W, H)) with INTER_LINEAR on a CV_8UC1 image as OpenCV 3.4's own
(non-IPP) code runs it -- what both of the reference's engines do in front of their networks (superpoint_tensorrt.cpp:123-125, mobilenetvlad_tensorrt.cpp:6-8).
OpenCV is on no machine of this project: parity with it is unpinned; this file is the statement the plan header, the kernel and the key-frame unit are held to.
Written independently of the header: vectorised float32 / int32 numpy, no loop over pixels."""
import numpy as np

COPY, AREA2, LINEAR = 0, 1, 2
ONE = 2048


def axis(n_src: int, n_dst: int, clamp_x: bool):
    """(ofs int32 [n_dst], coef int16 [n_dst][2]) of one axis"""
    scale = 1.0 / (float(n_dst) / float(n_src))                                # double
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = f - s                                                                  # float32 - float32
    s = s.astype(np.int32)
    c0 = np.rint((np.float32(1) - f) * np.float32(ONE))                        # round half to even
    c1 = np.rint(f * np.float32(ONE))
    if clamp_x:
        lo, hi = s < 0, s >= n_src - 1
        s = np.where(lo, 0, np.where(hi, n_src - 1, s)).astype(np.int32)
        c0 = np.where(lo | hi, ONE, c0)
        c1 = np.where(lo | hi, 0, c1)
    return s, np.stack([c0, c1], 1).astype(np.int16)


def plan(w: int, h: int, W: int, H: int):
    mode = COPY if (w == W and h == H) else AREA2 if (w == 2 * W and h == 2 * H) else LINEAR
    xofs, ialpha = axis(w, W, True)
    yofs, ibeta = axis(h, H, False)
    return {"mode": mode, "xofs": xofs, "ialpha": ialpha, "yofs": yofs, "ibeta": ibeta}


def resize(src: np.ndarray, W: int, H: int) -> np.ndarray:
    """[h][w] or [n][h][w] uint8 -> the same with [H][W]"""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    if src.ndim == 3:
        return np.stack([resize(s, W, H) for s in src])
    h, w = src.shape
    p = plan(w, h, W, H)
    if p["mode"] == COPY:
        return src.copy()
    s = src.astype(np.int32)
    if p["mode"] == AREA2:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1 = p["xofs"], np.minimum(p["xofs"] + 1, w - 1)
    a = p["ialpha"].astype(np.int32)
    R = s[:, x0] * a[None, :, 0] + s[:, x1] * a[None, :, 1]                    # [h][W]
    y0, y1 = np.clip(p["yofs"], 0, h - 1), np.clip(p["yofs"] + 1, 0, h - 1)
    b = p["ibeta"].astype(np.int32)
    out = (((b[:, None, 0] * (R[y0] >> 4)) >> 16) + ((b[:, None, 1] * (R[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def edge_frame(seed: int, h: int, w: int) -> np.ndarray:
    """the tests' source frame: a synthetic image (cut out of a larger one where the generator's shapes need the room) with a saturated band at every edge,
    so that the clamped border taps read extreme values"""
    from omni_swarm_amd import synth
    g = synth.image_u8(seed, max(h, 64), max(w, 64), n_shapes=60)[:h, :w].copy()
    g[0], g[-1], g[:, 0], g[:, -1] = 255, 0, 0, 255
    return g
