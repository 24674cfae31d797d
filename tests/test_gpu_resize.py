"""The resize kernel (csrc/resize.hip, the stand-alone entry omni_resize_enqueue_dev) against the numpy restatement of its spec (tests/resize_ref.py): batch 3,
a source pitch of src_w + 5, destination images written back to back -- zero differing bytes, there is no tolerance (all arithmetic is integer and both sides read
the same tables' definition).  Sizes: a downscale of the camera's aspect, odd source sizes, an upscale whose first and last columns and rows clamp, the area-2x
and copy modes, and a source two columns wider than the destination (long runs of whole-weight taps).  The frames carry a saturated band at every edge."""
import numpy as np
import pytest

from tests import resize_ref as R

pytestmark = pytest.mark.gpu

CASES = [((188, 120), (128, 96), R.LINEAR), ((95, 61), (64, 48), R.LINEAR), ((37, 29), (96, 64), R.LINEAR), ((128, 96), (64, 48), R.AREA2), ((64, 48), (64, 48), R.COPY),
         ((130, 96), (128, 96), R.LINEAR)]


@pytest.mark.parametrize("src,dst,mode", CASES)
def test_bytes_equal_the_restatement(omni, ctx, src, dst, mode):
    c = omni.capi
    (w, h), (W, H) = src, dst
    frames = np.stack([R.edge_frame(40 + b, h, w) for b in range(3)])
    rs = c.Resize(ctx, w, h, W, H)
    try:
        assert rs.mode == mode == R.plan(w, h, W, H)["mode"]
        got = rs(frames, src_stride=w + 5)
        packed = rs(frames)
    finally:
        rs.close()
    ref = R.resize(frames, W, H)
    diff = int((got != ref).sum())
    print(f"{w}x{h} -> {W}x{H} (mode {mode}): {diff} of {ref.size} bytes differ from the restatement")
    assert got.shape == ref.shape == (3, H, W) and ref.std() > 5
    assert diff == 0
    assert np.array_equal(packed, ref)


def test_refusals(omni, ctx):
    c = omni.capi
    for bad in ((1, 48, 64, 48), (64, 48, 66, 48), (64, 48, 0, 48), (64, 0, 64, 48)):      # a one-column source, a width that is no multiple of 4, empty sides
        with pytest.raises(c.OmniError, match="omni_resize_create"):
            c.Resize(ctx, *bad)
    rs = c.Resize(ctx, 95, 61, 64, 48)
    try:
        with pytest.raises(c.OmniError, match="stride"):
            rs.enqueue_dev(16, 94, 1, 16)                                                    # (refused before the pointers are used)
        assert np.array_equal(rs(R.edge_frame(1, 61, 95)), R.resize(R.edge_frame(1, 61, 95), 64, 48)[None])
    finally:
        rs.close()
