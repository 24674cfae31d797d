"""The JPEG stage alone (csrc/jpeg.hip through omni_jpeg_enqueue_dev) against the g++ build of the arithmetic it runs (csrc/jpeg_plan.h in
tests/cpp/jpeg_plan_pin.cpp and inside the library, both held to Pillow's whole files by tests/test_jpeg_plan_cpu.py) and against the committed Pillow files
(tests/golden/jpeg_cases.npz; Pillow itself is not needed here): size, status and EVERY byte equal, nothing written past a capacity.  Cases: tests/jpeg_cases.py --
8 x 8, 16 x 8, 24 x 16, 13 x 11, 64 x 48, five different 64 x 48 images in one call, 24 x 16 with stride 40; noise, smooth, all 0, all 255, black / white;
qualities 10, 50, 75, 100 -- and one 600 x 480 synthetic frame (4 500 blocks: 18 workgroups of the block kernels, 5 steps of the scan) with zero_from_row = 360."""
import numpy as np
import pytest

from tests import jpeg_cases as J

pytestmark = pytest.mark.gpu
NAMES = [f"{c}_{w}x{h}" for (w, h) in J.SHAPES for c in J.CONTENTS] + ["batch_64x48"]


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """case id -> the pin program's [(status, size, buffer)] per image; computed once"""
    tmp = tmp_path_factory.mktemp("jpeg_plan")
    exe = J.build_pin(tmp)
    cases = J.cases()
    res = J.run_pin(exe, [(g, g.shape[1], q, g.shape[0], J.roomy(g.shape[1], g.shape[0])) for _, imgs, q, _ in cases for g in imgs], tmp)
    out, at = {}, 0
    for name, imgs, q, files in cases:
        out[name] = (imgs, q, files, res[at:at + len(imgs)])
        at += len(imgs)
    return out


def differing(a: bytes, b: bytes) -> int:
    return abs(len(a) - len(b)) + sum(x != y for x, y in zip(a, b))


@pytest.mark.parametrize("name", NAMES)
def test_kernels_equal_the_cpu_build_and_pillow_byte_for_byte(omni, ctx, reference, name):
    c = omni.capi
    total = 0
    for q in J.QUALITIES:
        imgs, _, files, ref = reference[f"{name}_q{q}"]
        k, h, w = imgs.shape
        enc = c.Jpeg(ctx, w, h, k, q, J.roomy(w, h))
        got = enc(imgs)
        enc.close()
        assert enc.last_guard_ok
        for i in range(k):
            st, sz, buf = ref[i]
            d = differing(got[i][1], buf[:sz].tobytes()) + differing(got[i][1], files[i])
            total += d
            assert got[i][0] == st == c.JPEG_OK and len(got[i][1]) == sz and d == 0, (name, q, i, got[i][0], len(got[i][1]), sz)
            assert (enc.last_raw[i, sz:] == 0xA5).all()                                    # nothing behind the file either
    print(f"{name}: differing bytes against the g++ build and Pillow's files over {len(J.QUALITIES)} qualities: {total}")


def test_stride_above_width(omni, ctx, reference):
    c = omni.capi
    (w, h), stride = J.STRIDE_CASE
    for content in J.CONTENTS:
        for q in J.QUALITIES:
            imgs, _, files, _ = reference[f"{content}_{w}x{h}_q{q}"]
            enc = c.Jpeg(ctx, w, h, 1, q, J.roomy(w, h))
            (st, data), = enc(imgs, stride=stride)
            enc.close()
            assert st == c.JPEG_OK and data == files[0] and enc.last_guard_ok, (content, q)


def test_a_network_size_frame_with_the_mask_row(omni, ctx):
    """600 x 480 (the reference's flattened views), two different frames, zero_from_row = 360 = omni_fisheye_mask_rows(480)'s first row, the default capacity"""
    from omni_swarm_amd import synth
    c = omni.capi
    w, h = 600, 480
    frames = np.stack([synth.image_u8(77, h, w, n_shapes=120), synth.image_u8(78, h, w, n_shapes=40)[::-1]])
    for q, zfr in ((75, 360), (100, 360), (50, -1)):
        enc = c.Jpeg(ctx, w, h, 2, q)
        assert enc.capacity == w * h // 2
        got = enc(frames, zero_from_row=zfr)
        enc.close()
        for g, (st, data) in zip(frames, got):
            st_h, ref = c.jpeg_encode_host(g, q, zero_from_row=zfr, capacity=enc.capacity)
            d = differing(data, ref)
            print(f"600 x 480 q{q} zero_from_row {zfr}: {len(ref)} bytes, status {st} / {st_h}, differing bytes {d}")
            assert st == st_h and d == 0 and enc.last_guard_ok
        assert any(st == c.JPEG_OK for st, _ in got) or q == 100
        blank = frames.copy()
        if zfr >= 0:
            blank[:, zfr:] = 0
            assert [c.jpeg_encode_host(g, q, capacity=enc.capacity) for g in blank] == got          # = the image with those rows zeroed


def test_truncation(omni, ctx, reference):
    """a capacity one byte short of the largest file of a batch: that image TRUNCATED with size 0, the others whole, no byte past any image's capacity"""
    c = omni.capi
    imgs, q, files, _ = reference["batch_64x48_q75"]
    sizes = [len(f) for f in files]
    big = int(np.argmax(sizes))
    assert sizes.count(sizes[big]) == 1
    for cap, want in ((sizes[big], [c.JPEG_OK] * J.BATCH), (sizes[big] - 1, [c.JPEG_TRUNCATED if i == big else c.JPEG_OK for i in range(J.BATCH)])):
        enc = c.Jpeg(ctx, 64, 48, J.BATCH, q, cap)
        got = enc(imgs)
        enc.close()
        assert [st for st, _ in got] == want and enc.last_guard_ok
        for i, (st, data) in enumerate(got):
            assert data == (files[i] if st == c.JPEG_OK else b"")
            if st == c.JPEG_OK:
                assert (enc.last_raw[i, len(data):] == 0xA5).all()
    small = sorted(sizes)[0]
    enc = c.Jpeg(ctx, 64, 48, J.BATCH, q, c.JPEG_HEADER_BYTES + 2)              # room for no scan at all: every image TRUNCATED before its scan is read
    got = enc(imgs)
    enc.close()
    assert small > c.JPEG_HEADER_BYTES + 2 and got == [(c.JPEG_TRUNCATED, b"")] * J.BATCH and enc.last_guard_ok


def test_refusals(omni, ctx):
    c = omni.capi
    L = c.lib()
    for args, word in (((0, 8, 1, 75, 4096), b"outside 1..65535"), ((8, 65536, 1, 75, 4096), b"outside 1..65535"), ((8, 8, 0, 75, 4096), b"max_images"),
                       ((8, 8, 1, 75, c.JPEG_HEADER_BYTES + 1), b"capacity"), ((65535, 65535, 1, 75, 4096), b"blocks")):
        assert not L.omni_jpeg_create(ctx.h, *args) and word in L.omni_last_error(), args
    enc = c.Jpeg(ctx, 16, 8, 2, 75, 4096)
    buf = ctx.to_device(np.full(2 * 4096 + 64, 0xA5, np.uint8))
    src = ctx.to_device(np.zeros((2, 8, 16), np.uint8))
    try:
        for (stride, n, zfr), word in (((16, 0, 8), b"images"), ((16, 3, 8), b"images"), ((15, 1, 8), b"stride"), ((16, 1, 9), b"zero_from_row"), ((16, 1, -1), b"zero_from_row")):
            assert L.omni_jpeg_enqueue_dev(enc.h, src, stride, n, zfr, buf, buf + 8192, buf + 8192 + 16) == c.ERR_INVALID and word in L.omni_last_error(), (stride, n, zfr)
        assert L.omni_jpeg_enqueue_dev(enc.h, None, 16, 1, 8, buf, buf + 8192, buf + 8192 + 16) == c.ERR_INVALID
        assert (ctx.from_device(buf, (2 * 4096 + 64,), np.uint8) == 0xA5).all()            # refused before anything was launched
    finally:
        ctx.free(buf)
        ctx.free(src)
        enc.close()
