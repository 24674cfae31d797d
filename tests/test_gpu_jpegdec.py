"""The JPEG decode stage alone (csrc/jpeg_dec.hip through omni_jpegdec_enqueue_host) against the g++ build of the arithmetic it runs (csrc/jpeg_dec_plan.h inside
the library, held to Pillow's pixels by tests/test_jpegdec_plan_cpu.py) and against the committed Pillow pixels (tests/golden/jpegdec_cases.npz; Pillow itself is
not needed here): status and EVERY pixel equal, nothing written outside the pictures or behind the stage's own buffers.  Every OK fixture at the default
subsequence length and at S = 128 (hundreds of subsequences and dozens of relaxation rounds on a tiny picture; the 160 x 120 file then has more subsequences than
the entropy kernel's workgroup has lanes), mixed batches, strides, mutated scans, refusals."""
import numpy as np
import pytest

from tests import jpegdec_cases as J

pytestmark = pytest.mark.gpu
S_ENV = "OMNI_JPEGDEC_SUBSEQ_BITS"


@pytest.fixture(scope="module")
def reference(omni):
    """name -> (status, pixels) of the g++ build; computed once"""
    c = omni.capi
    out = {}
    for name in J.names(J.OK) + J.names(J.HOST):
        out[name] = c.jpeg_decode_host(J.file_of(name))
        assert out[name][0] == J.SPECS[name][4] and np.array_equal(out[name][1], J.pixels_of(name)), name
    return out


def differing(a, b) -> int:
    return int((np.asarray(a) != np.asarray(b)).sum()) if np.asarray(a).shape == np.asarray(b).shape else -1


@pytest.mark.parametrize("name", J.names(J.OK))
def test_kernels_equal_the_cpu_build_and_pillow_pixel_for_pixel(omni, ctx, reference, monkeypatch, name):
    c = omni.capi
    w, h = J.SPECS[name][:2]
    data = J.file_of(name)
    default = c.config_value(S_ENV)
    total = 0
    for S in (None, 128):
        if S:
            monkeypatch.setenv(S_ENV, str(S))
        dec = c.JpegDec(ctx, w, h, 1, max(len(data), 1024))
        (st,), pix = dec([data])
        rounds, n_sub, bits = dec.last_stats(1)[0]
        dec.close()
        _, _, emu = c.jpeg_decode_parallel_host(data, S or default)
        d = differing(pix[0], reference[name][1]) + differing(pix[0], J.pixels_of(name))
        total += d
        print(f"{name} S={bits}: {n_sub} subsequences, {rounds} rounds, differing pixels {d}")
        assert st == c.JPEGDEC_OK and d == 0 and dec.last_guard_ok, (name, S, st, d)
        assert (n_sub, bits, rounds) == (emu["n_sub"], emu["subseq_bits"], emu["rounds"]) and bits == (S or default), (name, S)
        if S == 128 and name == "gray_160x120_q75":
            assert n_sub > 256                                 # lanes stride over the subsequences
        if S == 128 and name == "gray_96x64_q100":
            assert rounds > 16                                 # dozens of rounds
    assert total == 0


def test_a_mixed_batch_gray_colour_and_a_file_for_the_host(omni, ctx, reference):
    c = omni.capi
    st, gray = c.jpeg_encode_host(np.ascontiguousarray(J.pixels_of("color_80x48_444")), 75)      # a gray file of the same size, the project's own encoder
    assert st == c.JPEG_OK
    names = ["color_80x48_420", "color_80x48_444", "rst_color_80x48_420"]
    files = [gray] + [J.file_of(n) for n in names]
    want = [c.jpeg_decode_host(gray)] + [reference[n] for n in names]
    dec = c.JpegDec(ctx, 80, 48, 4, 8192)
    status, pix = dec(files)
    assert status == [c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_HOST] == [s for s, _ in want] and dec.last_guard_ok
    for i in range(4):
        assert differing(pix[i], want[i][1]) == 0, i
    status, pix = dec(files[::-1])                                                               # the handle again, another order
    assert status == [c.JPEGDEC_HOST, c.JPEGDEC_OK, c.JPEGDEC_OK, c.JPEGDEC_OK] and all(differing(pix[i], want[3 - i][1]) == 0 for i in range(4))
    dec.close()


def test_batch_of_one_and_of_max_images(omni, ctx, reference):
    c = omni.capi
    names = ["gray_96x64_q5", "gray_96x64_q75", "gray_96x64_q100", "noise_96x64_q100", "opt_96x64_q75", "rst_96x64_q75"]
    dec = c.JpegDec(ctx, 96, 64, len(names), 16384)
    status, pix = dec([J.file_of(n) for n in names])
    assert status == [reference[n][0] for n in names] and dec.last_guard_ok
    assert all(differing(pix[i], reference[n][1]) == 0 for i, n in enumerate(names))
    for n in (names[2], names[5]):
        status, pix = dec([J.file_of(n)])
        assert status == [reference[n][0]] and differing(pix[0], reference[n][1]) == 0 and dec.last_guard_ok
    # two enqueues back to back, no synchronisation in between: the second waits for the first one's upload before it refills the pinned block
    a, b = [J.file_of(n) for n in names[:3]], [J.file_of(n) for n in names[3:]]
    out = ctx.to_device(np.full(6 * 64 * 96, 0xA5, np.uint8))
    stat = ctx.to_device(np.full(6, -1, np.int32))
    try:
        dec.enqueue_host(a, out, 96, stat)
        dec.enqueue_host(b, out + 3 * 64 * 96, 96, stat + 12)
        got = ctx.from_device(out, (6, 64, 96), np.uint8)
        assert [int(v) for v in ctx.from_device(stat, (6,), np.int32)] == [reference[n][0] for n in names]
        assert all(differing(got[i], reference[n][1]) == 0 for i, n in enumerate(names))
    finally:
        ctx.free(out)
        ctx.free(stat)
        dec.close()


def test_out_stride_above_width_leaves_the_bytes_between_rows(omni, ctx, reference):
    c = omni.capi
    for names in (["gray_17x13_q75", "gray_17x13_q100"], ["color_72x40_422"], ["rst_96x64_q75", "gray_96x64_q75"]):
        w, h = J.SPECS[names[0]][:2]
        dec = c.JpegDec(ctx, w, h, 2, 8192)
        status, pix = dec([J.file_of(n) for n in names], stride=w + 7)
        dec.close()
        assert status == [reference[n][0] for n in names] and dec.last_guard_ok
        for i, n in enumerate(names):
            assert differing(pix[i][:, :w], reference[n][1]) == 0 and (pix[i][:, w:] == 0xA5).all(), n


def test_a_file_above_the_capacity_is_decoded_on_the_host(omni, ctx, reference):
    c = omni.capi
    big, small = "gray_96x64_q100", "gray_96x64_q5"
    assert len(J.file_of(small)) < 1024 < len(J.file_of(big))
    dec = c.JpegDec(ctx, 96, 64, 2, 1024)
    status, pix = dec([J.file_of(big), J.file_of(small)])
    dec.close()
    assert status == [c.JPEGDEC_HOST, c.JPEGDEC_OK] and dec.last_guard_ok
    assert differing(pix[0], reference[big][1]) == 0 and differing(pix[1], reference[small][1]) == 0


def test_the_camera_size_in_a_batch(omni, ctx, reference):
    c = omni.capi
    name = "gray_640x480_q75"
    dec = c.JpegDec(ctx, 640, 480, 2)
    status, pix = dec([J.file_of(name)] * 2)
    stats = dec.last_stats(2)
    dec.close()
    print(f"640 x 480: (rounds, subsequences, bits) {stats}")
    assert status == [c.JPEGDEC_OK] * 2 and dec.last_guard_ok and differing(pix[0], reference[name][1]) == 0 and differing(pix[1], reference[name][1]) == 0


def test_more_subsequences_than_the_kernel_holds_double_their_length(omni, ctx, monkeypatch):
    """640 x 480 noise at quality 100 and S = 128: tens of thousands of subsequences, above the entropy kernel's 4096 per image -- S is doubled until they fit, every
    lane then owns 16 of them (all its `need` bits), and the pixels are the g++ build's"""
    c = omni.capi
    noise = np.random.default_rng(11).integers(0, 256, (480, 640)).astype(np.uint8)
    st, data = c.jpeg_encode_host(noise, 100)
    assert st == c.JPEG_OK
    want = c.jpeg_decode_host(data)
    monkeypatch.setenv(S_ENV, "128")
    dec = c.JpegDec(ctx, 640, 480, 1, len(data))
    (status,), pix = dec([data])
    rounds, n_sub, bits = dec.last_stats(1)[0]
    dec.close()
    print(f"640 x 480 noise q100: {len(data)} bytes, {n_sub} subsequences of {bits} bits, {rounds} rounds")
    assert len(data) * 8 // 128 > 4096 and bits > 128 and 2048 < n_sub <= 4096
    assert status == want[0] == c.JPEGDEC_OK and differing(pix[0], want[1]) == 0 and dec.last_guard_ok


def test_mutated_scans_equal_the_host_decoder(omni, ctx, monkeypatch):
    """status and pixels equal the host function's (a CORRUPT picture is all zeros); the guard bands behind the output, the coefficient and the DC buffer are
    unchanged.  The same files ran clean under the sanitizers on the CPU (tests/test_jpegdec_plan_cpu.py); they go to the GPU once, at S = 128 (many subsequences
    and rounds)"""
    c = omni.capi
    muts = J.mutations()
    want = [c.jpeg_decode_host(data) for _, data in muts]
    monkeypatch.setenv(S_ENV, "128")
    dec = c.JpegDec(ctx, 96, 64, len(muts), 4096)
    status, pix = dec([data for _, data in muts])
    dec.close()
    assert dec.last_guard_ok
    n_corrupt = 0
    for i, (what, _) in enumerate(muts):
        assert status[i] == want[i][0] and differing(pix[i], want[i][1]) == 0, what
        n_corrupt += status[i] == c.JPEGDEC_CORRUPT
    print(f"{len(muts)} mutations: {n_corrupt} CORRUPT")
    assert n_corrupt >= 10


def test_refusals_enqueue_nothing(omni, ctx, monkeypatch):
    c = omni.capi
    L = c.lib()
    for args, word in (((0, 8, 1, 4096), b"outside 1..65535"), ((8, 65536, 1, 4096), b"outside 1..65535"), ((8, 8, 0, 4096), b"max_images"), ((8, 8, 1, 100), b"capacity"),
                       ((65535, 65535, 1, 4096), b"blocks")):
        assert not L.omni_jpegdec_create(ctx.h, *args) and word in L.omni_last_error(), args
    monkeypatch.setenv(S_ENV, "384")
    assert not L.omni_jpegdec_create(ctx.h, 8, 8, 1, 4096) and b"power of two" in L.omni_last_error()
    monkeypatch.setenv(S_ENV, "64")
    assert not L.omni_jpegdec_create(ctx.h, 8, 8, 1, 4096) and S_ENV.encode() in L.omni_last_error()
    monkeypatch.delenv(S_ENV)
    dec = c.JpegDec(ctx, 96, 64, 2)
    out = ctx.to_device(np.full(2 * 64 * 96 + 64, 0xA5, np.uint8))
    stat = ctx.to_device(np.full(2, -1, np.int32))
    good = J.file_of("gray_96x64_q75")
    try:
        for files, stride, word in (([good, J.file_of("prog_96x64_q75")], 96, "UNSUPPORTED"), ([J.file_of("gray_17x13_q75"), good], 96, "17x13"), ([good] * 3, 96, "images"),
                                    ([], 96, "images"), ([good], 95, "out_stride")):
            with pytest.raises(c.OmniError, match=word):
                dec.enqueue_host(files, out, stride, stat)
        assert (ctx.from_device(out, (2 * 64 * 96 + 64,), np.uint8) == 0xA5).all() and (ctx.from_device(stat, (2,), np.int32) == -1).all()
        dec.enqueue_host([good, b"\xff\xd8 no frame header at all"], out, 96, stat)               # (a file that is no file is not refused: zeros + CORRUPT)
        got = ctx.from_device(out, (2 * 64 * 96 + 64,), np.uint8)
        assert [int(v) for v in ctx.from_device(stat, (2,), np.int32)] == [c.JPEGDEC_OK, c.JPEGDEC_CORRUPT]
        assert differing(got[:64 * 96].reshape(64, 96), J.pixels_of("gray_96x64_q75")) == 0 and not got[64 * 96:2 * 64 * 96].any() and (got[2 * 64 * 96:] == 0xA5).all()
    finally:
        ctx.free(out)
        ctx.free(stat)
        dec.close()
