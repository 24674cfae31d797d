"""CPU gate of the JPEG arithmetic (csrc/jpeg_plan.h, what csrc/jpeg.hip runs one 8 x 8 block per lane): built with g++ into tests/cpp/jpeg_plan_pin.cpp and held
to Pillow (libjpeg-turbo: jpeg_set_defaults, jpeg_set_quality(q, TRUE), JDCT_ISLOW, standard Huffman tables, JFIF APP0 -- the defaults cv::imencode uses) on the
WHOLE FILE, byte for byte, on the cases of tests/jpeg_cases.py: 8 x 8, 16 x 8, 24 x 16, 13 x 11, 64 x 48 and a batch of five 64 x 48 images; noise, a smooth field,
all 0, all 255, black / white; qualities 10, 50, 75, 100; 24 x 16 with stride 40.  What cv::imencode adds beyond libjpeg's defaults is not pinned here (no OpenCV)."""
import io

import numpy as np
import pytest

from tests import jpeg_cases as J


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_plan")
    return J.build_pin(tmp), tmp


@pytest.fixture(scope="module")
def plan_files(pin):
    """the pin program's file for every image of every case, in one run"""
    exe, tmp = pin
    cases = J.cases()
    jobs = [(g, g.shape[1], q, g.shape[0], J.roomy(g.shape[1], g.shape[0])) for _, imgs, q, _ in cases for g in imgs]
    res = J.run_pin(exe, jobs, tmp)
    out, at = [], 0
    for _, imgs, _, _ in cases:
        out.append(res[at:at + len(imgs)])
        at += len(imgs)
    return cases, out


def pillow_file(gray, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(gray, np.uint8), "L").save(b, "JPEG", quality=quality)
    return b.getvalue()


def test_the_cases_are_the_ones_named():
    cases = J.cases()
    assert len(cases) == (len(J.SHAPES) * len(J.CONTENTS) + 1) * len(J.QUALITIES)
    assert {(imgs.shape[2], imgs.shape[1]) for _, imgs, _, _ in cases} == set(J.SHAPES)
    assert max(imgs.shape[0] for _, imgs, _, _ in cases) == J.BATCH and all(imgs.shape[1] <= 48 and imgs.shape[2] <= 64 for _, imgs, _, _ in cases)
    batch = [imgs for name, imgs, _, _ in cases if name.startswith("batch")][0]
    assert len({g.tobytes() for g in batch}) == J.BATCH                    # five DIFFERENT images


def test_fixture_equals_a_fresh_pillow_run():
    fresh = J.image_sets()
    f = J.fixture()
    assert {k[4:] for k in f if k.startswith("img_")} == set(fresh)
    for name, imgs in fresh.items():
        assert np.array_equal(f["img_" + name], imgs), name
        for q in J.QUALITIES:
            for i, g in enumerate(imgs):
                assert f[f"jpg_{name}_q{q}_{i}"].tobytes() == pillow_file(g, q), (name, q, i)


def test_fixtures_hold_a_stuffed_ff00_and_a_zrl():
    stuffed = zrl = eob = 0
    for _, imgs, _, files in J.cases():
        for g, data in zip(imgs, files):
            syms, st = J.scan_symbols(data, g.shape[1], g.shape[0])
            stuffed += st > 0
            zrl += 0xF0 in syms
            eob += 0x00 in syms
    print(f"files with a stuffed FF 00: {stuffed}, with ZRL: {zrl}, with EOB: {eob}")
    assert stuffed >= 1 and zrl >= 1 and eob >= 1


def test_header_equals_pillow_whole_file_byte_for_byte(plan_files):
    cases, out = plan_files
    differing = n = 0
    for (name, imgs, q, files), res in zip(cases, out):
        for (st, sz, buf), ref in zip(res, files):
            got = buf[:sz].tobytes()
            n += 1
            d = abs(len(got) - len(ref)) + sum(a != b for a, b in zip(got, ref))
            differing += d
            assert st == J.OK and d == 0, (name, sz, len(ref))
            assert got[:J.HEADER_BYTES] == ref[:J.HEADER_BYTES] and (buf[J.roomy(imgs.shape[2], imgs.shape[1]):] == 0xA5).all()
    print(f"{n} files against Pillow: {differing} differing bytes")
    assert differing == 0


def test_pillow_decodes_every_output_to_the_size_given(plan_files):
    from PIL import Image
    cases, out = plan_files
    for (name, imgs, q, _), res in zip(cases, out):
        for g, (st, sz, buf) in zip(imgs, res):
            im = Image.open(io.BytesIO(buf[:sz].tobytes()))
            im.load()
            assert im.size == (g.shape[1], g.shape[0]) and im.mode == "L", name
            if q == 100:                                                    # (a sanity bound only: quality 100 keeps every pixel within a few grey levels)
                assert np.abs(np.asarray(im).astype(int) - g.astype(int)).max() <= 8, name


def test_stride_above_width(pin):
    exe, tmp = pin
    (w, h), stride = J.STRIDE_CASE
    f = J.fixture()
    for content in J.CONTENTS:
        g = f[f"img_{content}_{w}x{h}"][0]
        padded = np.full((h, stride), 0xA5, np.uint8)
        padded[:, :w] = g
        for q in J.QUALITIES:
            assert J.pin_file(exe, tmp, padded, q, width=w) == f[f"jpg_{content}_{w}x{h}_q{q}_0"].tobytes(), (content, q)


@pytest.mark.parametrize("r", [0, 5, 8, None])
def test_zero_from_row_equals_the_image_with_those_rows_zeroed(pin, r):
    """None: r = h, no row blanked"""
    exe, tmp = pin
    f = J.fixture()
    for name in ("noise_13x11", "smooth_64x48", "white_24x16", "pattern_16x8"):
        g = f["img_" + name][0]
        row = g.shape[0] if r is None else r
        blank = g.copy()
        blank[row:] = 0
        for q in (50, 100):
            got = J.pin_file(exe, tmp, g, q, zero_from_row=row)
            assert got == J.pin_file(exe, tmp, blank, q) == pillow_file(blank, q), (name, q, row)


def test_a_capacity_one_byte_short_truncates_and_nothing_is_written_past_it(pin):
    exe, tmp = pin
    for name, imgs, q, files in J.cases():
        if not name.startswith(("noise_64x48", "zeros_8x8", "smooth_13x11")):
            continue
        g, ref = imgs[0], files[0]
        (st, sz, buf), (st1, sz1, buf1) = J.run_pin(exe, [(g, g.shape[1], q, g.shape[0], len(ref)), (g, g.shape[1], q, g.shape[0], len(ref) - 1)], tmp)
        assert st == J.OK and sz == len(ref) and buf[:sz].tobytes() == ref and (buf[len(ref):] == 0xA5).all(), name      # the exact capacity fits
        assert st1 == J.TRUNCATED and sz1 == 0 and (buf1[len(ref) - 1:] == 0xA5).all(), name


def test_library_entry_equals_the_pin_program(omni, plan_files):
    """omni_jpeg_encode_host / omni_jpeg_header (the header compiled by g++ into libomni_hip.so) through ctypes: the same bytes, the same statuses, the refusals"""
    c = omni.capi
    cases, out = plan_files
    for (name, imgs, q, _), res in zip(cases, out):
        for g, (st, sz, buf) in zip(imgs, res):
            status, data = c.jpeg_encode_host(g, q)
            assert status == st == c.JPEG_OK and data == buf[:sz].tobytes(), name
            assert c.jpeg_header(g.shape[1], g.shape[0], q) == data[:c.JPEG_HEADER_BYTES]
    g = np.ascontiguousarray(J.fixture()["img_noise_8x8"][0])
    size = len(c.jpeg_encode_host(g, 75)[1])
    assert c.jpeg_encode_host(g, 75, capacity=size)[0] == c.JPEG_OK and c.jpeg_encode_host(g, 75, capacity=size - 1) == (c.JPEG_TRUNCATED, b"")
    padded = np.full((g.shape[0], 40), 0xA5, np.uint8)
    padded[:, :g.shape[1]] = g
    assert c.jpeg_encode_host(padded, 75, width=g.shape[1]) == c.jpeg_encode_host(g, 75)
    import ctypes as C
    L = c.lib()
    buf, size, status = np.empty(4096, np.uint8), C.c_int64(), C.c_int()
    p, o = g.ctypes.data, buf.ctypes.data

    def call(stride=8, w=8, h=8, zfr=8, cap=4096):
        return L.omni_jpeg_encode_host(p, stride, w, h, 75, zfr, o, cap, C.byref(size), C.byref(status))
    assert call() == c.OK
    for kw, word in (({"w": 0}, b"outside 1..65535"), ({"h": 65536}, b"outside 1..65535"), ({"stride": 7}, b"stride"), ({"cap": c.JPEG_HEADER_BYTES + 1}, b"capacity"),
                     ({"zfr": 9}, b"zero_from_row")):
        assert call(**kw) == c.ERR_INVALID and word in L.omni_last_error(), kw
    assert L.omni_jpeg_header(0, 8, 75, o) == c.ERR_INVALID and L.omni_jpeg_header(8, 8, 75, None) == c.ERR_INVALID
