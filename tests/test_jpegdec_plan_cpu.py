"""CPU gate of the JPEG decoder's arithmetic (csrc/jpeg_dec_plan.h, what csrc/jpeg_dec.hip runs lane-wise): built with g++ into tests/cpp/jpegdec_plan_pin.cpp and
held to Pillow (libjpeg-turbo, JDCT_ISLOW; Image.draft('L') for colour files = libjpeg's JCS_GRAYSCALE, the first component alone) on EVERY PIXEL of the
fixtures of tests/jpegdec_cases.py: gray 8 x 8, 17 x 13, 96 x 64 at q 5 / 75 / 100, noise at q 100, an optimised DHT, 160 x 120, colour 4:2:0 / 4:2:2 / 4:4:4,
640 x 480, two files with restart intervals (HOST), one progressive file (UNSUPPORTED).  The parallel scheme (decode_planned_host with both switches off, the CPU stand-in for the
kernels) equals the sequential decoder at S = 128, 256, 1024, 4096 and really crosses the relaxation; both agree on truncated and byte-flipped scans, and the same
program runs clean under -fsanitize=address,undefined.  cv::imdecode itself is not pinned here (no OpenCV)."""
import io

import numpy as np
import pytest

from tests import jpegdec_cases as J


@pytest.fixture(scope="module")
def pin(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpegdec_plan")
    return J.build_pin(tmp), tmp


@pytest.fixture(scope="module")
def decoded(pin):
    """name -> {0 (sequential) or S: the pin program's result}, in one run"""
    exe, tmp = pin
    names = J.names()
    modes = [0] + J.PARALLEL_S
    res = J.run_pin(exe, [(J.file_of(n), S, 0) for S in modes for n in names], tmp)
    return {n: {S: res[k * len(names) + i] for k, S in enumerate(modes)} for i, n in enumerate(names)}


@pytest.fixture(scope="module")
def mutated(pin):
    """[(what, file, sequential result, parallel S = 128, parallel S = 1024)]"""
    exe, tmp = pin
    muts = J.mutations()
    res = J.run_pin(exe, [(data, S, 0) for _, data in muts for S in (0, 128, 1024)], tmp)
    return [(what, data, res[3 * k], res[3 * k + 1], res[3 * k + 2]) for k, (what, data) in enumerate(muts)]


def test_the_cases_are_the_ones_named():
    f = J.fixture()
    assert {k[4:] for k in f if k.startswith("jpg_")} == set(J.SPECS) == {k[4:] for k in f if k.startswith("pix_")}
    for name, (w, h, _, _, _) in J.SPECS.items():
        assert f["pix_" + name].shape == (h, w) and f["pix_" + name].dtype == np.uint8, name
    assert len(J.names(J.HOST)) == 2 and len(J.names(J.UNSUPPORTED)) == 1


def test_fixture_equals_a_fresh_pillow_run():
    from PIL import Image
    for name, (w, h, content, save, _) in J.SPECS.items():
        b = io.BytesIO()
        img = J.make_image(content, w, h)
        Image.fromarray(img, "L" if img.ndim == 2 else "RGB").save(b, "JPEG", **save)
        assert b.getvalue() == J.file_of(name), name
        im = Image.open(io.BytesIO(J.file_of(name)))
        if im.mode != "L":
            im.draft("L", im.size)
        assert im.mode == "L" and np.array_equal(np.asarray(im), J.pixels_of(name)), name


def test_fixtures_hold_what_they_are_named_for():
    """16-bit codes and ZRL in the noise file, a DHT that is not Annex K's in the optimised one, stuffed FF 00 pairs, three components in the colour files"""
    from tests import jpeg_cases as E
    noise = J.file_of("noise_96x64_q100")
    syms, stuffed = E.scan_symbols(noise, 96, 64)
    tabs, _ = E._huff_tables(noise)
    assert 0xF0 in syms and stuffed > 0 and max(ln for ln, _ in tabs[0x10]) == 16
    assert E._huff_tables(J.file_of("opt_96x64_q75"))[0] != E._huff_tables(J.file_of("gray_96x64_q75"))[0]
    for name, sampling in (("color_80x48_420", 0x22), ("color_72x40_422", 0x21), ("color_80x48_444", 0x11)):
        d = J.file_of(name)
        p = d.index(b"\xff\xc0")
        assert d[p + 9] == 3 and d[p + 11] == sampling and d[p + 14] == 0x11 and d[p + 17] == 0x11, name


def test_sequential_decoder_equals_pillow_on_every_pixel(decoded):
    differing = n = 0
    for name in J.names(J.OK) + J.names(J.HOST):
        r = decoded[name][0]
        d = int((r["pixels"] != J.pixels_of(name)).sum()) if r["pixels"] is not None and r["pixels"].shape == J.pixels_of(name).shape else -1
        n += 1
        differing += abs(d)
        assert r["status"] == J.SPECS[name][4] and d == 0, (name, r["status"], d)
    print(f"{n} files against Pillow: {differing} differing pixels")
    assert differing == 0


@pytest.mark.parametrize("S", J.PARALLEL_S)
def test_parallel_scheme_equals_the_sequential_decoder(decoded, S):
    for name in J.names(J.OK) + J.names(J.HOST):
        r, seq = decoded[name][S], decoded[name][0]
        d = int((r["pixels"] != seq["pixels"]).sum()) + int((r["pixels"] != J.pixels_of(name)).sum())
        assert r["status"] == seq["status"] == J.SPECS[name][4] and d == 0, (name, S, r["status"], d)
        if J.SPECS[name][4] == J.OK:
            assert r["S"] == S and r["n_sub"] >= 1 and 0 <= r["rounds"] <= r["n_sub"], (name, r)


def test_the_relaxation_is_really_crossed(decoded):
    """the 96 x 64 q 100 file at S = 128: most first-pass exit states are wrong, and the fixed point takes many rounds -- but never more than N.  The figures
    DESIGN.md 0.2e quotes are the ones asserted here (name, S) -> (subsequences, wrong after the first pass, rounds)"""
    quoted = {("gray_96x64_q100", 128): (372, 362, 81), ("gray_96x64_q100", 256): (186, 176, 41), ("gray_96x64_q100", 1024): (47, 35, 10),
              ("gray_160x120_q75", 1024): (44, 0, 1), ("gray_640x480_q75", 128): (915, 98, 5)}
    for (name, S), want in quoted.items():
        q = decoded[name][S]
        print(f"{name}, S={S}: {q['n_sub']} subsequences, {q['wrong']} wrong after the first pass, fixed point after {q['rounds']} rounds")
        assert (q["n_sub"], q["wrong"], q["rounds"]) == want and q["rounds"] <= q["n_sub"], (name, S)
    r = decoded["gray_96x64_q100"][128]
    assert r["n_sub"] > 256 and r["wrong"] > 0 and 1 < r["rounds"] <= r["n_sub"]
    assert decoded["gray_160x120_q75"][128]["n_sub"] > 256                      # more subsequences than the entropy kernel's workgroup has lanes


def test_a_limit_on_the_subsequences_doubles_their_length(pin):
    exe, tmp = pin
    name = "gray_96x64_q100"
    free, capped = J.run_pin(exe, [(J.file_of(name), 128, 0), (J.file_of(name), 128, 100)], tmp)
    assert free["S"] == 128 and free["n_sub"] > 100
    assert capped["S"] == 512 and 50 < capped["n_sub"] <= 100 and np.array_equal(capped["pixels"], J.pixels_of(name))


def test_classification_of_every_fixture(decoded):
    for name, (w, h, _, _, cls) in J.SPECS.items():
        r = decoded[name][0]
        assert r["status"] == cls, (name, r["status"])
        if cls == J.UNSUPPORTED:
            assert r["pixels"] is None
        else:
            assert (r["w"], r["h"]) == (w, h)


def test_files_that_are_no_files_are_corrupt(pin):
    exe, tmp = pin
    good = J.file_of("gray_8x8_q75")
    sof = good.index(b"\xff\xc0")
    sos = good.index(b"\xff\xda")
    cases = [b"", b"\xff\xd8", b"not a jpeg at all", good[:sof], good[:sos], good[:sos + 4], good[:2] + good[sof:], b"\xff\xd8\xff\xd9"]
    for r in J.run_pin(exe, [(c, 0, 0) for c in cases] + [(c, 128, 0) for c in cases], tmp):
        assert r["status"] == J.CORRUPT and (r["pixels"] is None or not r["pixels"].any())
    twelve = bytearray(good)
    twelve[sof + 4] = 12
    lossless = good[:sof + 1] + b"\xc3" + good[sof + 2:]
    arith = good[:sof + 1] + b"\xc9" + good[sof + 2:]
    for r in J.run_pin(exe, [(bytes(twelve), 0, 0), (lossless, 0, 0), (arith, 0, 0)], tmp):
        assert r["status"] == J.UNSUPPORTED


def test_mutated_scans_both_decoders_agree_and_finish(mutated):
    kinds = {J.OK: 0, J.CORRUPT: 0}
    for what, _, seq, p128, p1024 in mutated:
        for par in (p128, p1024):
            assert par["status"] == seq["status"] and np.array_equal(par["pixels"], seq["pixels"]), what
        assert seq["status"] in kinds and seq["pixels"].shape == (64, 96), what
        if seq["status"] == J.CORRUPT:
            assert not seq["pixels"].any(), what
        kinds[seq["status"]] += 1
    print(f"{len(mutated)} mutations: {kinds[J.CORRUPT]} CORRUPT, {kinds[J.OK]} decoded without an error")
    assert len(mutated) == J.N_MUTATIONS and kinds[J.CORRUPT] >= 10


def test_the_same_program_runs_clean_under_asan_and_ubsan(tmp_path_factory, mutated, decoded):
    """a stand-alone binary with its own main: nothing loaded into python is sanitised.  Every mutation and every fixture, both decoders; the results equal the
    plain build's"""
    tmp = tmp_path_factory.mktemp("jpegdec_san")
    exe = J.build_pin(tmp, sanitize=True)
    jobs = [(data, S, 0) for _, data, *_ in mutated for S in (0, 128, 1024)] + [(J.file_of(n), S, 0) for n in J.names() for S in (0, 128)]
    res = J.run_pin(exe, jobs, tmp)
    for k, (what, _, seq, p128, p1024) in enumerate(mutated):
        for got, want in zip(res[3 * k:3 * k + 3], (seq, p128, p1024)):
            assert got["status"] == want["status"] and np.array_equal(got["pixels"], want["pixels"]), what
    at = 3 * len(mutated)
    for n in J.names():
        for S in (0, 128):
            assert res[at]["status"] == decoded[n][S]["status"], n
            at += 1
