"""Files without a restart interval through the chunk, seam and write kernels (csrc/jpeg_dec.hip with OMNI_JPEGDEC_PLAIN_WGS = W >= 2: a picture's subsequences
over min(W, n_sub) workgroups that relax on their own, a seam relaxation over the whole picture, one subsequence per lane in the write pass) against the committed
Pillow pixels (tests/golden/jpegdec_cases.npz), the g++ build of the sequential decoder, and the CPU stand-in (omni_jpeg_decode_plain_parallel_host: same
subsequences, same length, same rounds, same seam): every OK fixture at W in {2, 3, 8} and S in {default, 128}; a picture of more subsequences than one workgroup
holds; a mixed batch with both switches on; the 40 mutations against the switch-off kernels; switch 0 and 1 against the variable unset; the key-frame unit."""
import numpy as np
import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_plain_cases as P
from tests import jpegdec_restart_cases as R

pytestmark = pytest.mark.gpu
differing = P.differing


@pytest.fixture(scope="module")
def reference(omni):
    """name -> pixels of the g++ build's sequential decoder (status OK), equal to Pillow's; computed once"""
    out = {}
    for name in J.names(J.OK):
        st, pix = omni.capi.jpeg_decode_host(J.file_of(name))
        assert st == P.OK and np.array_equal(pix, J.pixels_of(name)), name
        out[name] = pix
    return out


def decode_one(c, ctx, w, h, data, capacity=0):
    """one file on a handle of its own -> (status, pixels, stats in the stand-in's names, guards looked at)"""
    dec = c.JpegDec(ctx, w, h, 1, capacity or max(len(data), 1024))
    try:
        (st,), pix = dec([data])
        (rounds, n_sub, bits), (chunks,), (seam_rounds, seam_changed) = dec.last_stats(1)[0], dec.last_chunks(1), dec.last_seam(1)[0]
        assert dec.last_guard_ok
        return st, pix[0], dict(n_sub=n_sub, subseq_bits=bits, rounds=rounds, chunks=chunks, seam_rounds=seam_rounds, seam_changed=seam_changed), dec.guarded
    finally:
        dec.close()


@pytest.mark.parametrize("name,W", [(n, W) for n in J.names(J.OK) for W in P.WGS])
def test_kernels_equal_the_stand_in_the_cpu_build_and_pillow(omni, ctx, reference, monkeypatch, name, W):
    c = omni.capi
    w, h = J.SPECS[name][:2]
    data = J.file_of(name)
    default = c.config_value(P.S_ENV)
    monkeypatch.setenv(P.W_ENV, str(W))
    for S in (None, 128):
        if S:
            monkeypatch.setenv(P.S_ENV, str(S))
        st, pix, got, guarded = decode_one(c, ctx, w, h, data)
        st_e, pix_e, emu = c.jpeg_decode_plain_parallel_host(data, S or default, W)
        d = differing(pix, reference[name]) + differing(pix, J.pixels_of(name)) + differing(pix, pix_e)
        print(f"{name} W={W} S={got['subseq_bits']}: {got}, differing pixels {d}")
        assert st == st_e == c.JPEGDEC_OK and d == 0 and guarded == 3, (name, W, S, st, d, guarded)
        assert got == {k: emu[k] for k in P.STAT_KEYS}, (name, W, S, got, emu)
        if S == 128 and W == 8 and name == "noise_96x64_q100":
            assert got["seam_rounds"] >= 2                       # a repair that crosses chunks
        if W == 8 and name == "gray_640x480_q75":
            assert got["chunks"] == 8                            # eight workgroups decoded a share of the picture


def test_more_subsequences_than_one_workgroup_holds(omni, ctx, monkeypatch):
    """256 x 256 noise at quality 100, S = 128: between 4096 and 8192 subsequences.  Switch off: S is doubled; W = 2: S stays, two chunks"""
    c = omni.capi
    data = P.big_noise_file(c)
    st_h, pix_h = c.jpeg_decode_host(data)
    assert st_h == c.JPEGDEC_OK and 4096 < c.jpeg_decode_plain_parallel_host(data, 128, 2)[2]["n_sub"] <= 8192
    monkeypatch.setenv(P.S_ENV, "128")
    monkeypatch.delenv(P.W_ENV, raising=False)
    st, pix, got, guarded = decode_one(c, ctx, P.BIG_W, P.BIG_H, data)
    assert st == c.JPEGDEC_OK and differing(pix, pix_h) == 0 and (got["subseq_bits"], got["chunks"], guarded) == (256, 1, 2) and got["n_sub"] <= 4096, got
    monkeypatch.setenv(P.W_ENV, "2")
    st, pix, got, guarded = decode_one(c, ctx, P.BIG_W, P.BIG_H, data)
    emu = c.jpeg_decode_plain_parallel_host(data, 128, 2)[2]
    print(f"noise {P.BIG_W}x{P.BIG_H} W=2: {got}")
    assert st == c.JPEGDEC_OK and differing(pix, pix_h) == 0 and guarded == 3
    assert got["subseq_bits"] == 128 and got["n_sub"] > 4096 and got["chunks"] == 2 and got == {k: emu[k] for k in P.STAT_KEYS}, (got, emu)


def test_a_mixed_batch_with_both_switches_on(omni, ctx, monkeypatch):
    """one batch on one handle: a spread file, a file of one subsequence (a flat picture, written by the library's host encoder), a restart file (planned), a
    file above the capacity (HOST) and a truncated mutation (CORRUPT, zeros) -- forwards, reversed, and twice back to back without a synchronisation"""
    c = omni.capi
    monkeypatch.setenv(P.W_ENV, "3")
    monkeypatch.setenv(P.R_ENV, "3")
    S = c.config_value(P.S_ENV)
    big = J.file_of("noise_96x64_q100")
    cut = [data for what, data in J.mutations() if what.startswith("cut at") and c.jpeg_decode_host(data)[0] == c.JPEGDEC_CORRUPT][0]
    st_f, flat = c.jpeg_encode_host(np.full((64, 96), 97, np.uint8), 5)
    assert st_f == 0
    files = [J.file_of("gray_96x64_q100"), flat, R.file_of("rows_gray_96x64_q75"), big, cut]
    capacity = 6400
    assert len(big) > capacity >= max(len(f) for f in files if f is not big)
    want = [(c.JPEGDEC_OK, J.pixels_of("gray_96x64_q100")), (c.JPEGDEC_OK, c.jpeg_decode_host(flat)[1]), (c.JPEGDEC_OK, R.pixels_of("rows_gray_96x64_q75")),
            (c.JPEGDEC_HOST, J.pixels_of("noise_96x64_q100")), (c.JPEGDEC_CORRUPT, np.zeros((64, 96), np.uint8))]
    emu = [c.jpeg_decode_plain_parallel_host(f, S, 3)[2] for f in files[:2]]
    assert emu[0]["chunks"] == 3 and emu[0]["seam_changed"] > 0 and (emu[1]["n_sub"], emu[1]["chunks"]) == (1, 1)
    want_chunks = [3, 1, c.jpeg_decode_restart_parallel_host(files[2], S, 3)[2]["chunks"], 0, None]      # (the truncated file: whatever ran of it)
    want_seam = [(emu[0]["seam_rounds"], emu[0]["seam_changed"]), (0, 0), (0, 0), (0, 0), None]
    assert want_chunks[2] > 1
    n = len(files)
    dec = c.JpegDec(ctx, 96, 64, n, capacity)
    try:
        for order in (list(range(n)), list(range(n))[::-1]):
            status, pix = dec([files[i] for i in order])
            chunks, seam = dec.last_chunks(n), dec.last_seam(n)
            assert status == [want[i][0] for i in order] and dec.last_guard_ok and dec.guarded == 3, (order, status)
            assert all(differing(pix[k], want[i][1]) == 0 for k, i in enumerate(order)), order
            assert all(want_chunks[i] is None or chunks[k] == want_chunks[i] for k, i in enumerate(order)), (order, chunks)
            assert all(want_seam[i] is None or seam[k] == want_seam[i] for k, i in enumerate(order)), (order, seam)
        out = ctx.to_device(np.full(n * 64 * 96, 0xA5, np.uint8))
        stat = ctx.to_device(np.full(n, -1, np.int32))
        try:
            dec.enqueue_host(files[:3], out, 96, stat)
            dec.enqueue_host(files[3:], out + 3 * 64 * 96, 96, stat + 12)
            got = ctx.from_device(out, (n, 64, 96), np.uint8)
            assert [int(v) for v in ctx.from_device(stat, (n,), np.int32)] == [s for s, _ in want]
            assert all(differing(got[i], want[i][1]) == 0 for i in range(n)) and dec.guards_ok()
        finally:
            ctx.free(out)
            ctx.free(stat)
    finally:
        dec.close()


def test_the_mutations_equal_the_switch_off_kernels(omni, ctx, monkeypatch):
    c = omni.capi
    files = [data for _, data in J.mutations()]
    monkeypatch.setenv(P.S_ENV, "128")
    runs = []
    for W in (None, "3"):
        if W:
            monkeypatch.setenv(P.W_ENV, W)
        else:
            monkeypatch.delenv(P.W_ENV, raising=False)
        dec = c.JpegDec(ctx, 96, 64, len(files), 4096)
        try:
            runs.append(dec(files) + (dec.last_chunks(len(files)),))
            assert dec.last_guard_ok
        finally:
            dec.close()
    (st_0, pix_0, ch_0), (st_3, pix_3, ch_3) = runs
    assert st_3 == st_0 and np.array_equal(pix_3, pix_0) and set(st_0) == {c.JPEGDEC_OK, c.JPEGDEC_CORRUPT}
    assert max(ch_0) == 1 and max(ch_3) == 3                                                   # ... and the second run did take the spread path
    for i, data in enumerate(files):
        st_e, pix_e, _ = c.jpeg_decode_plain_parallel_host(data, 128, 3)
        assert st_e == st_3[i] and differing(pix_e, pix_3[i]) == 0, i


def test_switch_0_and_1_are_the_handle_with_the_variable_unset(omni, ctx, monkeypatch):
    c = omni.capi
    names = ["gray_96x64_q75", "noise_96x64_q100", "opt_96x64_q75", "gray_96x64_q5"]
    files = [J.file_of(n) for n in names]
    runs = []
    for W in (None, "0", "1"):
        if W is None:
            monkeypatch.delenv(P.W_ENV, raising=False)
        else:
            monkeypatch.setenv(P.W_ENV, W)
        dec = c.JpegDec(ctx, 96, 64, len(files), 16384)
        try:
            status, pix = dec(files)
            runs.append((status, pix, dec.last_stats(len(files)), dec.last_chunks(len(files)), dec.last_ms()[2]))
            assert dec.last_seam(len(files)) == [(0, 0)] * len(files) and dec.last_guard_ok and dec.guarded == 2      # no state arrays: nothing was allocated
        finally:
            dec.close()
    for status, pix, stats, chunks, uploaded in runs:
        assert status == [c.JPEGDEC_OK] * len(files) and all(np.array_equal(pix[i], J.pixels_of(n)) for i, n in enumerate(names))
        assert (stats, chunks, uploaded) == runs[0][2:] and chunks == [1] * len(files)
    monkeypatch.setenv(P.W_ENV, "65")                                                          # outside the range: the handle is refused
    with pytest.raises(c.OmniError, match=P.W_ENV):
        c.JpegDec(ctx, 96, 64, 1, 4096)


def test_key_frame_unit_fed_plain_files_with_the_switch_on_equals_the_unit_with_it_off(omni, ctx, monkeypatch):
    """a mono unit, network-size frames decoded straight into its input block: the same files with W = 8 and with the switch off -- every frame OK,
    omni_cam_get_input and every field of omni_cam_result bit-identical"""
    from oracle import mobilenetvlad_ref as V
    from oracle import superpoint_ref as SP
    from omni_swarm_amd import synth
    c = omni.capi
    n, cap = R.CAM_FRAMES, 4
    keys = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")
    (comp, mean), vw = synth.pca(), V.synth_weights()
    files = [R.file_of(f"cam_plain_{k}") for k in range(n)]
    assert all(c.jpeg_decode_plain_parallel_host(f, c.config_value(P.S_ENV), 8)[2]["chunks"] == 8 for f in files)      # every frame is spread
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, SP.synth_weights(0), comp, mean, R.CAM_W, R.CAM_H, 0.015, 100, c.PREC_F16, cap)
    vlad = c.MobileNetVLAD(vctx, vw, V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, R.CAM_W, R.CAM_H, cap)
    runs = []
    try:
        for W in (None, "8"):
            if W:
                monkeypatch.setenv(P.W_ENV, W)
            else:
                monkeypatch.delenv(P.W_ENV, raising=False)
            cam = c.Cam(sp, vlad, cap, V.OUT_DIM, mono=True)                                       # (the unit makes its decoder at its first JPEG enqueue)
            try:
                cam.set_active(n)
                cam.enqueue_jpeg_host(None, files)
                res = {k: v.copy() for k, v in cam.wait().items()}
                runs.append((res, cam.get_input(), cam.jpegdec_status()))
            finally:
                cam.close()
    finally:
        sp.close()
        vlad.close()
        vctx.close()
    (ref, ref_in, ref_st), (got, got_in, got_st) = runs
    moved = [k for k in keys if not np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8))]
    print(f"plain files, W = 8: input block {int((got_in != ref_in).sum())} bytes differ, fields with other bits: {moved}; key points {ref['n_kps'].tolist()}")
    assert ref_st == got_st == [c.JPEGDEC_OK] * n
    assert np.array_equal(got_in, ref_in) and ref_in.shape == (n, R.CAM_H, R.CAM_W) and all(np.array_equal(ref_in[k], c.jpeg_decode_host(files[k])[1]) for k in range(n))
    assert (ref["n_kps"] >= 20).all() and moved == []
