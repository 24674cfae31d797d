"""Restart-interval files through the JPEG decode kernels (csrc/jpeg_dec.hip with OMNI_JPEGDEC_RESTART_WGS = W >= 1: the intervals of a picture spread over at most W
workgroups of the entropy kernel, the DC scan segmented at every interval) against the committed Pillow pixels (tests/golden/jpegdec_restart_cases.npz), the g++
build of the sequential decoder, and the CPU stand-in (omni_jpeg_decode_restart_parallel_host: same subsequences, same length, same rounds): every fixture at
W in {1, 3, 8} and S in {default, 128} (the file of 4800 intervals at W in {3, 8}: one workgroup cannot hold it); that file's fallback at W = 1; mixed batches
on one handle; the switch left off; the mutations and the one documented divergence from the host decoder (tests/jpegdec_restart_cases.py); the key-frame unit
fed restart files."""
import numpy as np
import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_restart_cases as R

pytestmark = pytest.mark.gpu
S_ENV, W_ENV = "OMNI_JPEGDEC_SUBSEQ_BITS", "OMNI_JPEGDEC_RESTART_WGS"


@pytest.fixture(scope="module")
def reference(omni):
    """name -> pixels of the g++ build's sequential decoder (status HOST), equal to Pillow's; computed once"""
    out = {}
    for name in R.names():
        st, pix = omni.capi.jpeg_decode_host(R.file_of(name))
        assert st == R.HOST and np.array_equal(pix, R.pixels_of(name)), name
        out[name] = pix
    return out


def differing(a, b) -> int:
    return int((np.asarray(a) != np.asarray(b)).sum()) if np.asarray(a).shape == np.asarray(b).shape else -1


# every fixture at every W the plan can take: the 4800-interval file at W = 1 is the fallback test's (below)
@pytest.mark.parametrize("name,W", [(n, W) for n in R.names() for W in R.WGS if R.plannable(n, W)])
def test_kernels_equal_the_stand_in_the_cpu_build_and_pillow(omni, ctx, reference, monkeypatch, name, W):
    c = omni.capi
    w, h = R.SPECS[name][:2]
    data = R.file_of(name)
    default = c.config_value(S_ENV)
    monkeypatch.setenv(W_ENV, str(W))
    for S in (None, 128):
        if S:
            monkeypatch.setenv(S_ENV, str(S))
        dec = c.JpegDec(ctx, w, h, 1, max(len(data), 1024))
        (st,), pix = dec([data])
        (rounds, n_sub, bits), (chunks,) = dec.last_stats(1)[0], dec.last_chunks(1)
        dec.close()
        st_e, pix_e, emu = c.jpeg_decode_restart_parallel_host(data, S or default, W)
        d = differing(pix[0], reference[name]) + differing(pix[0], R.pixels_of(name)) + differing(pix[0], pix_e)
        print(f"{name} W={W} S={bits}: {n_sub} subsequences in {chunks} chunks, {rounds} rounds, differing pixels {d}")
        assert st == st_e == c.JPEGDEC_OK and d == 0 and dec.last_guard_ok, (name, W, S, st, d)
        assert (n_sub, bits, rounds, chunks) == (emu["n_sub"], emu["subseq_bits"], emu["rounds"], emu["chunks"]), (name, W, S)
        if S == 128 and name == "rows_noise_96x64_q100":
            assert rounds > 0                                  # an interval of dozens of subsequences needs relaxation rounds
        if W == 8 and name == "rows_gray_640x480_q75":
            assert chunks > 1                                  # more than one workgroup decoded a share of the picture
        if name == R.MANY:
            assert n_sub >= 4800 and chunks == W               # more than a thousand intervals in every workgroup's share


def test_more_intervals_than_a_workgroup_holds_fall_back_or_spread(omni, ctx, reference, monkeypatch):
    """4800 intervals: one workgroup (W = 1) holds 4096 subsequences and every interval costs one -- HOST, decoded on the calling thread; W = 2 plans it"""
    c = omni.capi
    data = R.file_of(R.MANY)
    for W, want in ((1, c.JPEGDEC_HOST), (2, c.JPEGDEC_OK)):
        monkeypatch.setenv(W_ENV, str(W))
        dec = c.JpegDec(ctx, 640, 480, 1, len(data))
        (st,), pix = dec([data])
        stats, (chunks,) = dec.last_stats(1)[0], dec.last_chunks(1)
        dec.close()
        st_e, pix_e, emu = c.jpeg_decode_restart_parallel_host(data, c.config_value(S_ENV), W)
        print(f"{R.MANY} W={W}: status {st}, (rounds, subsequences, bits) {stats}, {chunks} chunks")
        assert st == st_e == want and dec.last_guard_ok
        assert differing(pix[0], reference[R.MANY]) == 0 and differing(pix[0], R.pixels_of(R.MANY)) == 0 and differing(pix[0], pix_e) == 0
        assert (stats[1], stats[2], stats[0], chunks) == (emu["n_sub"], emu["subseq_bits"], emu["rounds"], emu["chunks"]) and chunks == (0 if W == 1 else 2)


def test_a_mixed_batch_restart_plain_host_and_truncated(omni, ctx, reference, monkeypatch):
    """one batch: a restart file (OK by the kernels), a file without restart markers (OK, the one-chunk path), a file above the capacity (HOST) and the truncated
    mutation (CORRUPT, zeros); the same handle again in reverse order; then two enqueues back to back without a synchronisation"""
    c = omni.capi
    monkeypatch.setenv(W_ENV, "3")
    big = J.file_of("noise_96x64_q100")
    cut = R.mutations()[0][1]
    names = ["rows_gray_96x64_q75", "blk1_gray_96x64_q75"]
    files = [R.file_of(names[0]), J.file_of("gray_96x64_q75"), big, cut, R.file_of(names[1])]
    capacity = 4096
    assert len(big) > capacity >= max(len(f) for f in files if f is not big)
    want = [(c.JPEGDEC_OK, reference[names[0]]), (c.JPEGDEC_OK, J.pixels_of("gray_96x64_q75")), (c.JPEGDEC_HOST, J.pixels_of("noise_96x64_q100")),
            (c.JPEGDEC_CORRUPT, np.zeros((64, 96), np.uint8)), (c.JPEGDEC_OK, reference[names[1]])]
    want_chunks = [0 if f is big else c.jpeg_decode_restart_parallel_host(f, c.config_value(S_ENV), 3)[2]["chunks"] for f in files]      # (the stand-in knows no capacity)
    assert want_chunks[1:4] == [1, 0, 0] and want_chunks[0] > 1 and want_chunks[4] > 1
    n = len(files)
    dec = c.JpegDec(ctx, 96, 64, len(files), capacity)
    try:
        for order in (list(range(n)), list(range(n))[::-1]):
            status, pix = dec([files[i] for i in order])
            chunks = dec.last_chunks(n)
            assert status == [want[i][0] for i in order] and dec.last_guard_ok, (order, status)
            assert all(differing(pix[k], want[i][1]) == 0 for k, i in enumerate(order)), order
            assert [chunks[order.index(i)] for i in range(n)] == want_chunks, chunks
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


def test_the_switch_left_off_decodes_restart_files_on_the_host(omni, ctx, reference, monkeypatch):
    c = omni.capi
    monkeypatch.delenv(W_ENV, raising=False)
    assert c.config_value(W_ENV) == 0
    for name in ("rows_gray_96x64_q75", "blk3_color_72x40_422"):
        w, h = R.SPECS[name][:2]
        dec = c.JpegDec(ctx, w, h, 1, 8192)
        (st,), pix = dec([R.file_of(name)])
        stats, chunks = dec.last_stats(1)[0], dec.last_chunks(1)
        dec.close()
        assert st == c.JPEGDEC_HOST and differing(pix[0], reference[name]) == 0 and dec.last_guard_ok and stats == (0, 0, 0) and chunks == [0], name


def test_mutations_and_the_documented_divergence(omni, ctx, monkeypatch):
    """fewer markers than the picture needs: CORRUPT, as the host decoder says.  An interval that lost its last bytes: the host decoder reads on into the next
    interval and returns a picture (HOST); the kernels and their stand-in bound every interval to its own bits: CORRUPT, zeros"""
    c = omni.capi
    muts = R.mutations()
    for W in (1, 8):
        monkeypatch.setenv(W_ENV, str(W))
        monkeypatch.setenv(S_ENV, "128")
        dec = c.JpegDec(ctx, 96, 64, len(muts), 4096)
        status, pix = dec([data for _, data, _, _ in muts])
        dec.close()
        assert dec.last_guard_ok
        for i, (what, data, st_host, st_restart) in enumerate(muts):
            assert c.jpeg_decode_host(data)[0] == st_host and c.jpeg_decode_restart_parallel_host(data, 128, W)[0] == st_restart, what
            assert status[i] == st_restart == c.JPEGDEC_CORRUPT and not pix[i].any(), (what, W, status[i])


def test_key_frame_unit_fed_restart_files_equals_the_unit_fed_plain_files(omni, ctx, monkeypatch):
    """a mono unit, network-size frames decoded straight into its input block: restart-file versions of the frames with the switch on against the files without
    restart markers of the same images (switch off) -- every frame OK, omni_cam_get_input and every field of omni_cam_result bit-identical"""
    from oracle import mobilenetvlad_ref as V
    from oracle import superpoint_ref as SP
    from omni_swarm_amd import synth
    c = omni.capi
    n, cap = R.CAM_FRAMES, 4
    keys = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")
    (comp, mean), vw = synth.pca(), V.synth_weights()
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, SP.synth_weights(0), comp, mean, R.CAM_W, R.CAM_H, 0.015, 100, c.PREC_F16, cap)
    vlad = c.MobileNetVLAD(vctx, vw, V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, R.CAM_W, R.CAM_H, cap)
    runs = []
    try:
        for kind, W in (("plain", None), ("rows", "4")):
            if W:
                monkeypatch.setenv(W_ENV, W)
            else:
                monkeypatch.delenv(W_ENV, raising=False)
            cam = c.Cam(sp, vlad, cap, V.OUT_DIM, mono=True)                                       # (the unit makes its decoder at its first JPEG enqueue)
            try:
                cam.set_active(n)
                cam.enqueue_jpeg_host(None, [R.file_of(f"cam_{kind}_{k}") for k in range(n)])
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
    print(f"restart files: input block {int((got_in != ref_in).sum())} bytes differ, fields with other bits: {moved}; key points {ref['n_kps'].tolist()}")
    assert ref_st == got_st == [c.JPEGDEC_OK] * n
    assert np.array_equal(got_in, ref_in) and ref_in.shape == (n, R.CAM_H, R.CAM_W) and all(np.array_equal(ref_in[k], c.jpeg_decode_host(R.file_of(f"cam_rows_{k}"))[1]) for k in range(n))
    assert (ref["n_kps"] >= 20).all() and moved == []
