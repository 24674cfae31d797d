"""Unstuffing on the device (csrc/jpeg_dec.hip jpegdec_unstuff_kernel; OMNI_JPEGDEC_UNSTUFF_DEV = 1: the scans go over the bus as they stand in the files and one
workgroup per tile of 4096 raw bytes removes the stuffing and the restart markers) -- equality everywhere: the kernel alone against the byte-wise pass of the g++
build on seeded strings, seam patterns and a scan of 4 799 restart markers; through the handle, every fixture with the switch on against the switch off, the CPU
stand-ins, Pillow's committed pixels and the sequential decoder, with neither, either or both of the _WGS switches; files with fill bytes; a mixed batch; the 40
mutations; switch 0 against the variable unset; the key-frame unit."""
import numpy as np
import pytest

from tests import jpegdec_cases as J
from tests import jpegdec_plain_cases as P
from tests import jpegdec_restart_cases as R
from tests import jpegdec_unstuff_cases as U

pytestmark = pytest.mark.gpu
differing = P.differing


def set_env(monkeypatch, **env):
    """U=, W=, R=, S=: None unsets"""
    for key, name in (("U", U.U_ENV), ("W", U.W_ENV), ("R", U.R_ENV), ("S", U.S_ENV)):
        if env.get(key) is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(env[key]))


def decode_one(c, ctx, w, h, data, capacity=0):
    """one file on a handle of its own -> dict(status, pixels, stats, guarded, unstuff, unstuff_guarded, uploaded)"""
    dec = c.JpegDec(ctx, w, h, 1, capacity or max(len(data), 1024))
    try:
        (st,), pix = dec([data])
        (rounds, n_sub, bits), (chunks,), (seam_rounds, seam_changed) = dec.last_stats(1)[0], dec.last_chunks(1), dec.last_seam(1)[0]
        assert dec.last_guard_ok and dec.unstuff_guard_ok()
        return dict(status=st, pixels=pix[0].copy(), stats=dict(n_sub=n_sub, subseq_bits=bits, rounds=rounds, chunks=chunks, seam_rounds=seam_rounds, seam_changed=seam_changed),
                    guarded=dec.guarded, unstuff=dec.last_unstuff(), unstuff_guarded=dec.unstuff_guarded, uploaded=dec.last_ms()[2])
    finally:
        dec.close()


def dropped(c, data):
    """(raw bytes, clean bytes) of the file's scan as the survey of the g++ build sees it"""
    lo, hi = J.scan_range(data)
    t = c.jpeg_unstuff_tiled_host(data[lo:hi])
    assert t["raw_end"] == hi - lo
    return t["raw_end"], t["surveyed_clean"]


def on_against_off(c, ctx, monkeypatch, w, h, data, env, capacity=0):
    """the same file on a handle with the switch on and on one with it off, everything else in `env` -> (on, off), compared"""
    set_env(monkeypatch, U=1, **env)
    on = decode_one(c, ctx, w, h, data, capacity)
    set_env(monkeypatch, U=None, **env)
    off = decode_one(c, ctx, w, h, data, capacity)
    assert on["status"] == off["status"] and differing(on["pixels"], off["pixels"]) == 0 and on["stats"] == off["stats"] and on["guarded"] == off["guarded"], (on, off)
    assert off["unstuff"] == (0, 0, 0) and off["unstuff_guarded"] == 0 and on["unstuff_guarded"] == 1
    return on, off


# ---- the kernel alone -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_alone_equals_the_byte_wise_pass(omni, ctx):
    c = omni.capi
    T = c.jpeg_unstuff_tile_bytes()
    lo, hi = J.scan_range(R.file_of(R.MANY))
    cases = U.strings(T) + [(R.MANY, R.file_of(R.MANY)[lo:hi])]
    assert (hi - lo) // T >= 20
    for what, s in cases:
        want, n, rst = c.jpeg_unstuff_host(s)
        got, k = c.jpegdec_unstuff_dev(ctx, s)                     # (the entry itself refuses a byte written behind the padding: the block was all 0xA5)
        assert k == n and len(got) == n + U.PAD and np.array_equal(got, want) and not got[n:].any(), (what, k, n, int((got[:min(k, n)] != want[:min(k, n)]).sum()))
    assert len(rst) == 4799


# ---- through the handle -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", J.names(J.OK))
def test_ok_fixtures_switch_on_equal_switch_off_the_stand_ins_and_pillow(omni, ctx, monkeypatch, name):
    c = omni.capi
    w, h = J.SPECS[name][:2]
    data = J.file_of(name)
    set_env(monkeypatch)
    default = c.config_value(U.S_ENV)
    st_h, pix_h = c.jpeg_decode_host(data)
    assert st_h == c.JPEGDEC_OK and np.array_equal(pix_h, J.pixels_of(name))
    raw, clean = dropped(c, data)
    for W in (None, 3):
        for S in (None, 128):
            on, _ = on_against_off(c, ctx, monkeypatch, w, h, data, dict(W=W, S=S))
            if W:
                st_e, pix_e, emu = c.jpeg_decode_plain_parallel_host(data, S or default, W)
                want = {k: emu[k] for k in P.STAT_KEYS}
            else:
                st_e, pix_e, emu = c.jpeg_decode_parallel_host(data, S or default)
                want = dict(n_sub=emu["n_sub"], subseq_bits=emu["subseq_bits"], rounds=emu["rounds"], chunks=1, seam_rounds=0, seam_changed=0)
            d = differing(on["pixels"], J.pixels_of(name)) + differing(on["pixels"], pix_h) + differing(on["pixels"], pix_e)
            print(f"{name} W={W} S={S}: {on['stats']}, unstuff {on['unstuff']}, differing pixels {d}")
            assert on["status"] == st_e == c.JPEGDEC_OK and d == 0 and on["stats"] == want, (name, W, S, on["stats"], want)
            assert on["unstuff"] == (1, raw, clean) and raw >= clean, (name, on["unstuff"], raw, clean)


@pytest.mark.parametrize("name", R.names())
def test_restart_fixtures_switch_on_equal_switch_off_the_stand_in_and_pillow(omni, ctx, monkeypatch, name):
    c = omni.capi
    w, h = R.SPECS[name][:2]
    data = R.file_of(name)
    set_env(monkeypatch)
    S = c.config_value(U.S_ENV)
    raw, clean = dropped(c, data)
    on, _ = on_against_off(c, ctx, monkeypatch, w, h, data, dict(R=3))
    st_e, pix_e, emu = c.jpeg_decode_restart_parallel_host(data, S, 3)
    d = differing(on["pixels"], R.pixels_of(name)) + differing(on["pixels"], c.jpeg_decode_host(data)[1]) + differing(on["pixels"], pix_e)
    print(f"{name}: {on['stats']}, unstuff {on['unstuff']}, differing pixels {d}")
    assert R.plannable(name, 3) and on["status"] == st_e == c.JPEGDEC_OK and d == 0
    assert {k: on["stats"][k] for k in ("n_sub", "subseq_bits", "chunks", "rounds")} == {k: emu[k] for k in ("n_sub", "subseq_bits", "chunks", "rounds")}, (on["stats"], emu)
    assert on["unstuff"] == (1, raw, clean) and raw - clean >= 2 * (R.SPECS[name][4] - 1)
    if name == R.MUTATED:                                          # without the restart switch the file is the host's: nothing for the device to unstuff
        on, _ = on_against_off(c, ctx, monkeypatch, w, h, data, dict())
        assert on["status"] == c.JPEGDEC_HOST and differing(on["pixels"], R.pixels_of(name)) == 0 and on["unstuff"] == (0, 0, 0)


@pytest.mark.parametrize("extra", [1, 3])
def test_fill_bytes_in_front_of_every_restart_marker(omni, ctx, monkeypatch, extra):
    c = omni.capi
    data = U.fill_file(extra)
    raw, clean = dropped(c, data)
    on, _ = on_against_off(c, ctx, monkeypatch, 96, 64, data, dict(R=3))
    assert on["status"] == c.JPEGDEC_OK and differing(on["pixels"], R.pixels_of(U.FILL)) == 0
    assert on["unstuff"] == (1, raw, clean) and raw - clean == dropped(c, R.file_of(U.FILL))[0] - clean + 7 * extra


def test_a_mixed_batch_with_all_three_switches_on(omni, ctx, monkeypatch):
    """one batch on one handle: a spread file, a file of one subsequence, a planned restart file, a file above the capacity (HOST) and a truncated mutation (CORRUPT,
    zeros) -- forwards, reversed (another layout of the block: stale clean areas), and twice back to back without a synchronisation (the pinned block's reuse)"""
    c = omni.capi
    set_env(monkeypatch, U=1, W=3, R=3)
    S = c.config_value(U.S_ENV)
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
    assert emu[0]["chunks"] == 3 and (emu[1]["n_sub"], emu[1]["chunks"]) == (1, 1)
    want_chunks = [3, 1, c.jpeg_decode_restart_parallel_host(files[2], S, 3)[2]["chunks"], 0, None]      # (the truncated file: whatever ran of it)
    want_seam = [(emu[0]["seam_rounds"], emu[0]["seam_changed"]), (0, 0), (0, 0), (0, 0), None]
    n = len(files)
    dec = c.JpegDec(ctx, 96, 64, n, capacity)
    try:
        for order in (list(range(n)), list(range(n))[::-1]):
            status, pix = dec([files[i] for i in order])
            chunks, seam = dec.last_chunks(n), dec.last_seam(n)
            assert status == [want[i][0] for i in order] and dec.last_guard_ok and dec.guarded == 3 and dec.unstuff_guard_ok() and dec.unstuff_guarded == 1, (order, status)
            assert all(differing(pix[k], want[i][1]) == 0 for k, i in enumerate(order)), order
            assert all(want_chunks[i] is None or chunks[k] == want_chunks[i] for k, i in enumerate(order)), (order, chunks)
            assert all(want_seam[i] is None or seam[k] == want_seam[i] for k, i in enumerate(order)), (order, seam)
            pictures, raw, clean = dec.last_unstuff()
            assert pictures == 4 and raw > clean                   # all but the file above the capacity: the truncated file's scan is unstuffed too
        out = ctx.to_device(np.full(n * 64 * 96, 0xA5, np.uint8))
        stat = ctx.to_device(np.full(n, -1, np.int32))
        try:
            dec.enqueue_host(files[:3], out, 96, stat)
            dec.enqueue_host(files[3:], out + 3 * 64 * 96, 96, stat + 12)
            got = ctx.from_device(out, (n, 64, 96), np.uint8)
            assert [int(v) for v in ctx.from_device(stat, (n,), np.int32)] == [s for s, _ in want]
            assert all(differing(got[i], want[i][1]) == 0 for i in range(n)) and dec.guards_ok() and dec.unstuff_guard_ok()
            assert dec.last_unstuff()[0] == 1
        finally:
            ctx.free(out)
            ctx.free(stat)
    finally:
        dec.close()


def test_the_mutations_switch_on_equal_switch_off(omni, ctx, monkeypatch):
    c = omni.capi
    files = [data for _, data in J.mutations()]
    runs = []
    for on in (1, None):
        set_env(monkeypatch, U=on, S=128)
        dec = c.JpegDec(ctx, 96, 64, len(files), 4096)
        try:
            runs.append(dec(files) + (dec.last_stats(len(files)), dec.last_unstuff()))
            assert dec.last_guard_ok and dec.unstuff_guard_ok()
        finally:
            dec.close()
    (st_1, pix_1, stats_1, un_1), (st_0, pix_0, stats_0, un_0) = runs
    assert st_1 == st_0 and np.array_equal(pix_1, pix_0) and stats_1 == stats_0 and set(st_0) == {c.JPEGDEC_OK, c.JPEGDEC_CORRUPT}
    assert un_1[0] > 0 and un_1[1] >= un_1[2] and un_0 == (0, 0, 0), (un_1, un_0)


def test_switch_0_is_the_handle_with_the_variable_unset(omni, ctx, monkeypatch):
    c = omni.capi
    names = ["gray_96x64_q75", "noise_96x64_q100", "opt_96x64_q75", "gray_96x64_q5"]
    files = [J.file_of(n) for n in names] + [R.file_of("rows_gray_96x64_q75")]
    runs = []
    for on in (None, "0"):
        set_env(monkeypatch, U=on, R=3)
        dec = c.JpegDec(ctx, 96, 64, len(files), 16384)
        try:
            status, pix = dec(files)
            runs.append((status, pix, dec.last_stats(len(files)), dec.last_chunks(len(files)), dec.last_ms()[2], dec.guarded, dec.last_unstuff()))
            assert dec.last_guard_ok and dec.unstuff_guard_ok() and dec.unstuff_guarded == 0
        finally:
            dec.close()
    a, b = runs
    assert a[0] == b[0] == [c.JPEGDEC_OK] * len(files) and np.array_equal(a[1], b[1]) and a[2:] == b[2:] and a[6] == (0, 0, 0) and a[5] == 2
    assert all(np.array_equal(a[1][i], J.pixels_of(n)) for i, n in enumerate(names))
    set_env(monkeypatch, U=1, R=3)                                 # ... and the switch on uploads the raw scans in the clean ones' place
    dec = c.JpegDec(ctx, 96, 64, len(files), 16384)
    try:
        status, pix = dec(files)
        pictures, raw, clean = dec.last_unstuff()
        assert status == a[0] and np.array_equal(pix, a[1]) and pictures == len(files) and (raw, clean) == tuple(map(sum, zip(*[dropped(c, f) for f in files])))
        assert dec.last_ms()[2] > raw > clean and a[4] > clean
    finally:
        dec.close()
    set_env(monkeypatch, U=2)
    with pytest.raises(c.OmniError, match=U.U_ENV):
        c.JpegDec(ctx, 96, 64, 1, 4096)


def test_key_frame_unit_fed_plain_files_with_the_switch_on_equals_the_unit_with_every_switch_unset(omni, ctx, monkeypatch):
    """a mono unit, network-size frames decoded straight into its input block: the same files with OMNI_JPEGDEC_UNSTUFF_DEV=1 + OMNI_JPEGDEC_PLAIN_WGS=8 and with
    every switch unset -- every frame OK, omni_cam_get_input and every field of omni_cam_result bit-identical"""
    from oracle import mobilenetvlad_ref as V
    from oracle import superpoint_ref as SP
    from omni_swarm_amd import synth
    c = omni.capi
    n, cap = R.CAM_FRAMES, 4
    keys = ("kps_xy", "n_kps", "desc", "scores", "global_desc", "match_up", "match_down", "match_dist", "n_matches")
    (comp, mean), vw = synth.pca(), V.synth_weights()
    files = [R.file_of(f"cam_plain_{k}") for k in range(n)]
    vctx = c.Context(0)
    sp = c.SuperPoint(ctx, SP.synth_weights(0), comp, mean, R.CAM_W, R.CAM_H, 0.015, 100, c.PREC_F16, cap)
    vlad = c.MobileNetVLAD(vctx, vw, V.layer_specs(), V.N_CLUSTERS, V.FEAT_DIM, V.OUT_DIM, R.CAM_W, R.CAM_H, cap)
    runs = []
    try:
        for env in (dict(), dict(U=1, W=8)):
            set_env(monkeypatch, **env)
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
    print(f"plain files, unstuffed on the device, W = 8: input block {int((got_in != ref_in).sum())} bytes differ, fields with other bits: {moved}; key points {ref['n_kps'].tolist()}")
    assert ref_st == got_st == [c.JPEGDEC_OK] * n
    assert np.array_equal(got_in, ref_in) and ref_in.shape == (n, R.CAM_H, R.CAM_W) and all(np.array_equal(ref_in[k], c.jpeg_decode_host(files[k])[1]) for k in range(n))
    assert (ref["n_kps"] >= 20).all() and moved == []
