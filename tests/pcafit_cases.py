"""Shared inputs of the PCA-fit tests (tests/test_pca_plan_cpu.py, tests/test_gpu_pcafit.py, ...): synthetic operands of omni_pcafit_enqueue_rows_dev /
omni_pca_moments_host -- raw_desc [B][M][256], norm_partial [B][8][256], n_kps [B] -- and the numpy restatement of a row."""
import numpy as np

DIM, SEGS = 256, 8


def make_pass(seed: int, n_kps, max_num: int, zero_channel_images=(), garbage: bool = True) -> dict:
    """One pass's operands.  raw is N(0, 1); norm_partial holds what sp_chan_sumsq_kernel would: the image's per-channel sums of squares cut into eight
    key-point segments (so the rows are the channel-normalised descriptors).  Rows at or beyond n_kps[b] hold NaN / huge values (`garbage`): they do not exist.
    zero_channel_images: images whose channel 5 is zero at every key point -- 0/0 in every row of the image"""
    rng = np.random.default_rng(seed)
    n_kps = np.asarray(n_kps, np.int32)
    B = len(n_kps)
    raw = rng.normal(size=(B, max_num, DIM)).astype(np.float32)
    for b in zero_channel_images:
        raw[b, :, 5] = 0.0
    part = np.zeros((B, SEGS, DIM), np.float32)
    for b in range(B):
        n = int(n_kps[b])
        per = (n + SEGS - 1) // SEGS
        for s in range(SEGS):
            seg = raw[b, min(s * per, n):min(s * per + per, n)].astype(np.float64)
            part[b, s] = (seg * seg).sum(0).astype(np.float32)
        if garbage and n < max_num:
            raw[b, n:] = np.where(rng.random((max_num - n, DIM)) < 0.5, np.float32(np.nan), np.float32(3e38))
    return {"raw": raw, "part": part, "n_kps": n_kps, "max_num": max_num}


def rows_of(p) -> np.ndarray:
    """numpy's restatement of the rows of a pass, in stream order, float32 [n][256] -- skipped rows included (they hold a non-finite element)"""
    out = []
    for b in range(len(p["n_kps"])):
        ss = np.float32(0)
        for s in range(SEGS):
            ss = (ss + p["part"][b, s]).astype(np.float32)
        norm = np.sqrt(ss).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append((p["raw"][b, :int(p["n_kps"][b])] / norm).astype(np.float32))
    return np.concatenate(out) if out else np.zeros((0, DIM), np.float32)


def same_moments(a, b) -> list:
    """the fields in which two capi.PcaMoments differ bit for bit"""
    bad = [k for k in ("n", "skipped") if getattr(a, k) != getattr(b, k)]
    bad += [k for k in ("s", "S") if getattr(a, k).tobytes() != getattr(b, k).tobytes()]
    return bad
