// csrc/jpeg_dec_plan.h compiled by g++ into libomni_hip.so: omni_jpegdec_classify / omni_jpeg_decode_host / omni_jpeg_decode_parallel_host /
// omni_jpeg_decode_restart_parallel_host / omni_jpeg_decode_plain_parallel_host (one stand-in for the kernels under three settings of a handle's switches) give
// host callers and the tests the pixels of the GPU stage (jpeg_dec.hip) without a GPU -- and "what a host decoder would cost" on one thread.
#include <climits>

#include "jpeg_dec_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}

extern "C" int omni_jpegdec_classify(const uint8_t* file, int64_t size, int* width, int* height) {
    omni::jd::Desc d;
    const int st = omni::jd::parse(file, size, &d);
    if (width) *width = d.w;
    if (height) *height = d.h;
    return st;
}

static int decode_args(const uint8_t* file, int64_t size, uint8_t* out, int stride, int* width, int* height, int* status) {
    if (!file || !out || !width || !height || !status || size < 0) { omni::set_error("null argument"); return OMNI_ERR_INVALID; }
    omni::jd::Desc d;
    omni::jd::parse(file, size, &d);
    if (stride < d.w) { omni::set_error("omni_jpeg_decode_host: stride %d for a picture %d wide", stride, d.w); return OMNI_ERR_INVALID; }
    return OMNI_OK;
}

extern "C" int omni_jpeg_decode_host(const uint8_t* file, int64_t size, uint8_t* out, int stride, int* width, int* height, int* status) {
    const int rc = decode_args(file, size, out, stride, width, height, status);
    if (rc) return rc;
    *status = omni::jd::jpeg_decode_host(file, size, out, stride, stride, INT_MAX, width, height);
    return OMNI_OK;
}

// ---- the CPU stand-in for the kernels (jd::decode_planned_host) under the switches of each of its three entries ------------------------------------------------------
// what all three take, checked once
static int planned_args(const char* who, const uint8_t* file, int64_t size, int subseq_bits, uint8_t* out, int stride, int* width, int* height, int* status) {
    const int rc = decode_args(file, size, out, stride, width, height, status);
    if (rc) return rc;
    if (subseq_bits < JD_MIN_SUBSEQ_BITS || subseq_bits > JD_MAX_SUBSEQ_BITS || (subseq_bits & (subseq_bits - 1))) {
        omni::set_error("%s: %d bits per subsequence, a power of two in [%d, %d]", who, subseq_bits, JD_MIN_SUBSEQ_BITS, JD_MAX_SUBSEQ_BITS);
        return OMNI_ERR_INVALID;
    }
    return OMNI_OK;
}
// ... and the workgroup count of the two entries that have one
static int wgs_args(const char* who, int wgs, int max_wgs, int max_subseq) {
    if (wgs >= 1 && wgs <= max_wgs && max_subseq >= 1) return OMNI_OK;
    omni::set_error("%s: %d workgroups of at most %d subsequences, expected 1..%d and >= 1", who, wgs, max_subseq, max_wgs);
    return OMNI_ERR_INVALID;
}

extern "C" int omni_jpeg_decode_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, uint8_t* out, int stride, int* width, int* height, int* status,
                                              int* stats) {
    const int rc = planned_args("omni_jpeg_decode_parallel_host", file, size, subseq_bits, out, stride, width, height, status);
    if (rc) return rc;
    omni::jd::PlannedStats ps;
    *status = omni::jd::decode_planned_host(file, size, (uint32_t)subseq_bits, 0u, 0u, 0xffffffffu, out, stride, stride, INT_MAX, width, height, &ps);
    if (!stats) return OMNI_OK;
    stats[0] = (int)ps.n_sub; stats[1] = (int)ps.subseq_bits; stats[2] = (int)ps.chunk_rounds;
    stats[3] = (int)omni::jd::wrong_after_first(file, size, (uint32_t)subseq_bits, 0xffffffffu);
    return OMNI_OK;
}

extern "C" int omni_jpeg_decode_restart_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, int restart_wgs, int max_subseq, uint8_t* out, int stride,
                                                      int* width, int* height, int* status, int* stats) {
    const char* who = "omni_jpeg_decode_restart_parallel_host";
    int rc = planned_args(who, file, size, subseq_bits, out, stride, width, height, status);
    if (rc || (rc = wgs_args(who, restart_wgs, JD_MAX_RESTART_WGS, max_subseq))) return rc;
    omni::jd::PlannedStats ps;
    *status = omni::jd::decode_planned_host(file, size, (uint32_t)subseq_bits, (uint32_t)restart_wgs, 0u, (uint32_t)max_subseq, out, stride, stride, INT_MAX, width,
                                            height, &ps);
    if (stats) { stats[0] = (int)ps.n_sub; stats[1] = (int)ps.subseq_bits; stats[2] = (int)ps.n_chunks; stats[3] = (int)ps.chunk_rounds; }
    return OMNI_OK;
}

extern "C" int omni_jpeg_decode_plain_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, int plain_wgs, int max_subseq, uint8_t* out, int stride,
                                                    int* width, int* height, int* status, int* stats) {
    const char* who = "omni_jpeg_decode_plain_parallel_host";
    int rc = planned_args(who, file, size, subseq_bits, out, stride, width, height, status);
    if (rc || (rc = wgs_args(who, plain_wgs, JD_MAX_PLAIN_WGS, max_subseq))) return rc;
    omni::jd::PlannedStats ps;
    *status = omni::jd::decode_planned_host(file, size, (uint32_t)subseq_bits, 0u, (uint32_t)plain_wgs, (uint32_t)max_subseq, out, stride, stride, INT_MAX, width, height,
                                            &ps);
    if (stats) {
        stats[0] = (int)ps.n_sub; stats[1] = (int)ps.subseq_bits; stats[2] = (int)ps.n_chunks; stats[3] = (int)ps.chunk_rounds;
        stats[4] = (int)ps.seam_rounds; stats[5] = (int)ps.seam_changed; stats[6] = (int)ps.seam_chunks;
    }
    return OMNI_OK;
}

// ---- unstuffing by tiles (OMNI_JPEGDEC_UNSTUFF_DEV): the byte-wise pass, and survey + the tile-by-tile stand-in for jpegdec_unstuff_kernel ----------------------
extern "C" int omni_jpeg_unstuff_tile_bytes(void) { return JD_UNSTUFF_TILE; }

extern "C" int64_t omni_jpeg_scan_end(const uint8_t* file, int64_t size, int64_t from) {
    if (!file || size < 0 || from < 0 || from > size) return -1;
    return omni::jd::scan_end(file, size, from);
}

static int unstuff_args(const char* who, const uint8_t* scan, int64_t n, const uint8_t* out, int64_t out_cap, const int64_t* n_clean, const int64_t* rst, int64_t max_rst,
                        const int64_t* n_rst) {
    if (!scan || !out || !n_clean || !n_rst || n < 0 || max_rst < 0 || (max_rst && !rst)) { omni::set_error("%s: null argument", who); return OMNI_ERR_INVALID; }
    if (out_cap < n + JD_SCAN_PAD) { omni::set_error("%s: room for %lld bytes, a scan of %lld needs %lld", who, (long long)out_cap, (long long)n, (long long)(n + JD_SCAN_PAD)); return OMNI_ERR_INVALID; }
    return OMNI_OK;
}

extern "C" int omni_jpeg_unstuff_host(const uint8_t* scan, int64_t n, uint8_t* out, int64_t out_cap, int64_t* n_clean, int64_t* rst, int64_t max_rst, int64_t* n_rst) {
    const int rc = unstuff_args("omni_jpeg_unstuff_host", scan, n, out, out_cap, n_clean, rst, max_rst, n_rst);
    if (rc) return rc;
    *n_clean = omni::jd::unstuff(scan, n, out, max_rst ? rst : nullptr, max_rst, n_rst);
    return OMNI_OK;
}

extern "C" int omni_jpeg_unstuff_tiled_host(const uint8_t* scan, int64_t n, uint8_t* out, int64_t out_cap, int64_t* n_clean, int64_t* rst, int64_t max_rst, int64_t* n_rst,
                                            int64_t* raw_end, int64_t* surveyed_clean, uint32_t* tile_off, int64_t max_tiles, int64_t* n_tiles) {
    const int rc = unstuff_args("omni_jpeg_unstuff_tiled_host", scan, n, out, out_cap, n_clean, rst, max_rst, n_rst);
    if (rc) return rc;
    if (!raw_end || !surveyed_clean || !tile_off || !n_tiles || max_tiles < n / JD_UNSTUFF_TILE + 1) {
        omni::set_error("omni_jpeg_unstuff_tiled_host: a tile table of %lld entries, a scan of %lld bytes needs %lld", (long long)max_tiles, (long long)n,
                        (long long)(n / JD_UNSTUFF_TILE + 1));
        return OMNI_ERR_INVALID;
    }
    const omni::jd::Survey v = omni::jd::survey(scan, n, tile_off, max_tiles, max_rst ? rst : nullptr, max_rst);
    memset(out, 0xA5, (size_t)out_cap);                                                     // (the tiles and the padding are all that is written)
    *n_clean = omni::jd::unstuff_tiled_host(scan, v, tile_off, out);
    *n_rst = v.n_rst; *raw_end = v.raw_end; *surveyed_clean = v.n_clean; *n_tiles = v.n_tiles;
    return OMNI_OK;
}
