// csrc/jpeg_dec_plan.h compiled by g++ into libomni_hip.so: omni_jpegdec_classify / omni_jpeg_decode_host / omni_jpeg_decode_parallel_host /
// omni_jpeg_decode_restart_parallel_host / omni_jpeg_decode_plain_parallel_host (the stand-ins for a handle that spreads restart-interval files, or files without
// a restart interval, over workgroups) give host callers and the tests the pixels of the GPU stage (jpeg_dec.hip) without a GPU -- and "what a host decoder would cost" on one thread.
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

extern "C" int omni_jpeg_decode_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, uint8_t* out, int stride, int* width, int* height, int* status,
                                              int* stats) {
    const int rc = decode_args(file, size, out, stride, width, height, status);
    if (rc) return rc;
    if (subseq_bits < JD_MIN_SUBSEQ_BITS || subseq_bits > JD_MAX_SUBSEQ_BITS || (subseq_bits & (subseq_bits - 1))) {
        omni::set_error("omni_jpeg_decode_parallel_host: %d bits per subsequence, a power of two in [%d, %d]", subseq_bits, JD_MIN_SUBSEQ_BITS, JD_MAX_SUBSEQ_BITS);
        return OMNI_ERR_INVALID;
    }
    omni::jd::ParallelStats ps;
    *status = omni::jd::jpeg_decode_parallel_host(file, size, (uint32_t)subseq_bits, 0xffffffffu, out, stride, stride, INT_MAX, width, height, &ps);
    if (stats) { stats[0] = (int)ps.n_sub; stats[1] = (int)ps.subseq_bits; stats[2] = (int)ps.rounds; stats[3] = (int)ps.wrong_after_first; }
    return OMNI_OK;
}

extern "C" int omni_jpeg_decode_restart_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, int restart_wgs, int max_subseq, uint8_t* out, int stride,
                                                      int* width, int* height, int* status, int* stats) {
    const int rc = decode_args(file, size, out, stride, width, height, status);
    if (rc) return rc;
    if (subseq_bits < JD_MIN_SUBSEQ_BITS || subseq_bits > JD_MAX_SUBSEQ_BITS || (subseq_bits & (subseq_bits - 1))) {
        omni::set_error("omni_jpeg_decode_restart_parallel_host: %d bits per subsequence, a power of two in [%d, %d]", subseq_bits, JD_MIN_SUBSEQ_BITS,
                        JD_MAX_SUBSEQ_BITS);
        return OMNI_ERR_INVALID;
    }
    if (restart_wgs < 1 || restart_wgs > JD_MAX_RESTART_WGS || max_subseq < 1) {
        omni::set_error("omni_jpeg_decode_restart_parallel_host: %d workgroups of at most %d subsequences, expected 1..%d and >= 1", restart_wgs, max_subseq,
                        JD_MAX_RESTART_WGS);
        return OMNI_ERR_INVALID;
    }
    omni::jd::RestartStats rs;
    *status = omni::jd::jpeg_decode_restart_parallel_host(file, size, (uint32_t)subseq_bits, (uint32_t)restart_wgs, (uint32_t)max_subseq, out, stride, stride, INT_MAX,
                                                          width, height, &rs);
    if (stats) { stats[0] = (int)rs.n_sub; stats[1] = (int)rs.subseq_bits; stats[2] = (int)rs.n_chunks; stats[3] = (int)rs.rounds; }
    return OMNI_OK;
}

extern "C" int omni_jpeg_decode_plain_parallel_host(const uint8_t* file, int64_t size, int subseq_bits, int plain_wgs, int max_subseq, uint8_t* out, int stride,
                                                    int* width, int* height, int* status, int* stats) {
    const int rc = decode_args(file, size, out, stride, width, height, status);
    if (rc) return rc;
    if (subseq_bits < JD_MIN_SUBSEQ_BITS || subseq_bits > JD_MAX_SUBSEQ_BITS || (subseq_bits & (subseq_bits - 1))) {
        omni::set_error("omni_jpeg_decode_plain_parallel_host: %d bits per subsequence, a power of two in [%d, %d]", subseq_bits, JD_MIN_SUBSEQ_BITS,
                        JD_MAX_SUBSEQ_BITS);
        return OMNI_ERR_INVALID;
    }
    if (plain_wgs < 1 || plain_wgs > JD_MAX_PLAIN_WGS || max_subseq < 1) {
        omni::set_error("omni_jpeg_decode_plain_parallel_host: %d workgroups of at most %d subsequences, expected 1..%d and >= 1", plain_wgs, max_subseq,
                        JD_MAX_PLAIN_WGS);
        return OMNI_ERR_INVALID;
    }
    omni::jd::PlainStats ps;
    *status = omni::jd::jpeg_decode_plain_parallel_host(file, size, (uint32_t)subseq_bits, (uint32_t)plain_wgs, (uint32_t)max_subseq, out, stride, stride, INT_MAX,
                                                        width, height, &ps);
    if (stats) {
        stats[0] = (int)ps.n_sub; stats[1] = (int)ps.subseq_bits; stats[2] = (int)ps.n_chunks; stats[3] = (int)ps.chunk_rounds;
        stats[4] = (int)ps.seam_rounds; stats[5] = (int)ps.seam_changed; stats[6] = (int)ps.seam_chunks;
    }
    return OMNI_OK;
}
