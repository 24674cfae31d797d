// csrc/jpeg_plan.h compiled by g++ into libomni_hip.so: omni_jpeg_header / omni_jpeg_encode_host give host callers and the tests the bytes of the GPU stage
// (jpeg.hip) without a GPU -- and "what a host encoder would cost" on one thread.
#include "jpeg_plan.h"

namespace omni {
void set_error(const char* fmt, ...);
}

extern "C" int omni_jpeg_header(int width, int height, int quality, uint8_t* out_host) {
    if (!out_host || width < 1 || height < 1 || width > 65535 || height > 65535) {
        omni::set_error("omni_jpeg_header: null output or %dx%d outside 1..65535", width, height);
        return OMNI_ERR_INVALID;
    }
    return omni::jp::jpeg_header(width, height, quality, out_host) == JP_HEADER_BYTES ? OMNI_OK : OMNI_ERR_INVALID;
}

extern "C" int omni_jpeg_encode_host(const uint8_t* gray, int stride, int width, int height, int quality, int zero_from_row, uint8_t* out, int64_t capacity,
                                     int64_t* size, int* status) {
    if (!gray || !out || !size || !status) { omni::set_error("null argument"); return OMNI_ERR_INVALID; }
    if (width < 1 || height < 1 || width > 65535 || height > 65535) { omni::set_error("omni_jpeg_encode_host: %dx%d outside 1..65535", width, height); return OMNI_ERR_INVALID; }
    if (stride < width) { omni::set_error("omni_jpeg_encode_host: stride %d for an image %d wide", stride, width); return OMNI_ERR_INVALID; }
    if (capacity < JP_HEADER_BYTES + 2) {
        omni::set_error("omni_jpeg_encode_host: a capacity of %lld bytes, the header and EOI alone take %d", (long long)capacity, JP_HEADER_BYTES + 2);
        return OMNI_ERR_INVALID;
    }
    if (zero_from_row < 0 || zero_from_row > height) { omni::set_error("omni_jpeg_encode_host: zero_from_row %d outside [0, %d]", zero_from_row, height); return OMNI_ERR_INVALID; }
    const int st = omni::jp::jpeg_encode_host(gray, stride, width, height, quality, zero_from_row, out, capacity, size);
    if (st < 0) { omni::set_error("omni_jpeg_encode_host: bad arguments"); return OMNI_ERR_INVALID; }
    *status = st;
    return OMNI_OK;
}
