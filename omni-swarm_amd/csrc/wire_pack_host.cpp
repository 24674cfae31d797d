// csrc/wire_plan.h compiled by g++ into libomni_hip.so: omni_wire_pack_host gives host callers and the tests the bytes of the GPU stage (wire_pack.hip) without a
// GPU -- and "what packing on the calling thread would cost".  omni_wire_packet_capacity / omni_wire_table_ints are the plan's two sizes.
#include "wire_plan.h"

namespace omni {
void set_error(const char* fmt, ...);

// what both entries refuse before they touch anything; NULL when the call may go ahead
const char* wire_pack_refusal(int n_images, int max_num, int desc_dim, int global_dim) {
    if (n_images < 1 || n_images > 65535) return "n_images outside 1..65535";
    if (max_num < 1 || max_num > WP_MAX_NUM) return "max_num outside 1..1024";
    if (desc_dim != WP_DESC_DIM) return "a descriptor length other than 64";
    if (global_dim != WP_GLOBAL_DIM) return "a global descriptor length other than 4096";
    return nullptr;
}

// ... and what the two entries of the whole descriptor refuse on top of that (wire_pack_image_kernel reads a file's row as dwords)
const char* wire_pack_image_refusal(int with_image, const void* jpeg, const void* jpeg_sizes, const void* jpeg_status, int64_t jpeg_capacity) {
    if (jpeg_capacity < 0 || jpeg_capacity > WP_MAX_JPEG_CAPACITY) return "jpeg_capacity outside 0..2^30";
    if (jpeg_capacity % 4 != 0) return "a jpeg_capacity that is not a multiple of 4: a file's row would not be 4-byte aligned";
    if (with_image ? !(jpeg && jpeg_sizes && jpeg_status) : (jpeg || jpeg_sizes || jpeg_status))
        return "the three JPEG pointers are null exactly when with_image is 0";
    return nullptr;
}
}  // namespace omni

extern "C" int64_t omni_wire_image_capacity(int max_num, int64_t jpeg_capacity) {
    return max_num < 1 || max_num > WP_MAX_NUM || jpeg_capacity < 0 || jpeg_capacity > WP_MAX_JPEG_CAPACITY || jpeg_capacity % 4 != 0 ? 0 : omni::wp::whole_capacity(max_num, jpeg_capacity);
}

extern "C" int omni_wire_pack_image_host(int n_images, int max_num, int desc_dim, int global_dim, int with_features, int with_image, const float* kps_xy, const int* n_kps,
                                         const float* desc, const float* norm2d, const float* l3d, const uint8_t* flag, const float* global,
                                         const omni_wire_image_meta* meta, const uint8_t* jpeg, const int* jpeg_sizes, const int* jpeg_status, int64_t jpeg_capacity,
                                         int image_width, int image_height, uint8_t* packets_out, int* sizes_out) {
    if (!kps_xy || !n_kps || !desc || !norm2d || !l3d || !flag || !global || !meta || !packets_out || !sizes_out) {
        omni::set_error("omni_wire_pack_image_host: null argument");
        return OMNI_ERR_INVALID;
    }
    const char* why = omni::wire_pack_refusal(n_images, max_num, desc_dim, global_dim);
    if (!why) why = omni::wire_pack_image_refusal(with_image, jpeg, jpeg_sizes, jpeg_status, jpeg_capacity);
    if (why) {
        omni::set_error("omni_wire_pack_image_host: %s (n_images %d, max_num %d, desc_dim %d, global_dim %d, with_image %d, jpeg_capacity %lld)", why, n_images, max_num,
                        desc_dim, global_dim, with_image, (long long)jpeg_capacity);
        return OMNI_ERR_INVALID;
    }
    const int64_t cap = omni::wp::whole_capacity(max_num, jpeg_capacity);
    for (int g = 0; g < n_images; ++g) {
        const size_t at = (size_t)g * max_num;
        omni::wp::pack_whole_image_host(max_num, with_features, with_image, kps_xy + at * 2, n_kps[g], desc + at * WP_DESC_DIM, norm2d + at * 2, l3d + at * 3, flag + at,
                                        global + (size_t)g * WP_GLOBAL_DIM, meta[g], with_image ? jpeg + (size_t)g * jpeg_capacity : nullptr,
                                        with_image ? jpeg_sizes[g] : 0, with_image ? jpeg_status[g] : 0, jpeg_capacity, image_width, image_height,
                                        packets_out + (size_t)g * cap, sizes_out + 2 * (size_t)g);
    }
    return OMNI_OK;
}

extern "C" int64_t omni_wire_packet_capacity(int max_num) { return max_num < 1 || max_num > WP_MAX_NUM ? 0 : omni::wp::capacity(max_num); }

extern "C" int omni_wire_table_ints(int max_num) { return max_num < 1 || max_num > WP_MAX_NUM ? 0 : omni::wp::table_ints(max_num); }

extern "C" int omni_wire_pack_host(int n_images, int max_num, int desc_dim, int global_dim, int send_all_features, const float* kps_xy, const int* n_kps,
                                   const float* desc, const float* norm2d, const float* l3d, const uint8_t* flag, const float* global,
                                   const omni_wire_image_meta* meta, uint8_t* packets_out, int* table_out) {
    if (!kps_xy || !n_kps || !desc || !norm2d || !l3d || !flag || !global || !meta || !packets_out || !table_out) {
        omni::set_error("omni_wire_pack_host: null argument");
        return OMNI_ERR_INVALID;
    }
    if (const char* why = omni::wire_pack_refusal(n_images, max_num, desc_dim, global_dim)) {
        omni::set_error("omni_wire_pack_host: %s (n_images %d, max_num %d, desc_dim %d, global_dim %d)", why, n_images, max_num, desc_dim, global_dim);
        return OMNI_ERR_INVALID;
    }
    const int64_t cap = omni::wp::capacity(max_num);
    const int te = omni::wp::table_ints(max_num);
    for (int g = 0; g < n_images; ++g) {
        const size_t at = (size_t)g * max_num;
        omni::wp::pack_image_host(max_num, send_all_features, kps_xy + at * 2, n_kps[g], desc + at * WP_DESC_DIM, norm2d + at * 2, l3d + at * 3, flag + at,
                                  global + (size_t)g * WP_GLOBAL_DIM, meta[g], packets_out + (size_t)g * cap, table_out + (size_t)g * te);
    }
    return OMNI_OK;
}
