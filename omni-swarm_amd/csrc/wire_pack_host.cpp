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
}  // namespace omni

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
