// wire_plan.h -- the bytes one image of a key frame leaves a drone as, stated once: the two packets of host/loop_net_wire.hpp (wire::encode(ImageDescriptorHeader),
// wire::encode(LandmarkDescriptor)), which landmarks LoopNetWire::broadcast_img_desc sends, which images broadcast_fisheye_desc sends, and the packet buffer the
// pack stage fills.  Plain C++ for g++ AND hipcc: wire_pack.hip runs these functions one dword (or, for the header's head, one byte) per lane, wire_pack_host.cpp
// compiles pack_image_host into the library (omni_wire_pack_host, the CPU stand-in), tests/cpp/wire_plan_pin.cpp runs it next to LoopNetWire itself; nothing else
// restates the layout.  loop_net_wire.hpp stays the definition; that pin holds the two together byte for byte.  Bits only: a float travels as its 32 bits, so NaN
// payloads, infinities and -0.0 pass unchanged and there is nothing to round.  Both sides are little-endian machines: a packet dword is __builtin_bswap32 of the value.
//
//   header packet    WP_HEADER_BYTES = 161 + 4 * 4096 = 16545                                   (wire::encode(ImageDescriptorHeader))
//       0  i64 fingerprint "OMNIHDR1"      8  f64 timestamp      16  i32 drone_id      20  i64 msg_id (ZERO here)      28  i64 frame_id
//      36  i32 feature_num                40  i32 direction      44  u8  prevent_adding_db
//      45  7 x f64 pose_drone (xyz, quaternion wxyz)            101  7 x f64 camera_extrinsic  157  i32 4096           161  4096 x f32 image_desc
//   landmark packet  WP_LANDMARK_BYTES = 36 + 28 + 4 + 4 * 64 = 324 = 81 dwords                  (wire::encode(LandmarkDescriptor))
//       0  i64 fingerprint "OMNILMK1"      8  i64 msg_id (ZERO here)   16  i64 header_id (ZERO here)   24  i32 drone_id   28  i32 landmark_id   32  i32 landmark_flag
//      36  f32 landmark_2d_norm x, y      44  f32 landmark_2d x, y     52  f32 landmark_3d x, y, z     64  i32 64         68  64 x f32 feature_descriptor
//   every scalar big-endian, the length member in front of each float array (LCM's rules, as loop_net_wire.hpp states them).
//
//   ids        msg_id of every packet and header_id of the landmark packets are left ZERO: the host numbers a frame's packets in LoopNetWire's own sequence when it
//              takes them (patch_header_id / patch_landmark_ids below), so numbering does not depend on how many units are in flight.
//   record     every other field that is not an array of the unit comes from one omni_wire_image_meta per image: stamp, drone id, frame id, direction,
//              prevent_adding_db, the two poses.
//   landmarks  landmark_num = n_kps clamped to [0, max_num].  Landmark i < landmark_num is sent when flag[i] > 0 || send_all_features, in index order
//              (loop_net.cpp:66-68); feature_num counts the flagged ones, under send_all_features too (loop_net.cpp:62).
//   images     an image with landmark_num == 0 is not sent at all: no packets (broadcast_fisheye_desc, loop_net.cpp:22).  landmark_num > 0 with no landmark sent:
//              the header alone.
//   buffer     per image WP capacity(max_num) = 3 + 16545 + 324 * max_num bytes, a multiple of 4.  The header packet starts at byte WP_HEADER_OFFSET = 3, so its float
//              area starts at byte 164; the landmark packets follow at 16548 + 324 * k: every float area and every landmark packet starts on a 4-byte boundary and the
//              stage stores whole dwords only (the first dword's three leading bytes are zero padding).  Bytes behind the last packet are not written.
//   table      per image table_ints(max_num) = 2 + 2 * (1 + max_num) ints: [0] packets, [1] bytes used (the end of the last packet; 0 without packets), then
//              (offset, size) per packet, packet 0 the header (channel VIOKF_HEADER), the others landmarks (VIOKF_LANDMARKS); the unused entries are zero.
//
// The third packet of an image, the whole descriptor (wire::encode(ImageDescriptor, with_features), channel SWARM_LOOP_IMG_DES), has a buffer and a size table of its
// own, stated further down (whole_*): wire_pack_image_kernel / pack_whole_image_host, pinned by tests/cpp/wire_image_plan_pin.cpp in the same way.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define WP_HD __host__ __device__ inline
#else
#define WP_HD inline
#endif

#define WP_DESC_DIM 64
#define WP_GLOBAL_DIM 4096
#define WP_HEADER_HEAD_BYTES 161
#define WP_HEADER_BYTES OMNI_WIRE_HEADER_BYTES                // 161 + 4 * 4096
#define WP_LANDMARK_BYTES OMNI_WIRE_LANDMARK_BYTES            // 36 + 28 + 4 + 4 * 64
#define WP_LANDMARK_DWORDS (WP_LANDMARK_BYTES / 4)
#define WP_HEADER_OFFSET OMNI_WIRE_HEADER_OFFSET              // (3 + 161) % 4 == 0
#define WP_HEAD_PADDED (WP_HEADER_OFFSET + WP_HEADER_HEAD_BYTES)        // 164 bytes = 41 dwords: what the kernel builds in LDS
#define WP_HEAD_DWORDS (WP_HEAD_PADDED / 4)
#define WP_LANDMARKS_AT (WP_HEADER_OFFSET + WP_HEADER_BYTES)  // 16548
#define WP_TABLE_HEAD 2
#define WP_MAX_NUM 1024

static_assert(WP_HEADER_BYTES == 161 + 4 * WP_GLOBAL_DIM && WP_LANDMARK_BYTES == 36 + 28 + 4 + 4 * WP_DESC_DIM, "packet sizes");
static_assert(WP_HEAD_PADDED % 4 == 0 && WP_LANDMARKS_AT % 4 == 0 && WP_LANDMARK_BYTES % 4 == 0, "dword placement");
static_assert(sizeof(omni_wire_image_meta) == 144, "omni_wire_image_meta layout");

namespace omni {
namespace wp {

constexpr uint64_t kFpHeader = 0x4f4d4e4948445231ull;         // "OMNIHDR1" (wire::FP_HEADER)
constexpr uint64_t kFpLandmark = 0x4f4d4e494c4d4b31ull;       // "OMNILMK1" (wire::FP_LANDMARK)

WP_HD int64_t capacity(int max_num) { return (int64_t)WP_LANDMARKS_AT + (int64_t)WP_LANDMARK_BYTES * max_num; }
WP_HD int table_ints(int max_num) { return WP_TABLE_HEAD + 2 * (1 + max_num); }
WP_HD int clamp_count(int n, int max_num) { return n < 0 ? 0 : n > max_num ? max_num : n; }
WP_HD bool image_sent(int landmark_num) { return landmark_num > 0; }
WP_HD bool landmark_sent(int i, int landmark_num, uint8_t flag, int send_all_features) { return i < landmark_num && (flag > 0 || send_all_features != 0); }
WP_HD bool landmark_counted(int i, int landmark_num, uint8_t flag) { return i < landmark_num && flag > 0; }
WP_HD int landmark_offset(int k) { return WP_LANDMARKS_AT + WP_LANDMARK_BYTES * k; }

WP_HD uint32_t f32_bits(const float* p) { uint32_t u; __builtin_memcpy(&u, p, 4); return u; }
WP_HD uint64_t f64_bits(double v) { uint64_t u; __builtin_memcpy(&u, &v, 8); return u; }
WP_HD uint8_t be_byte64(uint64_t v, int j) { return (uint8_t)(v >> (56 - 8 * j)); }         // byte j of the big-endian form
WP_HD uint8_t be_byte32(uint32_t v, int j) { return (uint8_t)(v >> (24 - 8 * j)); }

// byte b of the first WP_HEAD_PADDED bytes of an image's buffer: three bytes of padding, then the header packet up to its float area
WP_HD uint8_t head_byte(int b, const omni_wire_image_meta& m, int feature_num) {
    const int o = b - WP_HEADER_OFFSET;
    if (o < 0) return 0;
    if (o < 8) return be_byte64(kFpHeader, o);
    if (o < 16) return be_byte64(f64_bits(m.timestamp), o - 8);
    if (o < 20) return be_byte32((uint32_t)m.drone_id, o - 16);
    if (o < 28) return 0;                                                                    // msg_id: the host's
    if (o < 36) return be_byte64((uint64_t)m.frame_id, o - 28);
    if (o < 40) return be_byte32((uint32_t)feature_num, o - 36);
    if (o < 44) return be_byte32((uint32_t)m.direction, o - 40);
    if (o < 45) return m.prevent_adding_db ? 1 : 0;
    if (o < 101) return be_byte64(f64_bits(m.pose_drone[(o - 45) >> 3]), (o - 45) & 7);
    if (o < 157) return be_byte64(f64_bits(m.camera_extrinsic[(o - 101) >> 3]), (o - 101) & 7);
    return be_byte32((uint32_t)WP_GLOBAL_DIM, o - 157);
}

// dword d (0..80) of landmark i's packet, as the little-endian machine stores it; the five arrays are the image's own rows
WP_HD uint32_t landmark_dword(int d, int i, int drone_id, const float* kps_xy, const float* desc, const float* norm2d, const float* l3d, const uint8_t* flag) {
    if (d >= 17) return __builtin_bswap32(f32_bits(desc + (size_t)i * WP_DESC_DIM + (d - 17)));
    switch (d) {
        case 0: return __builtin_bswap32((uint32_t)(kFpLandmark >> 32));
        case 1: return __builtin_bswap32((uint32_t)kFpLandmark);
        case 6: return __builtin_bswap32((uint32_t)drone_id);
        case 7: return __builtin_bswap32((uint32_t)i);
        case 8: return __builtin_bswap32((uint32_t)flag[i]);
        case 9: case 10: return __builtin_bswap32(f32_bits(norm2d + 2 * (size_t)i + (d - 9)));
        case 11: case 12: return __builtin_bswap32(f32_bits(kps_xy + 2 * (size_t)i + (d - 11)));
        case 13: case 14: case 15: return __builtin_bswap32(f32_bits(l3d + 3 * (size_t)i + (d - 13)));
        case 16: return __builtin_bswap32((uint32_t)WP_DESC_DIM);
        default: return 0;                                                                   // 2..5: msg_id and header_id, the host's
    }
}

// entry e of an image's table once the number of sent landmarks is known (n_sent < 0: the image is not sent)
WP_HD int table_entry(int e, int n_sent) {
    if (n_sent < 0) return 0;
    if (e == 0) return 1 + n_sent;
    if (e == 1) return WP_LANDMARKS_AT + WP_LANDMARK_BYTES * n_sent;
    const int k = (e - WP_TABLE_HEAD) >> 1, second = (e - WP_TABLE_HEAD) & 1;
    if (k > n_sent) return 0;
    if (k == 0) return second ? WP_HEADER_BYTES : WP_HEADER_OFFSET;
    return second ? WP_LANDMARK_BYTES : landmark_offset(k - 1);
}

// ---- the whole descriptor (wire::encode(ImageDescriptor, with_features); channel SWARM_LOOP_IMG_DES) ------------------------------------------------------------
//   head      WP_IMAGE_HEAD_BYTES = 177: every scalar and EVERY length member
//       0  i64 fingerprint "OMNIIMG1"      8  f64 timestamp      16  i32 drone_id      20  i64 msg_id (ZERO here)      28  i64 frame_id
//      36  i32 landmark_num               40  i32 direction      44  u8  prevent_adding_db
//      45  7 x f64 pose_drone            101  7 x f64 camera_extrinsic                157  i32 image_width            161  i32 image_height
//     165  i32 image_desc_size = 4096    169  i32 feature_descriptor_size = 64 * landmark_num, or 0 without with_features     173  i32 image_size
//   floats    image_desc, feature_descriptor, landmarks_2d_norm (2 per landmark), landmarks_2d (2), landmarks_3d (3): big-endian dwords, ALL landmark_num
//             landmarks (not only the flagged ones: the reference sends the message as it is, loop_net.cpp:105-114)
//   bytes     landmarks_flag (landmark_num bytes), then image (image_size bytes: the JPEG file of the unit's encode stage)
//   image     image_size = the file's size clamped to [0, jpeg_capacity] when with_image is set and the file's status is OMNI_JPEG_OK; 0 otherwise
//   buffer    per image whole_capacity(max_num, jpeg_capacity) bytes, a multiple of 4.  The packet starts at byte WP_IMAGE_OFFSET = 3, so the float area starts at byte
//             180 and the byte tail on a 4-byte boundary behind it.  Written: the three bytes of padding (zero), the packet, zeros up to the next 4-byte boundary
//             behind it; nothing behind that.  The JPEG file's rows are read as dwords: jpeg_capacity is a multiple of 4 and the host's rows are read bytewise.
//   sizes     per image 2 ints: (offset, size) of the packet, (0, 0) for an image that is not sent (landmark_num == 0, as broadcast_fisheye_desc)
//   id        msg_id is the image's, i.e. its header packet's: patch_whole_image_id
#define WP_IMAGE_HEAD_BYTES 177
#define WP_IMAGE_OFFSET 3
#define WP_IMAGE_HEAD_PADDED (WP_IMAGE_OFFSET + WP_IMAGE_HEAD_BYTES)     // 180 bytes = 45 dwords
#define WP_IMAGE_HEAD_DWORDS (WP_IMAGE_HEAD_PADDED / 4)
#define WP_LANDMARK_FLOATS 7                                             // 2 + 2 + 3 per landmark besides its descriptor
#define WP_MAX_JPEG_CAPACITY (1 << 30)
static_assert(WP_IMAGE_HEAD_PADDED % 4 == 0, "dword placement of the whole descriptor");

constexpr uint64_t kFpImage = 0x4f4d4e49494d4731ull;          // "OMNIIMG1" (wire::FP_IMAGE)

WP_HD int whole_feature_floats(int landmark_num, int with_features) { return with_features ? WP_DESC_DIM * landmark_num : 0; }
WP_HD int whole_float_dwords(int landmark_num, int with_features) { return WP_GLOBAL_DIM + whole_feature_floats(landmark_num, with_features) + WP_LANDMARK_FLOATS * landmark_num; }
WP_HD int64_t whole_capacity(int max_num, int64_t jpeg_capacity) {
    return (int64_t)WP_IMAGE_HEAD_PADDED + 4 * (int64_t)whole_float_dwords(max_num, 1) + (((int64_t)max_num + jpeg_capacity + 3) & ~(int64_t)3);
}
WP_HD int whole_image_size(int with_image, int status, int size, int64_t jpeg_capacity) {
    if (!with_image || status != OMNI_JPEG_OK || size < 0) return 0;
    return (int64_t)size > jpeg_capacity ? (int)jpeg_capacity : size;
}
WP_HD int whole_packet_bytes(int landmark_num, int with_features, int image_size) {
    return WP_IMAGE_HEAD_BYTES + 4 * whole_float_dwords(landmark_num, with_features) + landmark_num + image_size;
}

// byte b of the first WP_IMAGE_HEAD_PADDED bytes of an image's whole-descriptor buffer
WP_HD uint8_t whole_head_byte(int b, const omni_wire_image_meta& m, int landmark_num, int width, int height, int feature_floats, int image_size) {
    const int o = b - WP_IMAGE_OFFSET;
    if (o < 0) return 0;
    if (o < 8) return be_byte64(kFpImage, o);
    if (o < 16) return be_byte64(f64_bits(m.timestamp), o - 8);
    if (o < 20) return be_byte32((uint32_t)m.drone_id, o - 16);
    if (o < 28) return 0;                                                                    // msg_id: the host's
    if (o < 36) return be_byte64((uint64_t)m.frame_id, o - 28);
    if (o < 40) return be_byte32((uint32_t)landmark_num, o - 36);
    if (o < 44) return be_byte32((uint32_t)m.direction, o - 40);
    if (o < 45) return m.prevent_adding_db ? 1 : 0;
    if (o < 101) return be_byte64(f64_bits(m.pose_drone[(o - 45) >> 3]), (o - 45) & 7);
    if (o < 157) return be_byte64(f64_bits(m.camera_extrinsic[(o - 101) >> 3]), (o - 101) & 7);
    if (o < 161) return be_byte32((uint32_t)width, o - 157);
    if (o < 165) return be_byte32((uint32_t)height, o - 161);
    if (o < 169) return be_byte32((uint32_t)WP_GLOBAL_DIM, o - 165);
    if (o < 173) return be_byte32((uint32_t)feature_floats, o - 169);
    return be_byte32((uint32_t)image_size, o - 173);
}

// dword j of the float area, as the little-endian machine stores it; every array is the image's own rows, of which the first landmark_num are contiguous
WP_HD uint32_t whole_float_dword(int j, int landmark_num, int feature_floats, const float* global, const float* desc, const float* norm2d, const float* kps_xy,
                                 const float* l3d) {
    const float* p;
    if (j < WP_GLOBAL_DIM) p = global + j;
    else if ((j -= WP_GLOBAL_DIM) < feature_floats) p = desc + j;
    else if ((j -= feature_floats) < 2 * landmark_num) p = norm2d + j;
    else if ((j -= 2 * landmark_num) < 2 * landmark_num) p = kps_xy + j;
    else p = l3d + (j - 2 * landmark_num);
    return __builtin_bswap32(f32_bits(p));
}

// dword q of a JPEG file's row; only a dword with a byte of the file in it is ever asked for (4 * q < image_size <= jpeg_capacity, a multiple of 4)
WP_HD uint32_t jpeg_dword(const uint8_t* row, int q) {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const uint32_t*>(row)[q];                                        // (the row starts on a 4-byte boundary: refused otherwise)
#else
    uint32_t v; __builtin_memcpy(&v, row + 4 * (size_t)q, 4); return v;
#endif
}

// dword d of the byte tail (landmark_num flag bytes, then image_size bytes of the file, then zeros up to the 4-byte boundary), as the machine stores it.  The file's
// destination starts at byte landmark_num of the tail, its source on a dword of its own: an output dword is put together from two neighbouring source dwords.
WP_HD uint32_t whole_tail_dword(int d, int landmark_num, int image_size, const uint8_t* flag, const uint8_t* jpeg_row) {
    const int base = 4 * d, s = base - landmark_num;         // s: the file's byte that output byte 0 holds (negative: flag bytes come first)
    uint32_t v = 0;
    if (s < 0) {
        const int k = -s < 4 ? -s : 4;                        // flag bytes in this dword
        for (int j = 0; j < k; ++j) v |= (uint32_t)flag[base + j] << (8 * j);
        if (k < 4 && image_size > 0) v |= jpeg_dword(jpeg_row, 0) << (8 * k);
    } else if (s < image_size) {
        const int q = s >> 2, sh = 8 * (s & 3);
        const uint32_t lo = jpeg_dword(jpeg_row, q), hi = sh != 0 && 4 * (q + 1) < image_size ? jpeg_dword(jpeg_row, q + 1) : 0u;
        v = sh != 0 ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    const int valid = landmark_num + image_size - base;       // bytes of this dword that belong to the packet
    return valid >= 4 ? v : valid <= 0 ? 0u : v & ((1u << (8 * valid)) - 1u);
}

#if !defined(__HIP_DEVICE_COMPILE__)
inline void put_dword(uint8_t* at, uint32_t v) { __builtin_memcpy(at, &v, 4); }

// one image's whole descriptor on one thread, the dwords the kernel's lanes store.  out: whole_capacity(max_num, jpeg_capacity) bytes, sizes: 2 ints.  jpeg_row,
// jpeg_size and jpeg_status are read only with with_image set.
inline void pack_whole_image_host(int max_num, int with_features, int with_image, const float* kps_xy, int n_kps, const float* desc, const float* norm2d, const float* l3d,
                                  const uint8_t* flag, const float* global, const omni_wire_image_meta& m, const uint8_t* jpeg_row, int jpeg_size, int jpeg_status,
                                  int64_t jpeg_capacity, int width, int height, uint8_t* out, int* sizes) {
    const int n = clamp_count(n_kps, max_num);
    if (!image_sent(n)) { sizes[0] = sizes[1] = 0; return; }
    const int isz = whole_image_size(with_image, jpeg_status, jpeg_size, jpeg_capacity), ff = whole_feature_floats(n, with_features), fd = whole_float_dwords(n, with_features);
    for (int b = 0; b < WP_IMAGE_HEAD_PADDED; ++b) out[b] = whole_head_byte(b, m, n, width, height, ff, isz);
    for (int j = 0; j < fd; ++j) put_dword(out + WP_IMAGE_HEAD_PADDED + 4 * (size_t)j, whole_float_dword(j, n, ff, global, desc, norm2d, kps_xy, l3d));
    uint8_t* tail = out + WP_IMAGE_HEAD_PADDED + 4 * (size_t)fd;
    for (int d = 0; 4 * d < n + isz; ++d) put_dword(tail + 4 * (size_t)d, whole_tail_dword(d, n, isz, flag, jpeg_row));
    sizes[0] = WP_IMAGE_OFFSET; sizes[1] = whole_packet_bytes(n, with_features, isz);
}

// one image on one thread: the order the kernel's lanes produce, sequentially.  out: capacity(max_num) bytes, table: table_ints(max_num) ints
inline void pack_image_host(int max_num, int send_all_features, const float* kps_xy, int n_kps, const float* desc, const float* norm2d, const float* l3d,
                            const uint8_t* flag, const float* global, const omni_wire_image_meta& m, uint8_t* out, int* table) {
    const int n = clamp_count(n_kps, max_num), te = table_ints(max_num);
    if (!image_sent(n)) { for (int e = 0; e < te; ++e) table[e] = table_entry(e, -1); return; }
    int feature_num = 0, n_sent = 0;
    for (int i = 0; i < n; ++i) {
        if (landmark_counted(i, n, flag[i])) ++feature_num;
        if (!landmark_sent(i, n, flag[i], send_all_features)) continue;
        uint8_t* at = out + landmark_offset(n_sent++);
        for (int d = 0; d < WP_LANDMARK_DWORDS; ++d) put_dword(at + 4 * d, landmark_dword(d, i, m.drone_id, kps_xy, desc, norm2d, l3d, flag));
    }
    for (int b = 0; b < WP_HEAD_PADDED; ++b) out[b] = head_byte(b, m, feature_num);
    for (int j = 0; j < WP_GLOBAL_DIM; ++j) put_dword(out + WP_HEAD_PADDED + 4 * j, __builtin_bswap32(f32_bits(global + j)));
    for (int e = 0; e < te; ++e) table[e] = table_entry(e, n_sent);
}

// the host's part: the ids of LoopNetWire's sequence into a packed packet (big-endian, at the offsets above)
inline void put_be64(uint8_t* at, int64_t v) { for (int j = 0; j < 8; ++j) at[j] = be_byte64((uint64_t)v, j); }
inline void patch_header_id(uint8_t* header_packet, int64_t msg_id) { put_be64(header_packet + 20, msg_id); }
inline void patch_landmark_ids(uint8_t* landmark_packet, int64_t msg_id, int64_t header_id) { put_be64(landmark_packet + 8, msg_id); put_be64(landmark_packet + 16, header_id); }
inline void patch_whole_image_id(uint8_t* whole_packet, int64_t msg_id) { put_be64(whole_packet + 20, msg_id); }      // the image's id: its header packet's
#endif

}  // namespace wp
}  // namespace omni
