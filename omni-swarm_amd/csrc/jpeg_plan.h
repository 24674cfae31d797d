// jpeg_plan.h -- baseline sequential JPEG of ONE 8-bit component, stated once: what cv::imencode(".jpg", gray, {IMWRITE_JPEG_QUALITY, q}) asks of libjpeg for the
// main image of every direction when send_img is set (swarm_loop/src/loop_cam.cpp:56-71 encode_image, :306-308, :463-469).  Plain C++ for g++ AND hipcc:
// jpeg.hip runs these functions one 8 x 8 block per lane, jpeg_host.cpp compiles jpeg_encode_host into the library for host callers, tests/cpp/jpeg_plan_pin.cpp
// runs it on the host; nothing else restates the arithmetic.  Integers only: there is nothing to round differently on the two sides.
//
// PINNED: libjpeg's defaults (jpeg_set_defaults, jpeg_set_quality(q, TRUE), JDCT_ISLOW, the standard Huffman tables, JFIF APP0) as Pillow (libjpeg-turbo)
// writes them -- tests/test_jpeg_plan_cpu.py compares whole files byte for byte.  UNPINNED: whatever cv::imencode adds beyond those defaults (OpenCV is not
// vendored).
//
//   table      IJG luminance table (Annex K.1) scaled: q clamped to 1..100, s = q < 50 ? 5000 / q : 200 - 2 q, t = clamp((base * s + 50) / 100, 1, 255)
//   DCT        jfdctint.c's "islow" on samples - 128: CONST_BITS 13, PASS1_BITS 2, rows scaled up by << 2, columns descaled with rounding; the output is
//              8 x the DCT, and its DC term is EXACTLY the sum of the 64 centred samples (rows: 4 * sum; columns: (4 S + 2) >> 2 = S)
//   quantise   qv = t << 3; v < 0: -(((-v) + (qv >> 1)) / qv), else (v + (qv >> 1)) / qv -- truncating division
//   entropy    zig-zag; DC difference against the previous block in raster order (predictor 0 at the first); Annex K.3 / K.5 tables; ZRL for runs above
//              15, EOB when the tail is zero; a negative value is coded as v - 1 in its low nbits bits
//   bit stream MSB first, 0x00 behind every 0xFF, the last partial byte padded with 1-bits (and stuffed when that makes it 0xFF)
//   edges      blocks beyond the right / bottom edge replicate the last column / row
//   rows       rows at or beyond zero_from_row are READ AS 0 (h: none).  That is how the fisheye mask reaches the picture: the reference's blanking
//              (loop_cam.cpp:536-539) writes into the cv::Mat whose pixels msg.left_images[vcam_id] shares (extractor_img_desc_deepnet takes the Mat by value;
//              a cv::Mat copy shares the data), so the image encoded at :467 already has its bottom quarter black.  Read from the code; it cannot be run here.
//   file       SOI | APP0 JFIF 1.01, units 0, density 1 x 1, no thumbnail | DQT table 0, 8-bit, zig-zag | SOF0 8 bits, H, W, 1 component 1 x 1 table 0 |
//              DHT DC 0 | DHT AC 0 | SOS | scan | EOI.  The header is JP_HEADER_BYTES = 328 bytes for these choices.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define JP_HD __host__ __device__ inline
#else
#define JP_HD inline
#endif
#if defined(__clang__)
#define JP_UNROLL _Pragma("unroll")
#else
#define JP_UNROLL
#endif

#define JP_HEADER_BYTES 328
#define JP_MAX_BLOCK_BITS (63 * 26 + 20)                    // 63 AC terms of 16 code + 10 value bits, a DC term of 9 + 11

namespace omni {
namespace jp {

// ---- tables (host side: they reach the kernels as handle-owned arrays) ----------------------------------------------------------------------------
static const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                                      14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kDcBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kAcVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline int clamp_quality(int q) { return q < 1 ? 1 : q > 100 ? 100 : q; }
// t[64] in natural (row-major) order
inline void quant_table(int quality, uint8_t* t) {
    const int q = clamp_quality(quality), s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 64; ++i) {
        int v = ((int)kBaseLuma[i] * s + 50) / 100;
        t[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}
// The tables a coder needs: a Huffman table as tab[symbol] = code << 8 | length (length 0: no such symbol), Annex C's code assignment
struct Tables {
    uint16_t qv[64];                                        // t << 3, natural order
    uint32_t dc[16], ac[256];
};
inline void build_huff(const uint8_t* bits, const uint8_t* vals, uint32_t* tab, int n_tab) {
    for (int i = 0; i < n_tab; ++i) tab[i] = 0;
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) tab[vals[k++]] = code++ << 8 | (uint32_t)len;
        code <<= 1;
    }
}
inline void build_tables(int quality, Tables* T) {
    uint8_t t[64];
    quant_table(quality, t);
    for (int i = 0; i < 64; ++i) T->qv[i] = (uint16_t)(t[i] << 3);
    build_huff(kDcBits, kDcVals, T->dc, 16);
    build_huff(kAcBits, kAcVals, T->ac, 256);
}

// ---- the per-block pieces (host and device) --------------------------------------------------------------------------------------------------------
// pixel (x, y) of the picture as the coder reads it: the last column / row replicated, rows at or beyond zero_from_row black
JP_HD int sample(const uint8_t* gray, int stride, int w, int h, int zero_from_row, int x, int y) {
    const int r = y < h ? y : h - 1, c = x < w ? x : w - 1;
    return r >= zero_from_row ? 0 : (int)gray[(size_t)r * stride + c];
}
// block (bx, by)'s 64 samples minus 128, row-major
JP_HD void load_block(const uint8_t* gray, int stride, int w, int h, int zero_from_row, int bx, int by, int* s) {
    JP_UNROLL
    for (int j = 0; j < 8; ++j) {
        const int y = by * 8 + j, r = y < h ? y : h - 1;
        const uint8_t* row = gray + (size_t)r * stride;
        const bool zero = r >= zero_from_row;
        if (!zero && bx * 8 + 8 <= w && (((uintptr_t)row + (size_t)bx * 8) & 7) == 0) {     // an interior, aligned row: one 8-byte load
            const uint64_t v = *reinterpret_cast<const uint64_t*>(row + bx * 8);
            JP_UNROLL
            for (int i = 0; i < 8; ++i) s[j * 8 + i] = (int)((v >> (8 * i)) & 0xff) - 128;
        } else {
            JP_UNROLL
            for (int i = 0; i < 8; ++i) {
                const int x = bx * 8 + i, c = x < w ? x : w - 1;
                s[j * 8 + i] = (zero ? 0 : (int)row[c]) - 128;
            }
        }
    }
}
JP_HD int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// one pass of jfdctint.c over 8 values in place (stride st): first = the row pass
template <bool kFirst>
JP_HD void fdct_1d(int* d, int st) {
    const int kC = 13, kP = 2;
    const int t0 = d[0] + d[7 * st], t7 = d[0] - d[7 * st], t1 = d[st] + d[6 * st], t6 = d[st] - d[6 * st];
    const int t2 = d[2 * st] + d[5 * st], t5 = d[2 * st] - d[5 * st], t3 = d[3 * st] + d[4 * st], t4 = d[3 * st] - d[4 * st];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int sh = kFirst ? kC - kP : kC + kP;
    if (kFirst) {
        d[0] = (t10 + t11) * (1 << kP);                     // (jfdctint's `<< PASS1_BITS`, written so that a negative sum is defined before C++20 too)
        d[4 * st] = (t10 - t11) * (1 << kP);
    } else {
        d[0] = descale(t10 + t11, kP);
        d[4 * st] = descale(t10 - t11, kP);
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * st] = descale(z1 + t13 * 6270, sh);
    d[6 * st] = descale(z1 + t12 * (-15137), sh);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7 * st] = descale(u4 + z1 + z3, sh);
    d[5 * st] = descale(u5 + z2 + z4, sh);
    d[3 * st] = descale(u6 + z2 + z3, sh);
    d[st] = descale(u7 + z1 + z4, sh);
}
JP_HD int quantise(int v, int qv) { return v < 0 ? -(((-v) + (qv >> 1)) / qv) : (v + (qv >> 1)) / qv; }
// s: 64 centred samples in, 64 quantised coefficients out (natural order)
JP_HD void fdct_quant(int* s, const uint16_t* qv) {
    JP_UNROLL
    for (int r = 0; r < 8; ++r) fdct_1d<true>(s + 8 * r, 1);
    JP_UNROLL
    for (int c = 0; c < 8; ++c) fdct_1d<false>(s + c, 8);
    JP_UNROLL
    for (int i = 0; i < 64; ++i) s[i] = quantise(s[i], (int)qv[i]);
}
// the quantised DC of block (bx, by) from its pixel sum alone -- the predictor of the block behind it, without that block's DCT
JP_HD int block_dc(const uint8_t* gray, int stride, int w, int h, int zero_from_row, int bx, int by, int qv0) {
    int s[64], sum = 0;
    load_block(gray, stride, w, h, zero_from_row, bx, by, s);
    JP_UNROLL
    for (int i = 0; i < 64; ++i) sum += s[i];
    return quantise(sum, qv0);
}
JP_HD int nbits_of(int a) { return a == 0 ? 0 : 32 - __builtin_clz((unsigned)a); }   // a >= 0
// one coefficient's magnitude category and its value bits (a negative value as v - 1 in the low nbits bits)
JP_HD void value_bits(int v, int* nbits, uint32_t* bits) {
    const int a = v < 0 ? -v : v, n = nbits_of(a);
    *nbits = n;
    *bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
}
// The code of one block: c = its quantised coefficients (natural order), pred = the previous block's quantised DC.  sink.put(bits, n) takes n <= 27 bits,
// MSB first.  The walk is unrolled: kZigzag[k] is then a constant and c[] stays in registers.
template <class Sink>
JP_HD void block_code(const int* c, int pred, const uint32_t* dc_tab, const uint32_t* ac_tab, Sink& sink) {
    int n;
    uint32_t vb;
    value_bits(c[0] - pred, &n, &vb);
    uint32_t e = dc_tab[n];
    sink.put((e >> 8) << n | vb, (int)(e & 0xff) + n);
    int run = 0;
    JP_UNROLL
    for (int k = 1; k < 64; ++k) {
        const int v = c[kZigzag[k]];
        if (v == 0) {
            ++run;
        } else {
            while (run > 15) {
                e = ac_tab[0xf0];
                sink.put(e >> 8, (int)(e & 0xff));
                run -= 16;
            }
            value_bits(v, &n, &vb);
            e = ac_tab[run << 4 | n];
            sink.put((e >> 8) << n | vb, (int)(e & 0xff) + n);
            run = 0;
        }
    }
    if (run > 0) {
        e = ac_tab[0];
        sink.put(e >> 8, (int)(e & 0xff));
    }
}
struct BitCount {                                           // a sink that only measures
    uint32_t bits = 0;
    JP_HD void put(uint32_t, int n) { bits += (uint32_t)n; }
};
// block b (raster order) of a picture bw blocks wide: its code into `sink`
template <class Sink>
JP_HD void encode_block(const uint8_t* gray, int stride, int w, int h, int zero_from_row, int bw, int b, const uint16_t* qv, const uint32_t* dc_tab,
                        const uint32_t* ac_tab, Sink& sink) {
    int s[64];
    const int pred = b == 0 ? 0 : block_dc(gray, stride, w, h, zero_from_row, (b - 1) % bw, (b - 1) / bw, (int)qv[0]);
    load_block(gray, stride, w, h, zero_from_row, b % bw, b / bw, s);
    fdct_quant(s, qv);
    block_code(s, pred, dc_tab, ac_tab, sink);
}

// ---- the file ------------------------------------------------------------------------------------------------------------------------------------
// out[JP_HEADER_BYTES]: everything in front of the scan
inline int jpeg_header(int w, int h, int quality, uint8_t* out) {
    uint8_t t[64];
    quant_table(quality, t);
    uint8_t* p = out;
    auto u8 = [&](int v) { *p++ = (uint8_t)v; };
    auto u16 = [&](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
    u16(0xffd8);
    u16(0xffe0); u16(16); u8('J'); u8('F'); u8('I'); u8('F'); u8(0); u16(0x0101); u8(0); u16(1); u16(1); u8(0); u8(0);
    u16(0xffdb); u16(67); u8(0);
    for (int k = 0; k < 64; ++k) u8(t[kZigzag[k]]);
    u16(0xffc0); u16(11); u8(8); u16(h); u16(w); u8(1); u8(1); u8(0x11); u8(0);
    u16(0xffc4); u16(2 + 1 + 16 + 12); u8(0x00);
    for (int i = 0; i < 16; ++i) u8(kDcBits[i]);
    for (int i = 0; i < 12; ++i) u8(kDcVals[i]);
    u16(0xffc4); u16(2 + 1 + 16 + 162); u8(0x10);
    for (int i = 0; i < 16; ++i) u8(kAcBits[i]);
    for (int i = 0; i < 162; ++i) u8(kAcVals[i]);
    u16(0xffda); u16(8); u8(1); u8(1); u8(0x00); u8(0); u8(63); u8(0);
    return (int)(p - out);
}

// the host's sink: bytes with stuffing, never past `cap`; `pos` keeps counting so that the caller learns the size it would have needed
struct ByteSink {
    uint8_t* out;
    int64_t cap, pos = 0;
    uint64_t acc = 0;
    int nacc = 0;
    void byte(int v) {
        if (pos < cap) out[pos] = (uint8_t)v;
        ++pos;
    }
    void put(uint32_t bits, int n) {
        acc = acc << n | bits;
        nacc += n;
        while (nacc >= 8) {
            const int v = (int)(acc >> (nacc - 8)) & 0xff;
            byte(v);
            if (v == 0xff) byte(0);
            nacc -= 8;
        }
    }
    void flush() {
        if (nacc > 0) put((1u << (8 - nacc)) - 1u, 8 - nacc);
    }
};

// The whole file of one picture.  *size = its bytes and OMNI_JPEG_OK; or, when they exceed `capacity`, OMNI_JPEG_TRUNCATED with *size = 0: nothing is written
// past the capacity and what lies below it is unspecified.  Returns the status, or -1 for arguments no file can be made of.
inline int jpeg_encode_host(const uint8_t* gray, int stride, int w, int h, int quality, int zero_from_row, uint8_t* out, int64_t capacity, int64_t* size) {
    if (size) *size = 0;
    if (!gray || !out || !size || w < 1 || h < 1 || w > 65535 || h > 65535 || stride < w || capacity < JP_HEADER_BYTES + 2) return -1;
    Tables T;
    build_tables(quality, &T);
    static_assert(JP_HEADER_BYTES == 0x148, "SOI + APP0 + DQT + SOF0 + 2 DHT + SOS");
    if (jpeg_header(w, h, quality, out) != JP_HEADER_BYTES) return -1;
    ByteSink sink{out, capacity, JP_HEADER_BYTES};
    const int bw = (w + 7) / 8, bh = (h + 7) / 8;
    for (int b = 0; b < bw * bh; ++b) encode_block(gray, stride, w, h, zero_from_row, bw, b, T.qv, T.dc, T.ac, sink);
    sink.flush();
    sink.byte(0xff);
    sink.byte(0xd9);
    if (sink.pos > capacity) return OMNI_JPEG_TRUNCATED;
    *size = sink.pos;
    return OMNI_JPEG_OK;
}

}  // namespace jp
}  // namespace omni
