// jpeg_dec_plan.h -- the gray image of a baseline JPEG file, stated once: what cv::imdecode(data, cv::IMREAD_GRAYSCALE) asks of libjpeg for every frame of a
// CompressedImage topic when is_compressed_images is set (swarm_loop/src/swarm_loop.cpp:72-89, 291-292, 341-360; loop_utils.cpp:8).  Plain C++ for g++ AND
// hipcc: jpeg_dec.hip runs the phase functions lane-wise, jpeg_dec_host.cpp compiles the host decoders into the library, tests/cpp/jpegdec_plan_pin.cpp runs
// them on the host; nothing else restates the arithmetic.  Integers only.
//
// PINNED: libjpeg-turbo's output for out_color_space = JCS_GRAYSCALE, JDCT_ISLOW -- the FIRST component alone, dequantised, jidctint.c's islow IDCT, range
// limit -- as Pillow gives it (Image.open(..).convert-free 'L' files; Image.draft('L', size) for colour files): tests/test_jpegdec_plan_cpu.py compares every
// pixel.  UNPINNED: cv::imdecode itself (OpenCV is not vendored); that it asks libjpeg for JCS_GRAYSCALE is read from knowledge, not run.
//
//   parser     SOI, APPn / COM (skipped), DQT (8-bit tables), SOF0, DHT (any tables), DRI, SOS, EOI -> Desc: sizes, MCU layout, the first component's
//              quantisation table, the Huffman tables of the scan that holds the first component, that scan's byte range, and the classification
//                OK           the device decodes it
//                HOST         a valid baseline file the device does not take: restart interval != 0, more than one scan, a first component sampled other
//                             than {1,2} x {1,2} or other components other than 1 x 1 (the caller adds: a file above the handle's capacity)
//                UNSUPPORTED  progressive, arithmetic, lossless, extended / 12-bit, 16-bit quantisation tables, a component count other than 1 or 3, a first
//                             component sampled below another one
//                CORRUPT      anything else that cannot be a file
//   bytes      0xFF00 unstuffing and the end at a marker happen in a FIRST PASS on the host (unstuff): the scan the decoders and the kernels read is the
//              clean bit stream, MSB first, followed by >= JD_SCAN_PAD zero bytes.  Restart markers become a list of byte offsets (the host decoder and the chunk plan).
//              A handle whose OMNI_JPEGDEC_UNSTUFF_DEV is 1 splits that pass: survey() visits the 0xFF bytes alone (memchr) for the scan's end, the clean length,
//              the markers' offsets and the clean offset of every tile of JD_UNSTUFF_TILE raw bytes; the raw scan is uploaded as it is and every tile is compacted
//              on its own with unstuff_keep() -- the same clean bytes (unstuff_tiled_host is the stand-in for jpegdec_unstuff_kernel)
//   symbol     step(): ONE total function (bit position, z = next zig-zag index 0..63, b = block within the MCU) -> next state, at most one (block, natural
//              index, value) emission, an error flag.  z == 0: a DC category + value bits; else an AC (run, size): ZRL (z += 16; reaching 64 ends the block, as
//              libjpeg's loop does), EOB, value extension as in jpeg_plan.h.  Defined for EVERY bit pattern: an undefined code is 1 bit long and reads as symbol
//              0 (+ error); a run past 63 ends the block without emission (+ error); EOBn with n > 0 ends the block (+ error); bits past the end of the data
//              read as 0 (+ error).  Every step consumes at least one bit.  Only an error on the TRUE chain, before the picture's last block, means CORRUPT
//   subseq     decode_subseq(i, entry) over the symbols that START in bits [i S, (i + 1) S): -> exit state (the overhang into i + 1: 0..30 bits, z, b; 16 bits),
//              blocks completed, error
//   parallel   1  every subsequence from the guess (overhang 0, z 0, b 0)
//              2  relaxation rounds (Jacobi): subsequence i >= 1 again from the exit state of i - 1 whenever that differs from the entry it last used, until a
//                 round changes nothing.  After round r the first r + 1 subsequences are final: N rounds bound it, and the fixed point IS the sequential decode
//              3  exclusive scan of the block counts = every subsequence's first block
//              4  write pass: the first component's AC coefficients (int16, natural order, into a zeroed array, blocks in SCAN order) and DC differences
//                 (int32); other components are decoded and dropped.  Stops at the picture's last block; the error flag counts only up to there
//              5  inclusive scan of the DC differences in scan order (mod 2^32) = the DC values
//              6  per 8 x 8 block: dequantise, islow IDCT (CONST_BITS 13, PASS1_BITS 2; columns first with descale 11, rows with descale 18 -- the +128 level
//                 shift and the final >> 3 in one), clamp to 0..255, store cropped to width x height.  All in uint32 arithmetic (= two's complement int32,
//                 no overflow to be undefined for ANY coefficients); libjpeg's all-zero-AC column shortcut is arithmetically the same and is not restated
//   CORRUPT    the picture is all zeros
//   restart    a file with a restart interval (DRI) stays HOST at parse time; a handle whose OMNI_JPEGDEC_RESTART_WGS is W >= 1 promotes one whose ONLY obstacle is
//              the interval (Desc::restart_only).  Every interval starts byte-aligned behind its marker from the known state pack_state(0, 0, 0) with a DC
//              predictor of zero at block k * restart * bpm: intervals are independent streams.  plan_chunks() cuts every interval into subsequences of its own
//              ([bit_begin + j S, ...), bounded by the interval's end: decode_subseq_seg) and groups consecutive intervals into at most W chunks balanced by bits,
//              each of at most max_sub subsequences (S doubled until that holds) -- one workgroup per chunk, none reads what another wrote.  Phases 1-4 run per
//              chunk; the first subsequence of an interval has the fixed entry 0; a subsequence's first block is its interval's first block + the counts before
//              it INSIDE the interval; the write pass bounds every interval to its own blocks, and an interval that completes fewer inside its own bits is
//              CORRUPT (DIVERGENCE from decode_sequential, which reads on into the next interval; libjpeg's own resynchronisation is unpinned either way).
//              Fewer markers than ceil(mcus / restart) - 1: CORRUPT (decode_sequential: seg >= n_rst); surplus markers are ignored.  Phase 5 becomes a
//              segmented scan: the running DC sum restarts every restart * ny blocks of the first component.  A file that cannot be planned (more intervals in a
//              chunk than max_sub) stays HOST
//   plain      a file WITHOUT a restart interval is one stream: no point inside it has a known state.  A handle whose OMNI_JPEGDEC_PLAIN_WGS is W >= 2 still spreads
//              it, because the relaxation of phase 2 reaches its fixed point from ANY starting state: C = plain_chunks(n_sub, W) = min(W, n_sub) chunks of consecutive
//              subsequences, chunk c = [plain_chunk_begin(c, n_sub, C), plain_chunk_begin(c + 1, n_sub, C)) = [c n_sub / C, (c + 1) n_sub / C), with S =
//              plain_subseq_bits(): the configured length doubled only until every chunk holds at most max_sub subsequences.  Phases 1-2 run per chunk, the chunk's
//              first subsequence keeping the guess as its entry -- one workgroup per chunk, none reads what another wrote; then ONE relaxation over all the
//              picture's subsequences (the SEAM relaxation: only what the seams between chunks got wrong is decoded again) ends in the same fixed point, the
//              sequential decode; phase 3 is one scan over the picture, phase 4 one subsequence at a time from the stored entry and first block.  Phases 5-6 as
//              ever.  Same pixels, same status as the one-chunk path for EVERY input
//   stand-in   decode_planned_host: ONE CPU stand-in for all the kernels' paths, under a handle's two switches.  It sees a picture as they do -- an Interval table
//              and chunk bounds -- and has one relaxation, one scan, one write pass, one error rule.  jpeg_decode_host and Pillow's pixels share none of its code
#pragma once
#include <stdint.h>
#include <string.h>

#include "jpeg_plan.h"

#define JD_SCAN_PAD 16                                       // zero bytes behind a clean scan: the bit window reads up to 12 bytes past the last symbol
#define JD_UNSTUFF_TILE 4096                                 // raw scan bytes per tile of the unstuffing by tiles (csrc/jpeg_dec.hip: 16 per lane)
#define JD_UNSTUFF_OUTSIDE 0x01                              // stands for a neighbour outside the scan: neither 0x00 nor 0xFF
#define JD_MAX_BPM 10                                        // blocks per MCU (the standard's limit)
#define JD_MIN_SUBSEQ_BITS 128
#define JD_MAX_SUBSEQ_BITS 65536
#define JD_MAX_SUBSEQ 4096                                   // subsequences a workgroup of the entropy kernel holds (csrc/jpeg_dec.hip: 16 per lane)
#define JD_MAX_RESTART_WGS 64                                // workgroups a restart-interval picture is spread over, at most (OMNI_JPEGDEC_RESTART_WGS)
#define JD_MAX_PLAIN_WGS 64                                  // ... and a picture without a restart interval (OMNI_JPEGDEC_PLAIN_WGS)

namespace omni {
namespace jd {

// a Huffman table in the form the kernel reads: a first level over the next 8 bits, then Annex F's canonical walk for codes of 9..16 bits
struct HuffTab {
    uint16_t look[256];                                     // length << 8 | symbol of the code that starts these 8 bits; 0: longer than 8 bits, or none
    int32_t maxcode[17];                                    // [l]: the largest code of l bits, -1: none
    int32_t valoff[17];                                     // [l]: index of the first symbol of l bits - the smallest code of l bits
    uint8_t vals[256];
};
// what step() reads (the kernel keeps it in LDS)
struct Tables {
    int32_t bpm, ny;                                        // blocks per MCU; of which the first ny belong to the first component
    uint8_t blk_comp[JD_MAX_BPM + 2];                       // block of the MCU -> component of the scan (0: the first)
    uint8_t zz[64];                                         // zig-zag index -> natural index
    HuffTab dc[3], ac[3];                                   // per component of the scan
};
struct Desc {
    int32_t status;                                         // OMNI_JPEGDEC_*
    int32_t w, h, ncomp, hs, vs;                            // hs x vs: the first component's blocks per MCU
    int32_t mcus_x, mcus_y, restart, multi_scan;
    int32_t restart_only;                                   // HOST for its restart interval alone: without it the file would be OK
    uint32_t n_blocks, n_yblocks;                           // of the scan; of the first component (MCU padding included)
    uint32_t spread_chunks;                                 // filled by whoever packs the image, like the fields below: >= 2: a picture without a restart interval
                                                            // that takes the spread path (OMNI_JPEGDEC_PLAIN_WGS; mode JD_MODE_SPREAD) over that many chunks; 0: none
    int64_t scan_off, scan_bytes;                           // the scan's bytes in the file (stuffed, restart markers included)
    // filled by whoever packs the image for the kernels (jpeg_dec.hip)
    int32_t mode;                                           // JD_MODE_*
    uint32_t total_bits, subseq_bits, n_sub;
    int64_t dev_off;                                        // MODE_DECODE: the clean scan, MODE_PIXELS: w x h pixels -- byte offset inside the uploaded block
    uint32_t n_int, n_chunks;                               // a planned restart file: intervals and chunks (0 0: no restart interval, one chunk over the whole scan)
    int64_t tab_off;                                        // ... its tables: Interval[n_int + 1] (the last one a sentinel), then uint32 first interval of chunk [n_chunks + 1]
    uint16_t q[64];                                         // the first component's quantisation table, natural order
    Tables T;
};
enum { JD_MODE_DECODE = 0, JD_MODE_PIXELS = 1, JD_MODE_ZERO = 2, JD_MODE_SPREAD = 3 };      // SPREAD: decoded like DECODE, by the chunk, seam and write kernels

// ---- parser (host) -----------------------------------------------------------------------------------------------------------------------------------
inline int build_hufftab(const uint8_t* bits, const uint8_t* vals, bool dc, HuffTab* t) {
    memset(t, 0, sizeof(*t));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        t->maxcode[l] = -1;
        if (n) {
            if (code + n > (1 << l) || k + n > 256) return 1;
            t->valoff[l] = k - code;
            t->maxcode[l] = code + n - 1;
            if (l <= 8)
                for (int j = 0; j < n; ++j)
                    for (int f = 0; f < (1 << (8 - l)); ++f) t->look[((code + j) << (8 - l)) + f] = (uint16_t)(l << 8 | vals[k + j]);
        }
        k += n;
        code = (code + n) << 1;
    }
    for (int i = 0; i < k; ++i) {
        if (dc && vals[i] > 15) return 1;
        t->vals[i] = vals[i];
    }
    return 0;
}

// the end of the entropy-coded data that starts at p: the first marker that is neither a stuffed 0xFF00 nor a restart marker (or the end of the file)
// (memchr finds the 0xFF bytes; only they and the byte behind each run are looked at one by one)
inline int64_t scan_end(const uint8_t* f, int64_t size, int64_t p) {
    while (p < size) {
        const uint8_t* ff = static_cast<const uint8_t*>(memchr(f + p, 0xff, (size_t)(size - p)));
        if (!ff) return size;
        p = ff - f;
        int64_t q = p + 1;
        while (q < size && f[q] == 0xff) ++q;
        if (q >= size) return size;
        if (f[q] == 0 || (f[q] >= 0xd0 && f[q] <= 0xd7)) { p = q + 1; continue; }
        return p;
    }
    return size;
}

// The descriptor of a file.  Returns d->status; d->w / d->h are the frame's size as soon as a frame header was read (0 before).
inline int parse(const uint8_t* f, int64_t size, Desc* d) {
    memset(d, 0, sizeof(*d));
    d->status = OMNI_JPEGDEC_CORRUPT;
    d->dev_off = -1;
    if (!f || size < 4 || f[0] != 0xff || f[1] != 0xd8) return d->status;
    uint8_t qt[4][64], hbits[2][4][16], hvals[2][4][256];
    bool qset[4] = {false, false, false, false}, hset[2][4] = {{false, false, false, false}, {false, false, false, false}};
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    bool frame = false;
    int64_t p = 2;
    auto fail = [&](int st) { d->status = st; return st; };
    for (;;) {
        if (p >= size || f[p] != 0xff) return fail(OMNI_JPEGDEC_CORRUPT);
        while (p < size && f[p] == 0xff) ++p;
        if (p >= size) return fail(OMNI_JPEGDEC_CORRUPT);
        const int m = f[p++];
        if (m == 0xd8 || m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;
        if (m == 0xd9 || m == 0x00) return fail(OMNI_JPEGDEC_CORRUPT);                      // no scan holds the first component
        if (p + 2 > size) return fail(OMNI_JPEGDEC_CORRUPT);
        const int64_t len = (int64_t)f[p] << 8 | f[p + 1];
        if (len < 2 || p + len > size) return fail(OMNI_JPEGDEC_CORRUPT);
        const uint8_t* s = f + p + 2;
        const int64_t n = len - 2;
        if (m == 0xdb) {                                                                   // DQT
            int64_t i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                if (tq > 3) return fail(OMNI_JPEGDEC_CORRUPT);
                if (pq == 1) return fail(OMNI_JPEGDEC_UNSUPPORTED);
                if (pq != 0 || i + 65 > n) return fail(OMNI_JPEGDEC_CORRUPT);
                for (int k = 0; k < 64; ++k) qt[tq][jp::kZigzag[k]] = s[i + 1 + k];
                qset[tq] = true;
                i += 65;
            }
        } else if (m == 0xc4) {                                                            // DHT
            int64_t i = 0;
            while (i < n) {
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3 || i + 17 > n) return fail(OMNI_JPEGDEC_CORRUPT);
                int cnt = 0;
                for (int k = 0; k < 16; ++k) cnt += s[i + 1 + k];
                if (cnt > 256 || i + 17 + cnt > n) return fail(OMNI_JPEGDEC_CORRUPT);
                memcpy(hbits[tc][th], s + i + 1, 16);
                memset(hvals[tc][th], 0, 256);
                memcpy(hvals[tc][th], s + i + 17, (size_t)cnt);
                hset[tc][th] = true;
                i += 17 + cnt;
            }
        } else if (m == 0xc0) {                                                            // SOF0
            if (frame || n < 6) return fail(OMNI_JPEGDEC_CORRUPT);
            if (s[0] != 8) return fail(OMNI_JPEGDEC_UNSUPPORTED);
            d->h = s[1] << 8 | s[2];
            d->w = s[3] << 8 | s[4];
            d->ncomp = s[5];
            if (d->w < 1 || d->h < 1) { d->w = d->h = 0; return fail(OMNI_JPEGDEC_CORRUPT); }
            if (d->ncomp != 1 && d->ncomp != 3) return fail(OMNI_JPEGDEC_UNSUPPORTED);
            if (n < 6 + 3 * d->ncomp) return fail(OMNI_JPEGDEC_CORRUPT);
            for (int c = 0; c < d->ncomp; ++c) {
                cid[c] = s[6 + 3 * c];
                ch[c] = s[7 + 3 * c] >> 4;
                cv[c] = s[7 + 3 * c] & 15;
                ctq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4 || ctq[c] > 3) return fail(OMNI_JPEGDEC_CORRUPT);
                if (ch[c] > ch[0] || cv[c] > cv[0]) return fail(OMNI_JPEGDEC_UNSUPPORTED);
            }
            frame = true;
        } else if (m >= 0xc1 && m <= 0xcf) {                                               // every other frame type, DAC (0xc8 is reserved)
            return fail(m == 0xc8 ? OMNI_JPEGDEC_CORRUPT : OMNI_JPEGDEC_UNSUPPORTED);
        } else if (m == 0xdd) {                                                            // DRI
            if (n < 2) return fail(OMNI_JPEGDEC_CORRUPT);
            d->restart = s[0] << 8 | s[1];
        } else if (m == 0xda) {                                                            // SOS
            if (!frame || n < 1) return fail(OMNI_JPEGDEC_CORRUPT);
            const int ns = s[0];
            if (ns < 1 || ns > d->ncomp || n < 1 + 2 * ns + 3) return fail(OMNI_JPEGDEC_CORRUPT);
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(OMNI_JPEGDEC_CORRUPT);
            const int64_t start = p + len, end = scan_end(f, size, start);
            if (s[1] != cid[0]) {                                                          // a scan without the first component: skipped
                d->multi_scan = 1;
                p = end;
                continue;
            }
            Tables& T = d->T;
            int at = 0, comp_of[3] = {0, 0, 0};
            for (int j = 0; j < ns; ++j) {
                int c = -1;
                for (int k = 0; k < d->ncomp; ++k)
                    if (cid[k] == s[1 + 2 * j]) c = k;
                if (c < j) return fail(OMNI_JPEGDEC_CORRUPT);                              // (unknown, or out of the frame's order)
                comp_of[j] = c;
                const int td = s[2 + 2 * j] >> 4, ta = s[2 + 2 * j] & 15;
                if (td > 3 || ta > 3 || !hset[0][td] || !hset[1][ta]) return fail(OMNI_JPEGDEC_CORRUPT);
                if (build_hufftab(hbits[0][td], hvals[0][td], true, &T.dc[j]) || build_hufftab(hbits[1][ta], hvals[1][ta], false, &T.ac[j]))
                    return fail(OMNI_JPEGDEC_CORRUPT);
                const int nb = ns == 1 ? 1 : ch[c] * cv[c];                                // (a scan of one component is not interleaved: one block per MCU)
                if (at + nb > JD_MAX_BPM) return fail(OMNI_JPEGDEC_CORRUPT);
                for (int k = 0; k < nb; ++k) T.blk_comp[at++] = (uint8_t)j;
            }
            if (!qset[ctq[0]]) return fail(OMNI_JPEGDEC_CORRUPT);
            for (int k = 0; k < 64; ++k) {
                d->q[k] = qt[ctq[0]][k];
                T.zz[k] = jp::kZigzag[k];
            }
            d->hs = ns == 1 ? 1 : ch[0];
            d->vs = ns == 1 ? 1 : cv[0];
            T.bpm = at;
            T.ny = d->hs * d->vs;
            d->mcus_x = (d->w + 8 * d->hs - 1) / (8 * d->hs);                              // (the first component has the frame's largest factors)
            d->mcus_y = (d->h + 8 * d->vs - 1) / (8 * d->vs);
            d->n_blocks = (uint32_t)d->mcus_x * d->mcus_y * at;
            d->n_yblocks = (uint32_t)d->mcus_x * d->mcus_y * T.ny;
            d->scan_off = start;
            d->scan_bytes = end - start;
            if (ns < d->ncomp) d->multi_scan = 1;
            bool dev = !d->multi_scan && d->hs <= 2 && d->vs <= 2;
            for (int j = 1; j < ns; ++j) dev = dev && ch[comp_of[j]] == 1 && cv[comp_of[j]] == 1;
            d->restart_only = dev && d->restart != 0;
            return fail(dev && d->restart == 0 ? OMNI_JPEGDEC_OK : OMNI_JPEGDEC_HOST);
        }
        // APPn, COM and anything else with a length: skipped
        p += len;
    }
}

// scan[0..n) of the file -> the clean bytes at out (room for n + JD_SCAN_PAD), JD_SCAN_PAD zero bytes behind them.  Returns their number.  rst (or null): the
// clean byte offset behind every restart marker, at most max_rst of them, *n_rst their number
inline int64_t unstuff(const uint8_t* s, int64_t n, uint8_t* out, int64_t* rst, int64_t max_rst, int64_t* n_rst) {
    int64_t i = 0, o = 0, r = 0;
    while (i < n) {
        const uint8_t c = s[i++];
        if (c != 0xff) { out[o++] = c; continue; }
        while (i < n && s[i] == 0xff) ++i;
        if (i >= n) break;
        const uint8_t m = s[i++];
        if (m == 0) out[o++] = 0xff;
        else if (m >= 0xd0 && m <= 0xd7) { if (rst && r < max_rst) rst[r++] = o; }
        else break;
    }
    memset(out + o, 0, JD_SCAN_PAD);
    if (n_rst) *n_rst = r;
    return o;
}

// ---- the same bytes by tiles: what a handle whose OMNI_JPEGDEC_UNSTUFF_DEV is 1 leaves to the device -------------------------------------------------------------
// unstuff() is a stream compaction with a one-byte neighbourhood rule.  The host keeps the part that needs the whole scan -- where it ends, how many clean bytes it
// has, where the restart markers stand, and how many clean bytes lie in front of every tile of JD_UNSTUFF_TILE raw bytes (survey: it visits the 0xFF bytes alone)
// -- and every tile can then be compacted on its own (unstuff_tiled_host by plain loops, jpegdec_unstuff_kernel by one workgroup per tile).
// Whether raw byte `cur` of [0, raw_end) is a clean byte, given its neighbours; one outside [0, raw_end) is passed as JD_UNSTUFF_OUTSIDE (neither 0x00 nor 0xFF):
//   cur != 0xFF  kept unless it stands behind an 0xFF: that byte is the stuffed 00 or the RSTn of the run in front of it (the run's terminator lies beyond raw_end)
//   cur == 0xFF  kept when a 00 follows: the last 0xFF of a run in front of a stuffed zero; fill bytes and marker prefixes are dropped
JP_HD bool unstuff_keep(uint8_t prev, uint8_t cur, uint8_t next) { return cur != 0xff ? prev != 0xff : next == 0x00; }

struct Survey {
    int64_t raw_end = 0;                                    // where unstuff() stops: the start of the 0xFF run that ends in a marker other than RSTn (or runs off the
                                                            // end of the scan); n when there is none
    int64_t n_clean = 0, n_rst = 0;                         // unstuff()'s return value and its *n_rst
    int64_t n_tiles = 1;                                    // tiles of [0, max(raw_end, 1)): an empty scan still has one
};
// The host pass over scan[0..n).  tile_off[t] (t < min(n_tiles, max_tiles)): the clean bytes in front of raw byte t * JD_UNSTUFF_TILE; rst as unstuff()'s
inline Survey survey(const uint8_t* s, int64_t n, uint32_t* tile_off, int64_t max_tiles, int64_t* rst, int64_t max_rst) {
    Survey v;
    int64_t i = 0, o = 0, t = 1;                            // o: the clean bytes in front of raw byte i; t: the next tile to be filled, at raw byte t * TILE
    if (max_tiles > 0) tile_off[0] = 0;
    // the tiles that start in [from, to): `clean` clean bytes lie in front of `from`, and every byte of [from, to) adds `each` (1: data; 0: a run of 0xFF)
    auto fill = [&](int64_t from, int64_t to, int64_t clean, int64_t each) {
        for (; t * JD_UNSTUFF_TILE < to; ++t)
            if (t < max_tiles) tile_off[t] = (uint32_t)(clean + (t * JD_UNSTUFF_TILE - from) * each);
    };
    v.raw_end = n;
    while (i < n) {
        const uint8_t* ff = static_cast<const uint8_t*>(memchr(s + i, 0xff, (size_t)(n - i)));
        const int64_t j = ff ? ff - s : n;                  // [i, j): data
        fill(i, j, o, 1);
        o += j - i;
        if (!ff) break;
        int64_t k = j + 1;
        while (k < n && s[k] == 0xff) ++k;                  // [j, k): the run; s[k]: what it announces
        const bool zero = k < n && s[k] == 0, restart = k < n && s[k] >= 0xd0 && s[k] <= 0xd7;
        if (!zero && !restart) { v.raw_end = j; break; }
        fill(j, k + 1, o, 0);                               // (a tile that starts at k, behind a run's last 0xFF, is filled below)
        if (zero) {
            if (k % JD_UNSTUFF_TILE == 0 && k / JD_UNSTUFF_TILE < max_tiles) tile_off[k / JD_UNSTUFF_TILE] = (uint32_t)(o + 1);
            ++o;
        } else if (rst && v.n_rst < max_rst) {
            rst[v.n_rst++] = o;
        }
        i = k + 1;
    }
    v.n_clean = o;
    v.n_tiles = ((v.raw_end > 1 ? v.raw_end : 1) + JD_UNSTUFF_TILE - 1) / JD_UNSTUFF_TILE;
    return v;
}
// what jpegdec_unstuff_kernel reads about one scan, in a table of its own (Desc stays what it was): byte offsets inside the handle's device block
struct UnstuffJob {
    int64_t raw_off, raw_bytes;                             // the scan as it stands in the file, [0, raw_end), 16-aligned and zero-padded to a multiple of 16
    int64_t clean_off, clean_bytes;                         // where its clean bytes go (Desc::dev_off) and their number; JD_SCAN_PAD zero bytes follow
    int64_t tile_off;                                       // uint32 [tiles]: survey()'s table
};
// one tile of the compaction, by plain loops: raw bytes [t * TILE, min((t + 1) * TILE, raw_end)) from clean offset `at`.  Returns the clean offset behind it
inline int64_t unstuff_tile_host(const uint8_t* s, int64_t raw_end, int64_t t, int64_t at, uint8_t* out) {
    const int64_t lo = t * JD_UNSTUFF_TILE, hi = lo + JD_UNSTUFF_TILE < raw_end ? lo + JD_UNSTUFF_TILE : raw_end;
    for (int64_t x = lo; x < hi; ++x) {
        const uint8_t prev = x > 0 ? s[x - 1] : JD_UNSTUFF_OUTSIDE, next = x + 1 < raw_end ? s[x + 1] : JD_UNSTUFF_OUTSIDE;
        if (unstuff_keep(prev, s[x], next)) out[at++] = s[x];
    }
    return at;
}
// The CPU stand-in for jpegdec_unstuff_kernel: every tile on its own from tile_off[t]; the last one also writes the JD_SCAN_PAD zero bytes.  out need not be
// zeroed (room for n_clean + JD_SCAN_PAD).  Returns the clean offset behind the last tile: unstuff()'s count when the table is survey()'s
inline int64_t unstuff_tiled_host(const uint8_t* s, const Survey& v, const uint32_t* tile_off, uint8_t* out) {
    int64_t end = 0;
    for (int64_t t = v.n_tiles - 1; t >= 0; --t) {          // (no order among the tiles: backwards, so that none relies on the one in front of it)
        const int64_t e = unstuff_tile_host(s, v.raw_end, t, (int64_t)tile_off[t], out);
        if (t == v.n_tiles - 1) {
            end = e;
            memset(out + v.n_clean, 0, JD_SCAN_PAD);
        }
    }
    return end;
}

// ---- the bit reader: a 64-bit window over the clean scan (host and device) -----------------------------------------------------------------------------
JP_HD uint32_t be32(const uint8_t* s, uint32_t word, uint32_t n_words) {                    // word `word` of the scan, MSB first; 0 beyond the padded scan
    if (word >= n_words) return 0u;
    const uint32_t v = reinterpret_cast<const uint32_t*>(s)[word];                         // (the scan starts on a 4-byte boundary)
    return __builtin_bswap32(v);
}
struct Bits {
    const uint8_t* s;
    uint32_t n_words, pos, next;                            // pos: the bit the window starts at; next: the word to load
    uint64_t win;                                           // `have` valid bits, left-aligned
    int have;
    JP_HD void init(const uint8_t* scan, uint32_t words, uint32_t bit) {
        s = scan; n_words = words; pos = bit;
        const uint32_t w0 = bit >> 5, sh = bit & 31;
        win = ((uint64_t)be32(s, w0, n_words) << 32 | be32(s, w0 + 1, n_words)) << sh;
        have = 64 - (int)sh;
        next = w0 + 2;
    }
    JP_HD uint32_t peek32() const { return (uint32_t)(win >> 32); }                         // (have >= 32 always)
    JP_HD void skip(int n) {                                                                // n <= 31
        win <<= n; have -= n; pos += (uint32_t)n;
        if (have < 32) {
            win |= (uint64_t)be32(s, next++, n_words) << (32 - have);
            have += 32;
        }
    }
};
// words a clean scan of `bytes` bytes occupies with its padding
JP_HD uint32_t scan_words(int64_t bytes) { return (uint32_t)((bytes + JD_SCAN_PAD) >> 2); }

// ---- the symbol step -------------------------------------------------------------------------------------------------------------------------------------
#define JD_STEP_ERR 1
#define JD_STEP_BLOCK 2
// em.put(block of the MCU, natural index, value).  Returns JD_STEP_ERR | JD_STEP_BLOCK (a block was completed)
template <class Emit>
JP_HD int step(const Tables& T, Bits& br, uint32_t total_bits, int& z, int& b, Emit& em) {
    const uint32_t v = br.peek32();
    const int comp = T.blk_comp[b];
    const HuffTab& t = z == 0 ? T.dc[comp] : T.ac[comp];
    int len = 0, sym = 0, res = 0;
    const uint32_t e = t.look[v >> 24];
    if (e) {
        len = (int)(e >> 8); sym = (int)(e & 255);
    } else {
        for (int l = 9; l <= 16; ++l) {
            const int code = (int)(v >> (32 - l));
            if (code <= t.maxcode[l]) { len = l; sym = t.vals[(code + t.valoff[l]) & 255]; break; }
        }
        if (!len) { len = 1; sym = 0; res = JD_STEP_ERR; }
    }
    const int n = sym & 15;
    const int r = n ? (int)((v << len) >> (32 - n)) : 0;
    const int val = n ? (r < (1 << (n - 1)) ? r - (1 << n) + 1 : r) : 0;
    if (br.pos + (uint32_t)(len + n) > total_bits) res = JD_STEP_ERR;
    br.skip(len + n);
    if (z == 0) {
        em.put(b, 0, val);
        z = 1;
    } else {
        const int run = sym >> 4;
        if (n == 0) {
            if (run == 15) z += 16;
            else { if (run) res = JD_STEP_ERR; z = 64; }
        } else {
            z += run;
            if (z > 63) { res = JD_STEP_ERR; z = 64; }
            else { em.put(b, T.zz[z], val); ++z; }
        }
    }
    if (z >= 64) {
        z = 0;
        b = b + 1 >= T.bpm ? 0 : b + 1;
        em.next_block();
        res |= JD_STEP_BLOCK;
    }
    return res;
}

// ---- subsequences ------------------------------------------------------------------------------------------------------------------------------------------
// a state between two subsequences: overhang (bits of the last symbol of i that lie in i + 1) | z << 6 | b << 12.  0: the guess
JP_HD uint16_t pack_state(uint32_t ov, int z, int b) { return (uint16_t)(ov | (uint32_t)z << 6 | (uint32_t)b << 12); }
struct NoEmit {
    JP_HD void put(int, int, int) {}
    JP_HD void next_block() {}
};
// The first component's coefficients into coef[block in scan order][64] (zeroed by the caller) and DC differences into dcd[block in scan order]; nothing is
// stored at or beyond block n_yblocks
struct CoefEmit {
    int16_t* coef;
    int32_t* dcd;
    uint32_t n_yblocks, ybase;                              // ybase: the first block of the first component in the current MCU
    int ny, bpm, b;
    JP_HD void start(const Tables& T, uint32_t first_block, int entry_b) {
        ny = T.ny; bpm = T.bpm; b = entry_b;
        ybase = first_block / (uint32_t)bpm * (uint32_t)ny;
    }
    JP_HD void put(int blk, int nat, int val) {
        const uint32_t y = ybase + (uint32_t)blk;
        if (blk >= ny || y >= n_yblocks) return;
        if (nat == 0) dcd[y] = val;
        else coef[(size_t)y * 64 + nat] = (int16_t)val;
    }
    JP_HD void next_block() {
        if (++b >= bpm) { b = 0; ybase += (uint32_t)ny; }
    }
};
// Subsequence i of the segment [seg_begin, seg_end) of the scan (absolute bit positions: a restart interval; the whole scan is the segment [0, total_bits)) from
// `entry`: the symbols that start in [seg_begin + i S + overhang, min(seg_begin + (i + 1) S, seg_end)), and none once first_block + (blocks completed) reaches
// max_blocks.  seg_end is step()'s end of the data.  Returns the blocks completed; *exit_state, *err (any JD_STEP_ERR among its steps)
template <class Emit>
JP_HD uint32_t decode_subseq_seg(const Tables& T, const uint8_t* scan, uint32_t n_words, uint32_t seg_begin, uint32_t seg_end, uint32_t i, uint32_t S, uint16_t entry,
                                 uint32_t first_block, uint32_t max_blocks, Emit& em, uint16_t* exit_state, int* err) {
    const uint32_t bound = seg_begin + (i + 1) * S, end = bound < seg_end ? bound : seg_end;
    int z = (entry >> 6) & 63, b = entry >> 12, e = 0;
    uint32_t blocks = 0;
    Bits br;
    br.init(scan, n_words, seg_begin + i * S + (entry & 63u));
    while (br.pos < end && first_block + blocks < max_blocks) {
        const int r = step(T, br, seg_end, z, b, em);
        e |= r & JD_STEP_ERR;
        blocks += (uint32_t)(r >> 1);
    }
    *exit_state = pack_state(br.pos > bound ? br.pos - bound : 0u, z, b);
    *err = e;
    return blocks;
}
// ... of the whole scan
template <class Emit>
JP_HD uint32_t decode_subseq(const Tables& T, const uint8_t* scan, uint32_t n_words, uint32_t total_bits, uint32_t i, uint32_t S, uint16_t entry, uint32_t first_block,
                             uint32_t max_blocks, Emit& em, uint16_t* exit_state, int* err) {
    return decode_subseq_seg(T, scan, n_words, 0u, total_bits, i, S, entry, first_block, max_blocks, em, exit_state, err);
}
// the subsequence length an image is decoded with: the configured one, doubled until there are at most max_sub subsequences
JP_HD uint32_t subseq_bits_for(uint32_t total_bits, uint32_t S, uint32_t max_sub) {
    while (S < (1u << 30) && (total_bits + S - 1) / S > max_sub) S <<= 1;
    return S;
}

// ---- a picture without a restart interval over several workgroups: the partition ----------------------------------------------------------------------------------
// the subsequence length of a handle whose OMNI_JPEGDEC_PLAIN_WGS is W: the configured one, doubled only until W chunks of at most max_sub hold the picture
JP_HD uint32_t plain_subseq_bits(uint32_t total_bits, uint32_t S, uint32_t W, uint32_t max_sub) {
    const uint64_t room = (uint64_t)W * max_sub;
    return subseq_bits_for(total_bits, S, room > 0xffffffffull ? 0xffffffffu : (uint32_t)room);
}
// the chunks of a picture of n_sub subsequences: at least one, none empty
JP_HD uint32_t plain_chunks(uint32_t n_sub, uint32_t W) { return n_sub < W ? (n_sub ? n_sub : 1u) : (W ? W : 1u); }
// chunk c of C holds the subsequences [plain_chunk_begin(c), plain_chunk_begin(c + 1)); c == C: n_sub
JP_HD uint32_t plain_chunk_begin(uint32_t c, uint32_t n_sub, uint32_t C) { return (uint32_t)((uint64_t)c * n_sub / C); }
// a subsequence's words between the chunk relaxation, the seam relaxation and the write pass ([image][subsequence]: exit state, entry used, block count).  The
// seam relaxation keeps two marks in a count's top bits; a subsequence of at most 2^30 bits completes fewer than 2^30 blocks
#define JD_SEAM_NEED 0x80000000u                             // its predecessor's exit differs from the entry it last used: decode it again in this round
#define JD_SEAM_CHANGED 0x40000000u                          // the seam relaxation changed its exit state or its count at least once
#define JD_SEAM_COUNT 0x3fffffffu

// ---- restart intervals ---------------------------------------------------------------------------------------------------------------------------------------
// one interval of a planned restart file: its bits on the clean scan (absolute), its first subsequence (numbered through the picture) and its first block.  The
// table ends with a sentinel {total_bits, total_bits, n_sub, n_blocks}: interval k's subsequences are [first_sub, [k + 1].first_sub), its blocks likewise
struct Interval { uint32_t bit_begin, bit_end, first_sub, first_block; };
// the interval among [lo, hi) that holds subsequence g (first_sub is increasing; [lo].first_sub <= g)
JP_HD uint32_t interval_of(const Interval* iv, uint32_t lo, uint32_t hi, uint32_t g) {
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (iv[mid].first_sub <= g) lo = mid; else hi = mid;
    }
    return lo;
}
// subsequences of an interval of `bits` bits: at least one
JP_HD uint32_t interval_subs(uint32_t bits, uint32_t S) { return bits ? (bits + S - 1) / S : 1u; }

// ---- the block: dequantise, islow IDCT, level shift, clamp ---------------------------------------------------------------------------------------------------
JP_HD int32_t jd_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }
// one pass of jidctint.c over 8 values (stride st) of in -> out
template <int kShift>
JP_HD void idct_1d(const uint32_t* in, uint32_t* out, int st) {
    uint32_t z2 = in[2 * st], z3 = in[6 * st];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 + z3 * (uint32_t)(-15137), tmp3 = z1 + z2 * 6270u;
    z2 = in[0]; z3 = in[4 * st];
    uint32_t tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7 * st]; tmp1 = in[5 * st]; tmp2 = in[3 * st]; tmp3 = in[st];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u; tmp1 *= 16819u; tmp2 *= 25172u; tmp3 *= 12299u;
    z1 *= (uint32_t)(-7373); z2 *= (uint32_t)(-20995); z3 *= (uint32_t)(-16069); z4 *= (uint32_t)(-3196);
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = (uint32_t)jd_descale(tmp10 + tmp3, kShift);
    out[7 * st] = (uint32_t)jd_descale(tmp10 - tmp3, kShift);
    out[st] = (uint32_t)jd_descale(tmp11 + tmp2, kShift);
    out[6 * st] = (uint32_t)jd_descale(tmp11 - tmp2, kShift);
    out[2 * st] = (uint32_t)jd_descale(tmp12 + tmp1, kShift);
    out[5 * st] = (uint32_t)jd_descale(tmp12 - tmp1, kShift);
    out[3 * st] = (uint32_t)jd_descale(tmp13 + tmp0, kShift);
    out[4 * st] = (uint32_t)jd_descale(tmp13 - tmp0, kShift);
}
// coef: a block's 64 coefficients in natural order ([0] is not read), dc its DC value, q the table -> rows[j]: row j's 8 pixels, pixel i in bits 8 i
JP_HD void idct_block(const int16_t* coef, int32_t dc, const uint16_t* q, uint64_t* rows) {
    uint32_t ws[64];
    JP_UNROLL
    for (int i = 0; i < 64; ++i) ws[i] = (uint32_t)(int32_t)(i == 0 ? dc : (int32_t)coef[i]) * (uint32_t)q[i];
    JP_UNROLL
    for (int c = 0; c < 8; ++c) idct_1d<11>(ws + c, ws + c, 8);
    JP_UNROLL
    for (int r = 0; r < 8; ++r) {
        idct_1d<18>(ws + 8 * r, ws + 8 * r, 1);
        uint64_t row = 0;
        JP_UNROLL
        for (int i = 0; i < 8; ++i) {
            const int32_t v = (int32_t)ws[8 * r + i] + 128;
            row |= (uint64_t)(v < 0 ? 0 : v > 255 ? 255 : v) << (8 * i);
        }
        rows[r] = row;
    }
}
// where block y of the first component (scan order) lies in the picture, in blocks
JP_HD void yblock_pos(uint32_t y, int hs, int vs, int mcus_x, int* bx, int* by) {
    const uint32_t ny = (uint32_t)(hs * vs), mcu = y / ny, k = y % ny;
    *bx = (int)(mcu % (uint32_t)mcus_x) * hs + (int)(k % (uint32_t)hs);
    *by = (int)(mcu / (uint32_t)mcus_x) * vs + (int)(k / (uint32_t)hs);
}
// block (bx, by)'s rows into the picture, cropped to w x h
JP_HD void store_block(const uint64_t* rows, uint8_t* out, int64_t stride, int w, int h, int bx, int by) {
    JP_UNROLL
    for (int j = 0; j < 8; ++j) {
        const int y = by * 8 + j;
        if (y >= h) break;
        uint8_t* o = out + (int64_t)y * stride + bx * 8;
        if (bx * 8 + 8 <= w && ((uintptr_t)o & 7) == 0) {
            *reinterpret_cast<uint64_t*>(o) = rows[j];
        } else {
            for (int i = 0; i < 8 && bx * 8 + i < w; ++i) o[i] = (uint8_t)(rows[j] >> (8 * i));
        }
    }
}
// phases 5 + 6 for block y, given the scanned DC values
JP_HD void block_out(const Desc& d, const int16_t* coef, const int32_t* dcv, uint32_t y, bool zero, uint8_t* out, int64_t stride) {
    int bx, by;
    yblock_pos(y, d.hs, d.vs, d.mcus_x, &bx, &by);
    if (bx * 8 >= d.w || by * 8 >= d.h) return;                                            // MCU padding
    uint64_t rows[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!zero) idct_block(coef + (size_t)y * 64, dcv[y], d.q, rows);
    store_block(rows, out, stride, d.w, d.h, bx, by);
}

}  // namespace jd
}  // namespace omni

// ---- the host decoders (they allocate) -----------------------------------------------------------------------------------------------------------------------
#include <vector>
namespace omni {
namespace jd {

inline void zero_picture(uint8_t* out, int64_t stride, int w, int h) {
    for (int y = 0; y < h; ++y) memset(out + (int64_t)y * stride, 0, (size_t)w);
}

// The sequential decoder of a parsed file (status OK or HOST): restart intervals included.  out: d.w x d.h pixels, `stride` bytes between rows.  Returns
// d.status, or OMNI_JPEGDEC_CORRUPT with the picture all zeros.
inline int decode_sequential(const uint8_t* file, const Desc& d, uint8_t* out, int64_t stride) {
    std::vector<uint8_t> clean((size_t)d.scan_bytes + JD_SCAN_PAD + 4);
    std::vector<int64_t> rst((size_t)(d.scan_bytes / 2 + 1));
    int64_t n_rst = 0;
    const int64_t nclean = unstuff(file + d.scan_off, d.scan_bytes, clean.data(), rst.data(), (int64_t)rst.size(), &n_rst);
    const uint32_t total_bits = (uint32_t)(nclean * 8), n_words = scan_words(nclean);
    struct BlockEmit {
        int16_t blk[64];
        int32_t diff;
        int ny;
        void put(int b, int nat, int val) {
            if (b >= ny) return;
            if (nat == 0) diff = val;
            else blk[nat] = (int16_t)val;
        }
        void next_block() {}
    } em;
    memset(em.blk, 0, sizeof(em.blk));
    em.diff = 0; em.ny = d.T.ny;
    Bits br;
    br.init(clean.data(), n_words, 0);
    int z = 0, b = 0, err = 0;
    uint32_t g = 0, pred = 0, ybase = 0;
    int64_t seg = 0;
    const uint32_t per_restart = d.restart ? (uint32_t)d.restart * (uint32_t)d.T.bpm : 0u;
    while (g < d.n_blocks) {
        if (br.pos >= total_bits) { err = 1; break; }
        const int blk = b;
        const int r = step(d.T, br, total_bits, z, b, em);
        err |= r & JD_STEP_ERR;
        if (!(r & JD_STEP_BLOCK)) continue;
        if (blk < d.T.ny) {
            pred += (uint32_t)em.diff;
            uint64_t rows[8];
            idct_block(em.blk, (int32_t)pred, d.q, rows);
            int bx, by;
            yblock_pos(ybase + (uint32_t)blk, d.hs, d.vs, d.mcus_x, &bx, &by);
            if (bx * 8 < d.w && by * 8 < d.h) store_block(rows, out, stride, d.w, d.h, bx, by);
            memset(em.blk, 0, sizeof(em.blk));
            em.diff = 0;
        }
        ++g;
        if (b == 0) ybase += (uint32_t)d.T.ny;
        if (per_restart && g < d.n_blocks && g % per_restart == 0) {                        // the next interval starts behind the next restart marker
            if (seg >= n_rst) { err = 1; break; }
            br.init(clean.data(), n_words, (uint32_t)(rst[(size_t)seg++] * 8));
            z = 0; b = 0; pred = 0;
        }
    }
    if (err) {
        zero_picture(out, stride, d.w, d.h);
        return OMNI_JPEGDEC_CORRUPT;
    }
    return d.status;
}

// file -> gray picture.  *w, *h: the frame's size (0 x 0 when no frame header could be read).  out may be null (classification only); otherwise it has room for
// the picture at `stride` >= *w ... which the caller can only know from a first call: max_w / max_h bound what is written (a larger picture: -1).
// Returns OMNI_JPEGDEC_OK / HOST (decoded), UNSUPPORTED (nothing written), CORRUPT (zeros when the size is known).
inline int jpeg_decode_host(const uint8_t* file, int64_t size, uint8_t* out, int64_t stride, int max_w, int max_h, int* w, int* h) {
    Desc d;
    const int st = parse(file, size, &d);
    if (w) *w = d.w;
    if (h) *h = d.h;
    if (!out || st == OMNI_JPEGDEC_UNSUPPORTED) return st;
    if (d.w > max_w || d.h > max_h || stride < d.w) return -1;
    if (st == OMNI_JPEGDEC_CORRUPT) {
        zero_picture(out, stride, d.w, d.h);
        return st;
    }
    return decode_sequential(file, d, out, stride);
}

// ---- restart-interval files over several workgroups: the chunk plan ----------------------------------------------------------------------------------------------
struct ChunkPlan {
    int status = OMNI_JPEGDEC_HOST;                         // OK: planned; HOST: cannot be planned; CORRUPT: fewer restart markers than the picture needs
    uint32_t subseq_bits = 0, n_sub = 0, n_int = 0, n_chunks = 0, max_chunk_sub = 0;
    std::vector<Interval> iv;                               // n_int + 1 (sentinel)
    std::vector<uint32_t> chunk_first;                      // n_chunks + 1: chunk c holds the intervals [chunk_first[c], chunk_first[c + 1])
    size_t table_bytes() const { return iv.size() * sizeof(Interval) + chunk_first.size() * sizeof(uint32_t); }
    void store(uint8_t* at) const {                         // the form the kernel reads (Desc::tab_off; 4-byte aligned)
        memcpy(at, iv.data(), iv.size() * sizeof(Interval));
        memcpy(at + iv.size() * sizeof(Interval), chunk_first.data(), chunk_first.size() * sizeof(uint32_t));
    }
};
// The plan of a parsed restart file (d.restart != 0) whose clean scan has nclean bytes and whose restart markers stood at the clean byte offsets rst[0..n_rst):
// intervals of S bits per subsequence in at most W chunks of consecutive intervals, balanced by bits, each of at most max_sub subsequences (S is doubled until
// that holds; every interval costs at least one, so a chunk of more than max_sub intervals cannot be planned)
inline void plan_chunks(const Desc& d, int64_t nclean, const int64_t* rst, int64_t n_rst, uint32_t S, uint32_t W, uint32_t max_sub, ChunkPlan* p) {
    *p = ChunkPlan();
    const uint32_t mcus = (uint32_t)d.mcus_x * (uint32_t)d.mcus_y, restart = (uint32_t)d.restart;
    if (!restart || !mcus || !W || !max_sub || nclean < 0 || nclean > (1 << 28)) return;
    const uint32_t n_int = (mcus + restart - 1) / restart, total_bits = (uint32_t)(nclean * 8);
    if (n_rst < (int64_t)n_int - 1) { p->status = OMNI_JPEGDEC_CORRUPT; return; }
    p->n_int = n_int;
    p->iv.resize((size_t)n_int + 1);
    std::vector<uint32_t> chunk_of(n_int);
    uint32_t n_chunks = 0, in_chunk = 0, max_in_chunk = 0, max_bits = 0;
    for (uint32_t k = 0; k < n_int; ++k) {
        Interval& I = p->iv[k];
        I.bit_begin = k ? (uint32_t)(rst[k - 1] * 8) : 0u;
        I.bit_end = k + 1 < n_int ? (uint32_t)(rst[k] * 8) : total_bits;
        I.first_block = k * restart * (uint32_t)d.T.bpm;
        if (I.bit_end - I.bit_begin > max_bits) max_bits = I.bit_end - I.bit_begin;
        uint32_t c = total_bits ? (uint32_t)((uint64_t)I.bit_begin * W / total_bits) : 0u;
        if (c >= W) c = W - 1;
        if (k == 0 || c != chunk_of[k - 1]) {               // (c never decreases: the offsets never do)
            p->chunk_first.push_back(k);
            ++n_chunks;
            in_chunk = 0;
        }
        chunk_of[k] = c;
        if (++in_chunk > max_in_chunk) max_in_chunk = in_chunk;
    }
    p->chunk_first.push_back(n_int);
    p->n_chunks = n_chunks;
    if (max_in_chunk > max_sub) return;                                                     // HOST
    for (;; S <<= 1) {
        uint32_t sub = 0, worst = 0;
        for (uint32_t c = 0; c < n_chunks; ++c) {
            const uint32_t before = sub;
            for (uint32_t k = p->chunk_first[c]; k < p->chunk_first[c + 1]; ++k) {
                p->iv[k].first_sub = sub;
                sub += interval_subs(p->iv[k].bit_end - p->iv[k].bit_begin, S);
            }
            if (sub - before > worst) worst = sub - before;
        }
        p->n_sub = sub;
        p->max_chunk_sub = worst;
        if (worst <= max_sub) break;
        if (S >= (1u << 30) || S >= max_bits) return;                                       // (cannot happen: S >= max_bits makes every interval one subsequence)
    }
    p->subseq_bits = S;
    p->iv[n_int] = Interval{total_bits, total_bits, p->n_sub, d.n_blocks};
    p->status = OMNI_JPEGDEC_OK;
}

// phase 5 with a restart interval: the running sum starts again every `seg` blocks of the first component (seg = restart * ny; 0: never)
inline void dc_scan_host(int32_t* dc, uint32_t n, uint32_t seg) {
    uint32_t run = 0;
    for (uint32_t y = 0; y < n; ++y) {
        if (seg && y % seg == 0) run = 0;
        run += (uint32_t)dc[y];
        dc[y] = (int32_t)run;
    }
}

// ---- the CPU stand-in for the kernels ------------------------------------------------------------------------------------------------------------------------------
struct PlannedStats {
    uint32_t n_sub = 0, subseq_bits = 0, n_chunks = 0, chunk_rounds = 0;      // chunk_rounds: the maximum over the chunks of the rounds that changed something
    uint32_t seam_rounds = 0, seam_changed = 0, seam_chunks = 0;              // seam relaxation: rounds that changed something, subsequences it changed at least
};                                                                            // once, and the chunks those lie in
// The phase functions by plain loops, in the kernels' order, for a handle whose switches are restart_wgs and plain_wgs, with S bits per subsequence (a power of
// two) and workgroups of max_sub subsequences.  A picture is an Interval table and chunk bounds in subsequence numbers: a planned restart file has plan_chunks'
// table and chunks; every other file is ONE interval over the whole scan, cut into plain_chunks' chunks (plain_wgs >= 2 and status OK; S from plain_subseq_bits)
// or one chunk (S from subseq_bits_for).  1 every subsequence from the guess; 2 Jacobi rounds inside each chunk until nothing changes -- a subsequence that
// starts an interval keeps entry 0, a chunk's first one the entry it has -- and, where the chunks cut an interval, once more over the whole picture (the seam
// relaxation); 3 the exclusive scan of the counts inside every interval; 4 the write pass, every interval bounded to its own blocks; 5-6.  CORRUPT: a step error
// on the true chain, an interval whose last subsequence ends short of its blocks, no subsequence at all.
// Files the kernels do not take go where a handle sends them: UNSUPPORTED and CORRUPT at parse as jpeg_decode_host; a restart file that the switch or
// !restart_only leaves on the host, or whose plan is HOST: decode_sequential; a plan that is CORRUPT: zeros.  A HOST file without a restart interval takes the
// one-chunk path all the same and stays HOST (its statistics are reported with both switches off only: a handle decodes it on the host).
inline int decode_planned_host(const uint8_t* file, int64_t size, uint32_t S, uint32_t restart_wgs, uint32_t plain_wgs, uint32_t max_sub, uint8_t* out, int64_t stride,
                               int max_w, int max_h, int* w, int* h, PlannedStats* stats) {
    Desc d;
    const int st = parse(file, size, &d);
    if (stats) *stats = PlannedStats();
    if (!out || (st != OMNI_JPEGDEC_OK && st != OMNI_JPEGDEC_HOST) || (d.restart && !(restart_wgs && d.restart_only)) || d.w > max_w || d.h > max_h || stride < d.w)
        return jpeg_decode_host(file, size, out, stride, max_w, max_h, w, h);               // not the kernels' to decode (or no room for it: -1)
    if (w) *w = d.w;
    if (h) *h = d.h;
    std::vector<uint8_t> clean((size_t)d.scan_bytes + JD_SCAN_PAD + 4);
    std::vector<int64_t> rst(d.restart ? (size_t)(d.scan_bytes / 2 + 1) : 0);
    int64_t n_rst = 0;
    const int64_t nclean = unstuff(file + d.scan_off, d.scan_bytes, clean.data(), rst.data(), (int64_t)rst.size(), &n_rst);
    const uint32_t total_bits = (uint32_t)(nclean * 8), n_words = scan_words(nclean);
    // the picture as a table: intervals, and chunk c = the subsequences [bound[c], bound[c + 1])
    std::vector<Interval> iv;
    std::vector<uint32_t> bound;
    if (d.restart) {
        ChunkPlan P;
        plan_chunks(d, nclean, rst.data(), n_rst, S, restart_wgs, max_sub, &P);
        if (P.status == OMNI_JPEGDEC_CORRUPT) zero_picture(out, stride, d.w, d.h);
        if (P.status != OMNI_JPEGDEC_OK) return P.status == OMNI_JPEGDEC_CORRUPT ? OMNI_JPEGDEC_CORRUPT : decode_sequential(file, d, out, stride);
        S = P.subseq_bits;
        iv = P.iv;
        for (uint32_t k : P.chunk_first) bound.push_back(iv[k].first_sub);
    } else {
        const bool spread = plain_wgs >= 2 && st == OMNI_JPEGDEC_OK;
        S = spread ? plain_subseq_bits(total_bits, S, plain_wgs, max_sub) : subseq_bits_for(total_bits, S, max_sub);
        const uint32_t n_sub = (total_bits + S - 1) / S, C = spread ? plain_chunks(n_sub, plain_wgs) : 1u;
        iv = {Interval{0u, total_bits, 0u, 0u}, Interval{total_bits, total_bits, n_sub, d.n_blocks}};
        for (uint32_t c = 0; c <= C; ++c) bound.push_back(plain_chunk_begin(c, n_sub, C));
    }
    const uint32_t n_int = (uint32_t)iv.size() - 1, C = (uint32_t)bound.size() - 1, N = iv[n_int].first_sub;
    std::vector<uint16_t> ex(N), used(N, 0);
    std::vector<uint32_t> cnt(N), of(N);                                                    // of: the interval a subsequence lies in
    std::vector<uint8_t> need(N), moved(N, 0);
    for (uint32_t k = 0, i = 0; k < n_int; ++k)
        for (; i < iv[k + 1].first_sub; ++i) of[i] = k;
    NoEmit none;
    int e;
    auto run = [&](uint32_t i, uint16_t entry, uint32_t first_block, uint32_t max_blocks, auto& em, uint16_t* x) {
        const Interval& I = iv[of[i]];
        return decode_subseq_seg(d.T, clean.data(), n_words, I.bit_begin, I.bit_end, i - I.first_sub, S, entry, first_block, max_blocks, em, x, &e);
    };
    // Jacobi rounds over the subsequences [lo, hi), lo keeping its entry: the rounds that changed something
    auto relax = [&](uint32_t lo, uint32_t hi, bool mark) {
        uint32_t rounds = 0;
        for (uint32_t r = 0; r < hi - lo; ++r) {
            for (uint32_t i = lo + 1; i < hi; ++i) {
                need[i] = i != iv[of[i]].first_sub && ex[i - 1] != used[i];
                if (need[i]) used[i] = ex[i - 1];
            }
            bool changed = false;
            for (uint32_t i = lo + 1; i < hi; ++i) {
                if (!need[i]) continue;
                uint16_t x;
                const uint32_t n = run(i, used[i], 0u, 0xffffffffu, none, &x);
                if (x != ex[i] || n != cnt[i]) { ex[i] = x; cnt[i] = n; changed = true; if (mark) moved[i] = 1; }
            }
            if (!changed) break;
            ++rounds;
        }
        return rounds;
    };
    PlannedStats ps;
    ps.n_sub = N; ps.subseq_bits = S; ps.n_chunks = C;
    for (uint32_t i = 0; i < N; ++i) cnt[i] = run(i, 0, 0u, 0xffffffffu, none, &ex[i]);     // 1
    bool cut = false;                                                                       // a chunk starts inside an interval
    for (uint32_t c = 0; c < C; ++c) {                                                      // 2
        const uint32_t rounds = relax(bound[c], bound[c + 1], false);
        if (rounds > ps.chunk_rounds) ps.chunk_rounds = rounds;
        if (bound[c] < N && bound[c] != iv[of[bound[c]]].first_sub) cut = true;
    }
    if (cut) ps.seam_rounds = relax(0, N, true);
    for (uint32_t c = 0; c < C; ++c) {
        uint32_t n = 0;
        for (uint32_t i = bound[c]; i < bound[c + 1]; ++i) n += moved[i];
        ps.seam_changed += n;
        ps.seam_chunks += n != 0;
    }
    if (stats && (st == OMNI_JPEGDEC_OK || d.restart || (!restart_wgs && !plain_wgs))) *stats = ps;
    std::vector<int16_t> coef((size_t)d.n_yblocks * 64, 0);
    std::vector<int32_t> dc(d.n_yblocks, 0);
    int err = N == 0;
    for (uint32_t i = 0, fb = 0; i < N; ++i) {                                              // 3 + 4: fb, the subsequence's first block
        const uint32_t max_blocks = iv[of[i] + 1].first_block;
        if (i == iv[of[i]].first_sub) fb = iv[of[i]].first_block;
        CoefEmit em;
        em.coef = coef.data(); em.dcd = dc.data(); em.n_yblocks = d.n_yblocks;
        em.start(d.T, fb, used[i] >> 12);
        uint16_t x;
        const uint32_t wrote = run(i, used[i], fb, max_blocks, em, &x);
        err |= e;
        if (i + 1 == iv[of[i] + 1].first_sub && fb + wrote < max_blocks) err = 1;           // the interval ends short of its blocks
        fb += cnt[i];
    }
    dc_scan_host(dc.data(), d.n_yblocks, (uint32_t)d.restart * (uint32_t)d.T.ny);           // 5
    for (uint32_t y = 0; y < d.n_yblocks; ++y) block_out(d, coef.data(), dc.data(), y, err != 0, out, stride);      // 6
    return err ? OMNI_JPEGDEC_CORRUPT : d.restart ? OMNI_JPEGDEC_OK : st;
}

// For the record of the one-chunk path (S doubled until there are at most max_sub subsequences): how many subsequences leave phase 1 -- every one from the
// guess -- with an exit state other than the true chain's.  0 for a file that path does not take
inline uint32_t wrong_after_first(const uint8_t* file, int64_t size, uint32_t S, uint32_t max_sub) {
    Desc d;
    const int st = parse(file, size, &d);
    if ((st != OMNI_JPEGDEC_OK && st != OMNI_JPEGDEC_HOST) || d.restart) return 0;
    std::vector<uint8_t> clean((size_t)d.scan_bytes + JD_SCAN_PAD + 4);
    const int64_t nclean = unstuff(file + d.scan_off, d.scan_bytes, clean.data(), nullptr, 0, nullptr);
    const uint32_t total_bits = (uint32_t)(nclean * 8), n_words = scan_words(nclean);
    S = subseq_bits_for(total_bits, S, max_sub);
    NoEmit none;
    uint32_t wrong = 0;
    uint16_t chain = 0, guessed;
    for (uint32_t i = 0, N = (total_bits + S - 1) / S; i + 1 < N; ++i) {                    // (all but the last subsequence)
        int e;
        decode_subseq(d.T, clean.data(), n_words, total_bits, i, S, 0, 0u, 0xffffffffu, none, &guessed, &e);
        decode_subseq(d.T, clean.data(), n_words, total_bits, i, S, chain, 0u, 0xffffffffu, none, &chain, &e);
        wrong += chain != guessed;
    }
    return wrong;
}

}  // namespace jd
}  // namespace omni
