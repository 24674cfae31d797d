// jpeg_dec_pack.h -- the block a decoder handle (jpeg_dec.hip) uploads for a batch of files, stated once: how much room a handle needs, which files it refuses, what
// every picture is classified and planned as, and where every byte the kernels dereference lies.  Plain C++ for g++ AND hipcc, nothing of HIP or of the handle:
// jpeg_dec.hip calls pack_room when a handle is made and pack_parse + pack_fill for every batch; tests/cpp/jpegdec_pack_pin.cpp runs the same three into a heap
// block of exactly in_bytes under -fsanitize=address,undefined and checks every offset they hand to the kernels.
// Two layouts, every region 16-aligned:
//   clean  (OMNI_JPEGDEC_UNSTUFF_DEV = 0)  descriptors | per picture, in order: its clean scan (+ a planned restart file's tables), or its host-decoded pixels
//   raw    (OMNI_JPEGDEC_UNSTUFF_DEV = 1)  descriptors | jobs | tile tables | interval tables | host-decoded pixels | raw scans || clean areas
//          [0, upload_bytes) ends behind the raw scans; the clean areas (Desc::dev_off) follow it, jpegdec_unstuff_kernel's to write, and end at clean_end
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "jpeg_dec_plan.h"

namespace omni {
namespace jd {

// what a handle snapshots when it is made
struct PackConfig {
    int w = 0, h = 0, max_images = 0;
    int64_t capacity = 0;                                   // bytes of a file, at most (a larger one is decoded on the host)
    int subseq_bits = 0, restart_wgs = 0, plain_wgs = 0, unstuff_dev = 0;
};
// ... and the room it allocates for it
struct PackRoom {
    uint32_t nyb_max = 0;                                   // blocks of the first component of a w x h picture with 16 x 16 MCUs
    size_t tab_bytes = 0, in_bytes = 0;                     // one picture's interval and chunk tables (restart_wgs >= 1); the block
    uint32_t state_cap = 0;                                 // plain_wgs >= 2: subsequences of a spread picture, at most
};
struct PackRefusal { int code = OMNI_OK; std::string message; };
// pack_parse's: every file's descriptor, classified against the handle, and its size
struct PackBatch { std::vector<Desc> descs; std::vector<int64_t> sizes; };
// what a launch needs to know about the block pack_fill wrote
struct PackResult {
    size_t upload_bytes = 0;
    int max_chunks = 1;                                     // the most chunks of a picture the entropy kernel decodes (its grid)
    int spread_chunks = 0;                                  // ... of a picture that takes the spread path (the chunk kernel's grid; 0: none does)
    uint32_t spread_sub = 0;                                // ... and the most subsequences of one (the write kernel's grid)
    bool unspread = true;                                   // a picture is decoded by the entropy kernel (plain_wgs < 2: launched whatever the batch holds)
    // the raw layout alone (0 in the clean one)
    size_t jobs_off = 0; int n_jobs = 0;                    // UnstuffJob[n_jobs]: the pictures whose scan the device unstuffs
    int64_t job_tiles = 0, raw_bytes = 0, clean_bytes = 0;  // the most tiles of a job; the raw bytes uploaded for all of them, the clean bytes they become
    size_t clean_end = 0;                                   // the end of the last clean area
};

inline size_t pack_align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline int64_t pack_nyb(int w, int h) { return (int64_t)((w + 15) / 16) * ((h + 15) / 16) * 4; }

// Per image: a descriptor, the larger of a clean scan and the picture itself, with restart_wgs on its interval and chunk tables (one interval per MCU of 8 x 8 at
// the most, and no more than the chunks hold); with unstuff_dev on also its raw scan next to its clean one, a job and a tile table
inline PackRoom pack_room(const PackConfig& c) {
    PackRoom r;
    const size_t n = (size_t)c.max_images, cap = (size_t)c.capacity, W = (size_t)c.restart_wgs;
    r.nyb_max = (uint32_t)pack_nyb(c.w, c.h);
    const size_t per_scan = pack_align16(cap + JD_SCAN_PAD), per_px = pack_align16((size_t)c.w * c.h);
    if (W) {
        const size_t mcus = (size_t)((c.w + 7) / 8) * ((c.h + 7) / 8), planned = W * JD_MAX_SUBSEQ;
        r.tab_bytes = pack_align16(((mcus < planned ? mcus : planned) + 1) * sizeof(Interval) + (W + 1) * sizeof(uint32_t));
    }
    r.in_bytes = pack_align16(n * sizeof(Desc)) + n * ((per_scan > per_px ? per_scan : per_px) + r.tab_bytes);
    if (c.unstuff_dev) {
        const size_t tile_tab = (cap / JD_UNSTUFF_TILE + 2) * sizeof(uint32_t);
        r.in_bytes += n * (pack_align16(cap) + 16) + pack_align16(n * sizeof(UnstuffJob)) + pack_align16(n * tile_tab);
    }
    if (c.plain_wgs >= 2) r.state_cap = (uint32_t)c.plain_wgs * JD_MAX_SUBSEQ;
    return r;
}

inline int pack_refuse(PackRefusal* r, int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    r->code = code; r->message = buf;
    return code;
}

// Parses and classifies every file; touches no block.  Returns OMNI_OK, or the refusal's code
inline int pack_parse(const PackConfig& c, const PackRoom& room, const uint8_t* const* files, const int64_t* sizes, int n, PackBatch* batch, PackRefusal* refusal) {
    batch->descs.resize((size_t)n);
    batch->sizes.assign(sizes, sizes + n);
    for (int i = 0; i < n; ++i) {
        if (!files[i] || sizes[i] < 0) return pack_refuse(refusal, OMNI_ERR_INVALID, "omni_jpegdec: file %d is null", i);
        Desc& D = batch->descs[(size_t)i];
        const int st = parse(files[i], sizes[i], &D);
        if (st == OMNI_JPEGDEC_UNSUPPORTED)
            return pack_refuse(refusal, OMNI_ERR_INVALID, "omni_jpegdec: file %d is not a baseline JPEG of 1 or 3 components (UNSUPPORTED)", i);
        if (!((D.w == c.w && D.h == c.h) || (st == OMNI_JPEGDEC_CORRUPT && D.w == 0)))
            return pack_refuse(refusal, OMNI_ERR_INVALID, "omni_jpegdec: file %d holds a picture of %dx%d, the handle decodes %dx%d", i, D.w, D.h, c.w, c.h);
        if (st == OMNI_JPEGDEC_OK && (sizes[i] > c.capacity || D.n_yblocks > room.nyb_max)) D.status = OMNI_JPEGDEC_HOST;
    }
    return OMNI_OK;
}

// ---- one picture: classify and plan, then place, then write ----------------------------------------------------------------------------------------------------
// what plan_picture found out about a picture beyond its descriptor
struct PackPicture {
    bool decoded = false;                                   // its scan is the kernels' to decode (Desc::mode DECODE or SPREAD)
    bool planned = false;                                   // ... as a restart file: `plan` holds its tables
    int64_t raw_end = 0, n_clean = 0;                       // the scan: survey()'s end of the raw bytes (the raw layout), the clean bytes
    std::vector<uint32_t> tiles;                            // the raw layout: survey()'s table
    ChunkPlan plan;
};

// Classifies one parsed picture against the handle and plans it: D's status, mode, subsequences, intervals and chunks (not its offsets).  A file whose only
// obstacle is its restart interval is promoted when the handle can plan it (too few markers: CORRUPT; no plan, or tables above the handle's room: it stays
// HOST); an OK file is one chunk, or plain_chunks' chunks (SPREAD).  The clean bytes of a scan are needed for either: clean_dst != null unstuffs them there at
// once (the clean layout: the place of a picture's scan is known before its size), null surveys the scan instead (the raw layout).  rst: scratch
inline void plan_picture(const PackConfig& c, const PackRoom& room, const uint8_t* file, int64_t size, Desc& D, uint8_t* clean_dst, PackPicture* p,
                         std::vector<int64_t>* rst) {
    p->decoded = p->planned = false;
    auto clean_scan = [&](int64_t* rst_out, int64_t max_rst, int64_t* n_rst) -> int64_t {
        if (clean_dst) return p->n_clean = unstuff(file + D.scan_off, D.scan_bytes, clean_dst, rst_out, max_rst, n_rst);
        p->tiles.resize((size_t)(D.scan_bytes / JD_UNSTUFF_TILE + 1));
        const Survey v = survey(file + D.scan_off, D.scan_bytes, p->tiles.data(), (int64_t)p->tiles.size(), rst_out, max_rst);
        if (n_rst) *n_rst = v.n_rst;
        p->tiles.resize((size_t)v.n_tiles);
        p->raw_end = v.raw_end;
        return p->n_clean = v.n_clean;
    };
    const size_t W = (size_t)c.restart_wgs;
    // (intervals: every one costs a subsequence and 16 bytes of table -- a file that cannot be planned for that alone is not unstuffed twice)
    const size_t n_int = D.restart_only ? ((size_t)D.mcus_x * D.mcus_y + D.restart - 1) / D.restart : 0;
    if (W && D.status == OMNI_JPEGDEC_HOST && D.restart_only && size <= c.capacity && D.n_yblocks <= room.nyb_max && n_int <= W * JD_MAX_SUBSEQ &&
        (n_int + 1) * sizeof(Interval) + (W + 1) * sizeof(uint32_t) <= room.tab_bytes) {
        rst->resize((size_t)(D.scan_bytes / 2 + 1));
        int64_t n_rst = 0;
        const int64_t n = clean_scan(rst->data(), (int64_t)rst->size(), &n_rst);
        plan_chunks(D, n, rst->data(), n_rst, (uint32_t)c.subseq_bits, (uint32_t)W, JD_MAX_SUBSEQ, &p->plan);
        if (p->plan.status == OMNI_JPEGDEC_CORRUPT) {
            D.status = OMNI_JPEGDEC_CORRUPT;
        } else if (p->plan.status == OMNI_JPEGDEC_OK && p->plan.table_bytes() <= room.tab_bytes) {
            p->decoded = p->planned = true;
            D.status = OMNI_JPEGDEC_OK;
            D.mode = JD_MODE_DECODE;
            D.total_bits = (uint32_t)(n * 8);
            D.subseq_bits = p->plan.subseq_bits;
            D.n_sub = p->plan.n_sub;
            D.n_int = p->plan.n_int;
            D.n_chunks = p->plan.n_chunks;
            return;
        }
    }
    if (D.status == OMNI_JPEGDEC_OK) {
        const int64_t n = clean_scan(nullptr, 0, nullptr);
        const bool spread = c.plain_wgs >= 2;
        p->decoded = true;
        D.mode = JD_MODE_DECODE;
        D.total_bits = (uint32_t)(n * 8);
        D.subseq_bits = spread ? plain_subseq_bits(D.total_bits, (uint32_t)c.subseq_bits, (uint32_t)c.plain_wgs, JD_MAX_SUBSEQ)
                               : subseq_bits_for(D.total_bits, (uint32_t)c.subseq_bits, JD_MAX_SUBSEQ);
        D.n_sub = (D.total_bits + D.subseq_bits - 1) / D.subseq_bits;
        const uint32_t C = spread ? plain_chunks(D.n_sub, (uint32_t)c.plain_wgs) : 1u;
        if (C >= 2 && D.n_sub <= room.state_cap) {                                          // the spread path; one chunk is the entropy kernel's, as ever
            D.mode = JD_MODE_SPREAD;
            D.spread_chunks = C;
        }
    } else if (D.status != OMNI_JPEGDEC_HOST) {
        D.mode = JD_MODE_ZERO;
    }
}

// A picture the host decodes (status HOST behind plan_picture), placed and written in one: its pixels at *at, which moves behind them.  A scan that turns out
// CORRUPT leaves the zeros to the kernels and takes no room
inline void host_picture(const PackConfig& c, const uint8_t* file, Desc& D, uint8_t* block, size_t* at) {
    D.dev_off = (int64_t)*at;
    D.status = decode_sequential(file, D, block + *at, c.w);
    D.mode = D.status == OMNI_JPEGDEC_CORRUPT ? JD_MODE_ZERO : JD_MODE_PIXELS;
    if (D.mode == JD_MODE_PIXELS) *at += pack_align16((size_t)c.w * c.h);
}

// a picture's share of the maxima the grids are sized by, once its mode is final
inline void pack_tally(const Desc& D, PackResult* r) {
    if (D.mode == JD_MODE_DECODE) { r->unspread = true; r->max_chunks = std::max(r->max_chunks, (int)D.n_chunks); }
    if (D.mode == JD_MODE_SPREAD) { r->spread_chunks = std::max(r->spread_chunks, (int)D.spread_chunks); r->spread_sub = std::max(r->spread_sub, D.n_sub); }
}

// ---- the clean layout ----------------------------------------------------------------------------------------------------------------------------------------------
// a decoded picture whose clean scan plan_picture has unstuffed at *at (its Desc::dev_off): the tables of a planned restart file go behind the scan
inline void place_clean(const PackPicture& p, Desc& D, size_t* at) {
    const size_t scan_bytes = pack_align16((size_t)p.n_clean + JD_SCAN_PAD);
    if (p.planned) D.tab_off = (int64_t)(*at + scan_bytes);
    *at += scan_bytes + (p.planned ? pack_align16(p.plan.table_bytes()) : 0);
}

inline int fill_clean(const PackConfig& c, const PackRoom& room, PackBatch& b, const uint8_t* const* files, uint8_t* block, PackResult* R, PackRefusal* refusal) {
    size_t at = pack_align16(b.descs.size() * sizeof(Desc));
    PackPicture p;
    std::vector<int64_t> rst;
    for (size_t i = 0; i < b.descs.size(); ++i) {
        Desc& D = b.descs[i];
        plan_picture(c, room, files[i], b.sizes[i], D, block + at, &p, &rst);
        D.dev_off = (int64_t)at;
        if (p.decoded) {
            place_clean(p, D, &at);
            if (p.planned) p.plan.store(block + D.tab_off);
        } else if (D.status == OMNI_JPEGDEC_HOST) {
            host_picture(c, files[i], D, block, &at);
        }
        pack_tally(D, R);
    }
    R->upload_bytes = at;
    return at <= room.in_bytes ? OMNI_OK : pack_refuse(refusal, OMNI_ERR_CAPACITY, "omni_jpegdec: %zu bytes to upload, the handle holds %zu", at, room.in_bytes);
}

// ---- the raw layout ------------------------------------------------------------------------------------------------------------------------------------------------
// where the next job, tile table, interval table, raw scan and clean area go -- or, counted from zero, the bytes of each that a batch needs
struct RawCursor { size_t job = 0, tiles = 0, tabs = 0, raw = 0, clean = 0; };

// the cursor behind a decoded picture's regions
inline void raw_advance(const PackPicture& p, RawCursor* at) {
    at->job += sizeof(UnstuffJob);
    at->tiles += p.tiles.size() * sizeof(uint32_t);
    at->tabs += p.planned ? pack_align16(p.plan.table_bytes()) : 0;
    at->raw += pack_align16((size_t)p.raw_end); at->clean += pack_align16((size_t)p.n_clean + JD_SCAN_PAD);
}
// a decoded picture's regions at the cursor, which moves behind them, and the job that tells jpegdec_unstuff_kernel about them
inline UnstuffJob place_raw(const PackPicture& p, Desc& D, RawCursor* at) {
    const UnstuffJob J{(int64_t)at->raw, p.raw_end, (int64_t)at->clean, p.n_clean, (int64_t)at->tiles};
    D.dev_off = J.clean_off;
    if (p.planned) D.tab_off = (int64_t)at->tabs;
    raw_advance(p, at);
    return J;
}
// ... written: the job, the tile table, the tables of a planned restart file, the scan as it stands in the file, zero-padded to a multiple of 16
inline void write_raw(const PackPicture& p, const Desc& D, const UnstuffJob& J, size_t job_at, const uint8_t* file, uint8_t* block) {
    memcpy(block + job_at, &J, sizeof(J));
    memcpy(block + J.tile_off, p.tiles.data(), p.tiles.size() * sizeof(uint32_t));
    if (p.planned) p.plan.store(block + D.tab_off);
    if (J.raw_bytes) memcpy(block + J.raw_off, file + D.scan_off, (size_t)J.raw_bytes);
    memset(block + J.raw_off + J.raw_bytes, 0, pack_align16((size_t)J.raw_bytes) - (size_t)J.raw_bytes);
}

inline int fill_raw(const PackConfig& c, const PackRoom& room, PackBatch& b, const uint8_t* const* files, uint8_t* block, PackResult* R, PackRefusal* refusal) {
    const size_t n = b.descs.size();
    std::vector<PackPicture> pics(n);
    std::vector<int64_t> rst;
    RawCursor size;                                                                         // (raw_advance from zero: the sizes are the placement's own)
    size_t n_host = 0;
    for (size_t i = 0; i < n; ++i) {
        plan_picture(c, room, files[i], b.sizes[i], b.descs[i], nullptr, &pics[i], &rst);
        if (pics[i].decoded) raw_advance(pics[i], &size);
        n_host += b.descs[i].status == OMNI_JPEGDEC_HOST;
    }
    // everything but the host-decoded pixels has its size by now, and the handle was made for the largest of each
    RawCursor at;
    at.job = R->jobs_off = pack_align16(n * sizeof(Desc));
    at.tiles = at.job + pack_align16(size.job);
    at.tabs = at.tiles + pack_align16(size.tiles);
    size_t px_at = at.tabs + size.tabs;
    const size_t need = px_at + n_host * pack_align16((size_t)c.w * c.h) + size.raw + size.clean;
    if (need > room.in_bytes) return pack_refuse(refusal, OMNI_ERR_CAPACITY, "omni_jpegdec: a block of %zu bytes, the handle holds %zu", need, room.in_bytes);
    memset(block + at.tabs, 0, size.tabs);                                                  // (the padding between the tables is uploaded with them)
    for (size_t i = 0; i < n; ++i) {
        b.descs[i].dev_off = (int64_t)at.job;                                               // (a picture of zeros: no region of its own)
        if (b.descs[i].status == OMNI_JPEGDEC_HOST) host_picture(c, files[i], b.descs[i], block, &px_at);
        pack_tally(b.descs[i], R);
    }
    at.raw = px_at;
    at.clean = R->upload_bytes = px_at + size.raw;
    for (size_t i = 0; i < n; ++i) {
        if (!pics[i].decoded) continue;
        const size_t job_at = at.job;
        const UnstuffJob J = place_raw(pics[i], b.descs[i], &at);
        write_raw(pics[i], b.descs[i], J, job_at, files[i], block);
        ++R->n_jobs; R->raw_bytes += J.raw_bytes; R->clean_bytes += J.clean_bytes;
        R->job_tiles = std::max(R->job_tiles, (int64_t)pics[i].tiles.size());
    }
    R->clean_end = at.clean;
    return OMNI_OK;
}

// Plans every picture of a parsed batch and writes the block (room.in_bytes), the descriptors at its start.  Returns OMNI_OK with *result, or the refusal's code
// with *result as it was
inline int pack_fill(const PackConfig& c, const PackRoom& room, PackBatch& batch, const uint8_t* const* files, uint8_t* block, PackResult* result,
                     PackRefusal* refusal) {
    PackResult R;
    R.unspread = c.plain_wgs < 2;
    const int rc = c.unstuff_dev ? fill_raw(c, room, batch, files, block, &R, refusal) : fill_clean(c, room, batch, files, block, &R, refusal);
    if (rc) return rc;
    memcpy(block, batch.descs.data(), batch.descs.size() * sizeof(Desc));
    *result = R;
    return OMNI_OK;
}

}  // namespace jd
}  // namespace omni
