// jpegdec_pack_pin: csrc/jpeg_dec_pack.h -- pack_room, pack_parse, pack_fill, what a decoder handle does with a batch of files on the host -- built with g++ alone,
// with -fsanitize=address,undefined (tests/test_jpegdec_pack_cpu.py).  The block is a heap buffer of exactly pack_room's in_bytes: a byte written outside it is the
// sanitizer's report.
//   jpegdec_pack_pin <in> <out>
// in:  int32 n; per batch int32 {w, h, capacity, S, files, host_idx, dev_idx} + per file int32 size + the file.  host_idx / dev_idx (-1: none): a file that must
//      come out as host-decoded pixels / as a scan for the kernels, whatever the switches
// out: per batch and per combination of restart_wgs {0, 3} x plain_wgs {0, 3} x unstuff_dev {0, 1} (in that order, unstuff_dev fastest):
//      int32 {refusal code, upload_bytes, clean_end, in_bytes, jobs} + per file int32 {status, mode, n_sub, subseq_bits, n_int, n_chunks, spread_chunks}
//      (all zero when the batch was refused)
// Checked here, for every batch that is not refused, with an exit code each:
//   11  a region the descriptors and jobs name is out of bounds or misaligned: every one inside [0, in_bytes), uploaded ones inside [0, upload_bytes), the clean
//       areas of device-unstuffed scans inside [upload_bytes, clean_end], clean_end <= in_bytes; raw_off % 16, clean_off % 4, tile_off % 4, tab_off % 4
//   12  two regions overlap
//   13  a scan's bytes: switch off, dev_off holds unstuff()'s bytes + JD_SCAN_PAD zeros; switch on, raw_off holds the file's scan [0, raw_end) zero-padded to 16,
//       the tile table is survey()'s, clean_bytes unstuff()'s count -- and unstuff_tiled_host (the stand-in for jpegdec_unstuff_kernel), run on the block's own
//       job, leaves unstuff()'s bytes in the clean area
//   14  tab_off does not hold ChunkPlan::store's bytes
//   15  a PIXELS picture does not hold decode_sequential's pixels
//   16  mode, status, n_sub, subseq_bits, n_int, n_chunks, spread_chunks of a descriptor are not what decode_planned_host reports for the file under the same
//       switches (the stand-in knows no capacity: a file above it must be host-decoded)
//   17  PackResult's maxima and sums are not those of the descriptors and jobs
//   18  host_idx / dev_idx came out otherwise
//   19  pack_fill refused a batch pack_parse took
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_dec_pack.h"

using namespace omni::jd;

struct Region { int64_t lo, hi; };

static int check(const PackConfig& cfg, const PackRoom& room, const PackResult& R, const std::vector<std::vector<uint8_t>>& files, const uint8_t* block, int host_idx,
                 int dev_idx) {
    const size_t n = files.size();
    const Desc* descs = reinterpret_cast<const Desc*>(block);
    const int64_t upload = (int64_t)R.upload_bytes, in_bytes = (int64_t)room.in_bytes, px = (int64_t)cfg.w * cfg.h;
    const int64_t clean_lo = cfg.unstuff_dev ? upload : 0, clean_hi = cfg.unstuff_dev ? (int64_t)R.clean_end : upload;
    if (upload > in_bytes || (cfg.unstuff_dev && (R.clean_end < R.upload_bytes || R.clean_end > room.in_bytes))) return 11;
    std::vector<Region> regions{{0, (int64_t)(n * sizeof(Desc))}};
    auto add = [&](int64_t lo, int64_t bytes, int64_t align, int64_t from, int64_t to) {
        if (lo < from || bytes < 0 || lo + bytes > to || to > in_bytes || lo % align) return 11;
        regions.push_back(Region{lo, lo + bytes});
        return 0;
    };
    PackResult want;                                                                        // (its job totals alone)
    const UnstuffJob* jobs = reinterpret_cast<const UnstuffJob*>(block + R.jobs_off);
    size_t job = 0;
    if (cfg.unstuff_dev && add((int64_t)R.jobs_off, (int64_t)(R.n_jobs * sizeof(UnstuffJob)), 16, 0, upload)) return 11;
    for (size_t i = 0; i < n; ++i) {
        const Desc& D = descs[i];
        const std::vector<uint8_t>& f = files[i];
        // what the stand-in says of the file (plain_wgs 0 and 1 are both one chunk; 1, so that a file a handle decodes on the host reports no statistics)
        std::vector<uint8_t> pix((size_t)px, 0xA5);
        PlannedStats ps;
        int w = 0, h = 0;
        int st = decode_planned_host(f.data(), (int64_t)f.size(), (uint32_t)cfg.subseq_bits, (uint32_t)cfg.restart_wgs, (uint32_t)(cfg.plain_wgs ? cfg.plain_wgs : 1),
                                     JD_MAX_SUBSEQ, pix.data(), cfg.w, cfg.w, cfg.h, &w, &h, &ps);
        Desc P;
        const int cls = parse(f.data(), (int64_t)f.size(), &P);
        bool decoded = ps.subseq_bits != 0;
        if ((cls == OMNI_JPEGDEC_OK || cls == OMNI_JPEGDEC_HOST) && (int64_t)f.size() > cfg.capacity) {      // above the capacity: the sequential decoder
            decoded = false;
            P.status = OMNI_JPEGDEC_HOST;
            st = decode_sequential(f.data(), P, pix.data(), cfg.w);
        }
        if ((int)i == host_idx && !(D.mode == JD_MODE_PIXELS && D.status == OMNI_JPEGDEC_HOST)) return 18;
        if ((int)i == dev_idx && !(D.mode == JD_MODE_DECODE || D.mode == JD_MODE_SPREAD)) return 18;
        if (decoded) {
            const bool spread = !P.restart && ps.n_chunks >= 2;
            const uint32_t n_int = P.restart ? ((uint32_t)P.mcus_x * P.mcus_y + P.restart - 1) / P.restart : 0u;
            if (D.status != OMNI_JPEGDEC_OK || D.mode != (spread ? JD_MODE_SPREAD : JD_MODE_DECODE) || D.n_sub != ps.n_sub || D.subseq_bits != ps.subseq_bits ||
                D.n_int != n_int || D.n_chunks != (P.restart ? ps.n_chunks : 0u) || D.spread_chunks != (spread ? ps.n_chunks : 0u))
                return 16;
            // the scan
            std::vector<uint8_t> clean((size_t)P.scan_bytes + JD_SCAN_PAD);
            std::vector<int64_t> rst((size_t)(P.scan_bytes / 2 + 1));
            int64_t n_rst = 0;
            const uint8_t* scan = f.data() + P.scan_off;
            const int64_t n_clean = unstuff(scan, P.scan_bytes, clean.data(), rst.data(), (int64_t)rst.size(), &n_rst);
            if (D.total_bits != (uint32_t)(n_clean * 8)) return 13;
            if (add(D.dev_off, n_clean + JD_SCAN_PAD, 4, clean_lo, clean_hi)) return 11;
            if (!cfg.unstuff_dev) {
                if (memcmp(block + D.dev_off, clean.data(), (size_t)n_clean + JD_SCAN_PAD)) return 13;
            } else {
                if (job >= (size_t)R.n_jobs) return 17;
                const UnstuffJob& J = jobs[job++];
                std::vector<uint32_t> tiles((size_t)(P.scan_bytes / JD_UNSTUFF_TILE + 1));
                const Survey v = survey(scan, P.scan_bytes, tiles.data(), (int64_t)tiles.size(), nullptr, 0);
                const int64_t raw_room = (v.raw_end + 15) & ~(int64_t)15;
                if (J.clean_off != D.dev_off || J.raw_bytes != v.raw_end || J.clean_bytes != n_clean || v.n_clean != n_clean) return 13;
                if (add(J.raw_off, raw_room, 16, 0, upload) || add(J.tile_off, v.n_tiles * 4, 4, 0, upload)) return 11;
                if (memcmp(block + J.raw_off, scan, (size_t)v.raw_end) || memcmp(block + J.tile_off, tiles.data(), (size_t)v.n_tiles * 4)) return 13;
                for (int64_t k = v.raw_end; k < raw_room; ++k)
                    if (block[J.raw_off + k]) return 13;
                // what the kernel will make of the job: the block's own raw bytes and tile table into a copy of the clean area
                std::vector<uint8_t> area((size_t)n_clean + JD_SCAN_PAD, 0xA5);
                Survey s;
                s.raw_end = J.raw_bytes; s.n_clean = J.clean_bytes; s.n_tiles = v.n_tiles;
                if (unstuff_tiled_host(block + J.raw_off, s, reinterpret_cast<const uint32_t*>(block + J.tile_off), area.data()) != n_clean ||
                    memcmp(area.data(), clean.data(), area.size()))
                    return 13;
                if (v.n_tiles > want.job_tiles) want.job_tiles = v.n_tiles;
                want.raw_bytes += v.raw_end;
                want.clean_bytes += n_clean;
            }
            if (P.restart) {                                                                // the tables
                ChunkPlan plan;
                plan_chunks(P, n_clean, rst.data(), n_rst, (uint32_t)cfg.subseq_bits, (uint32_t)cfg.restart_wgs, JD_MAX_SUBSEQ, &plan);
                if (plan.status != OMNI_JPEGDEC_OK) return 14;
                std::vector<uint8_t> tab(plan.table_bytes());
                plan.store(tab.data());
                if (add(D.tab_off, (int64_t)tab.size(), 4, 0, upload)) return 11;
                if (memcmp(block + D.tab_off, tab.data(), tab.size())) return 14;
            }
        } else if (st == OMNI_JPEGDEC_HOST) {
            if (D.status != OMNI_JPEGDEC_HOST || D.mode != JD_MODE_PIXELS || D.n_sub || D.subseq_bits || D.n_int || D.n_chunks || D.spread_chunks) return 16;
            if (add(D.dev_off, px, 16, 0, upload)) return 11;
            if (memcmp(block + D.dev_off, pix.data(), (size_t)px)) return 15;
        } else {
            if (D.status != OMNI_JPEGDEC_CORRUPT || D.mode != JD_MODE_ZERO || D.n_sub || D.subseq_bits || D.n_int || D.n_chunks || D.spread_chunks) return 16;
        }
    }
    std::sort(regions.begin(), regions.end(), [](const Region& a, const Region& b) { return a.lo < b.lo; });
    for (size_t k = 1; k < regions.size(); ++k)
        if (regions[k].lo < regions[k - 1].hi) return 12;
    // the totals, recomputed from the descriptors
    int max_chunks = 1, spread_chunks = 0;
    uint32_t spread_sub = 0;
    bool unspread = cfg.plain_wgs < 2;
    for (size_t i = 0; i < n; ++i) {
        const Desc& D = descs[i];
        if (D.mode == JD_MODE_DECODE) { unspread = true; max_chunks = std::max(max_chunks, (int)D.n_chunks); }
        if (D.mode == JD_MODE_SPREAD) { spread_chunks = std::max(spread_chunks, (int)D.spread_chunks); spread_sub = std::max(spread_sub, D.n_sub); }
    }
    if (R.max_chunks != max_chunks || R.spread_chunks != spread_chunks || R.spread_sub != spread_sub || R.unspread != unspread) return 17;
    if ((size_t)R.n_jobs != job || R.job_tiles != want.job_tiles || R.raw_bytes != want.raw_bytes || R.clean_bytes != want.clean_bytes) return 17;
    if (!cfg.unstuff_dev && (R.jobs_off || R.n_jobs || R.clean_end)) return 17;
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 3;
    for (int b = 0; b < n; ++b) {
        int32_t a[7];
        if (fread(a, 4, 7, in) != 7 || a[4] < 1) return 3;
        std::vector<std::vector<uint8_t>> files((size_t)a[4]);
        std::vector<const uint8_t*> ptrs;
        std::vector<int64_t> sizes;
        for (auto& f : files) {
            int32_t size = 0;
            if (fread(&size, 4, 1, in) != 1 || size < 0) return 3;
            f.resize((size_t)size + 1);                                                     // (never empty: a null file is a refusal of its own)
            if (size && fread(f.data(), 1, (size_t)size, in) != (size_t)size) return 3;
            f.resize((size_t)size);
            ptrs.push_back(f.data());
            sizes.push_back(size);
        }
        for (int combo = 0; combo < 8; ++combo) {
            PackConfig cfg;
            cfg.w = a[0]; cfg.h = a[1]; cfg.capacity = a[2]; cfg.subseq_bits = a[3]; cfg.max_images = a[4];
            cfg.restart_wgs = combo & 4 ? 3 : 0; cfg.plain_wgs = combo & 2 ? 3 : 0; cfg.unstuff_dev = combo & 1;
            const PackRoom room = pack_room(cfg);
            uint8_t* block = static_cast<uint8_t*>(malloc(room.in_bytes));                  // exactly the handle's block: the sanitizer guards its end
            if (!block) return 4;
            memset(block, 0xA5, room.in_bytes);
            PackBatch batch;
            PackRefusal no;
            PackResult R;
            std::vector<int32_t> rec(5 + 7 * files.size(), 0);
            rec[3] = (int32_t)room.in_bytes;
            if (pack_parse(cfg, room, ptrs.data(), sizes.data(), (int)files.size(), &batch, &no)) {
                rec[0] = no.code;
                if (no.message.empty()) return 19;
            } else {
                if (pack_fill(cfg, room, batch, ptrs.data(), block, &R, &no)) return 19;
                const int rc = check(cfg, room, R, files, block, a[5], a[6]);
                if (rc) { fprintf(stderr, "batch %d combination %d: check %d\n", b, combo, rc); return rc; }
                rec[1] = (int32_t)R.upload_bytes; rec[2] = (int32_t)R.clean_end; rec[4] = R.n_jobs;
                const Desc* descs = reinterpret_cast<const Desc*>(block);
                for (size_t i = 0; i < files.size(); ++i) {
                    const Desc& D = descs[i];
                    const int32_t r[7] = {D.status, D.mode, (int32_t)D.n_sub, (int32_t)D.subseq_bits, (int32_t)D.n_int, (int32_t)D.n_chunks, (int32_t)D.spread_chunks};
                    std::copy(r, r + 7, rec.begin() + 5 + 7 * (long)i);
                }
            }
            free(block);
            if (fwrite(rec.data(), 4, rec.size(), out) != rec.size()) return 4;
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
