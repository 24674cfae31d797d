// jpegdec_unstuff_pin: the unstuffing by tiles of csrc/jpeg_dec_plan.h -- unstuff_keep, survey, unstuff_tiled_host -- and the memchr scan_end against the
// byte-wise pass (unstuff) and the byte-wise rules written out below, built with g++ alone, with -fsanitize=address,undefined (tests/test_jpegdec_unstuff_cpu.py,
// tests/jpegdec_unstuff_cases.py).  Every buffer has exactly the size the functions are promised, on the heap, so a byte too many is the sanitizer's to report.
//   jpegdec_unstuff_pin <in> <out>
// in:  int32 n; per case int32 size + the bytes
// out: per case int64 {clean bytes, raw_end, restart markers, tiles, scan_end from 0}
// Before the cases, patterns of its own: every string of up to 6 bytes over {FF, 00, D3, D9, 41} alone, and every one of up to 4 bytes laid across the first tile
// seam and across a 16-byte seam of a longer string.  Exit code 5: the tiles differ from unstuff; 6: survey differs; 7: scan_end differs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_dec_plan.h"

using namespace omni::jd;

static int64_t scan_end_bytewise(const uint8_t* f, int64_t size, int64_t p) {
    while (p < size) {
        if (f[p] != 0xff) { ++p; continue; }
        int64_t q = p + 1;
        while (q < size && f[q] == 0xff) ++q;
        if (q >= size) return size;
        if (f[q] == 0 || (f[q] >= 0xd0 && f[q] <= 0xd7)) { p = q + 1; continue; }
        return p;
    }
    return size;
}
// where unstuff stops: the start of the 0xFF run that ends in a marker other than RSTn or runs off the end; n when there is none
static int64_t raw_end_bytewise(const uint8_t* s, int64_t n) {
    int64_t i = 0;
    while (i < n) {
        if (s[i] != 0xff) { ++i; continue; }
        const int64_t j = i;
        while (i < n && s[i] == 0xff) ++i;
        if (i >= n) return j;
        if (s[i] == 0 || (s[i] >= 0xd0 && s[i] <= 0xd7)) { ++i; continue; }
        return j;
    }
    return n;
}

struct Result { int64_t n_clean, raw_end, n_rst, n_tiles, scan_end; };

// 0, or the exit code
static int check(const std::vector<uint8_t>& str, Result* r) {
    const int64_t n = (int64_t)str.size();
    uint8_t* s = (uint8_t*)malloc((size_t)n ? (size_t)n : 1);                               // (exactly n bytes: a read behind them is reported)
    if (n) memcpy(s, str.data(), (size_t)n);
    const int64_t max_rst = n / 2 + 1, max_tiles = n / JD_UNSTUFF_TILE + 1;
    std::vector<uint8_t> a((size_t)n + JD_SCAN_PAD, 0x5A), b((size_t)n + JD_SCAN_PAD, 0xA5);
    std::vector<int64_t> rst_a((size_t)max_rst, -1), rst_b((size_t)max_rst, -1);
    std::vector<uint32_t> tiles((size_t)max_tiles, 0xffffffffu);
    int64_t n_rst = 0;
    const int64_t n_clean = unstuff(s, n, a.data(), rst_a.data(), max_rst, &n_rst);
    const Survey v = survey(s, n, tiles.data(), max_tiles, rst_b.data(), max_rst);
    int rc = 0;
    if (v.n_clean != n_clean || v.n_rst != n_rst || v.raw_end != raw_end_bytewise(s, n) || v.n_tiles != ((v.raw_end > 1 ? v.raw_end : 1) + JD_UNSTUFF_TILE - 1) / JD_UNSTUFF_TILE ||
        v.n_tiles > max_tiles || rst_a != rst_b || tiles[0] != 0)
        rc = 6;
    for (int64_t t = 1; !rc && t < v.n_tiles; ++t)
        if (tiles[(size_t)t] < tiles[(size_t)t - 1] || tiles[(size_t)t] > n_clean) rc = 6;
    // a capped restart list and no list at all: the same counts, the same first entries
    if (!rc && n_rst > 1) {
        std::vector<int64_t> few((size_t)n_rst - 1, -1);
        const Survey c = survey(s, n, tiles.data(), max_tiles, few.data(), n_rst - 1);
        if (c.n_rst != n_rst - 1 || memcmp(few.data(), rst_a.data(), few.size() * sizeof(int64_t)) || c.n_clean != n_clean) rc = 6;
    }
    if (!rc && survey(s, n, tiles.data(), max_tiles, nullptr, 0).n_rst != 0) rc = 6;
    if (!rc) {
        const int64_t end = unstuff_tiled_host(s, v, tiles.data(), b.data());
        if (end != n_clean || memcmp(a.data(), b.data(), (size_t)n_clean + JD_SCAN_PAD)) rc = 5;
        for (size_t i = (size_t)n_clean + JD_SCAN_PAD; !rc && i < b.size(); ++i)
            if (b[i] != 0xA5) rc = 5;                                                      // nothing behind the padding is written
    }
    const int64_t se = scan_end(s, n, 0);
    if (!rc && se != scan_end_bytewise(s, n, 0)) rc = 7;
    for (int64_t p = 1; !rc && p <= n; p = p == 8 && n - 8 > 9 ? n - 8 : p + 1)            // from the first and from the last 8 positions
        if (scan_end(s, n, p) != scan_end_bytewise(s, n, p)) rc = 7;
    if (r) *r = Result{n_clean, v.raw_end, n_rst, v.n_tiles, se};
    free(s);
    return rc;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    static const uint8_t alphabet[5] = {0xff, 0x00, 0xd3, 0xd9, 0x41};
    for (int len = 0; len <= 6; ++len) {
        int total = 1;
        for (int k = 0; k < len; ++k) total *= 5;
        for (int code = 0; code < total; ++code) {
            std::vector<uint8_t> w((size_t)len);
            for (int k = 0, c = code; k < len; ++k, c /= 5) w[(size_t)k] = alphabet[c % 5];
            if (int rc = check(w, nullptr)) { fprintf(stderr, "pattern of %d bytes, code %d\n", len, code); return rc; }
            if (len < 1 || len > 4) continue;
            for (int64_t seam : {(int64_t)JD_UNSTUFF_TILE, (int64_t)JD_UNSTUFF_TILE + 16})      // the pattern's byte k at seam - len + shift + k: every split, and flush on either side
                for (int shift = 0; shift <= len; ++shift) {
                    if (seam != JD_UNSTUFF_TILE && code % 7) continue;                      // (the lane seam means nothing to these functions: a seventh of the patterns)
                    std::vector<uint8_t> str((size_t)seam + 9);
                    for (size_t i = 0; i < str.size(); ++i) str[i] = (uint8_t)(0x20 + i % 0x50);
                    memcpy(str.data() + seam - len + shift, w.data(), (size_t)len);
                    if (int rc = check(str, nullptr)) { fprintf(stderr, "pattern of %d bytes, code %d, at %lld\n", len, code, (long long)(seam - len + shift)); return rc; }
                    str.resize((size_t)(seam - len + shift) + (size_t)len);                // ... and as the string's last bytes
                    if (int rc = check(str, nullptr)) { fprintf(stderr, "pattern of %d bytes, code %d, ends the string at %zu\n", len, code, str.size()); return rc; }
                }
        }
    }
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 3;
    for (int i = 0; i < n; ++i) {
        int32_t size = 0;
        if (fread(&size, 4, 1, in) != 1 || size < 0) return 3;
        std::vector<uint8_t> str((size_t)size);
        if (size && fread(str.data(), 1, str.size(), in) != str.size()) return 3;
        Result r;
        if (int rc = check(str, &r)) { fprintf(stderr, "case %d of %d bytes\n", i, size); return rc; }
        fwrite(&r, sizeof(r), 1, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
