// The tile walk of the persistent convolution kernels and of MobileNetVLAD's block kernel with a rectangle of tiles left out (ConvArgs::skip_*,
// VladSBlockArgs::sk_*: the constant region of the fisheye mask, whose results the caller already holds).  A workgroup walks the numbers
// t = its id, + the grid, ... and splits t into (image, r) itself; r, a tile's number among the tiles of one image that RUN, counts
//   the tile rows above the rectangle (n_above tiles), the tiles left and right of it in its own rows (bw per row, up to n_upto), the tile rows below.
// No rectangle: n_above = n_upto = act = tiles_x * tiles_y.  Divisions are multiply-highs with ceil(2^32 / d), exact while r * d < 2^32 (the plan
// checks it for every r of the grid).  Host and device code: tests/cpp/tile_walk_pin.cpp runs it under plain g++.
#pragma once
#include <cstdint>
#include "../../include/omni_hip.h"

#if defined(__HIPCC__)
#define TW_HD __host__ __device__ __forceinline__
#else
#define TW_HD inline
#endif

namespace omni {

void set_error(const char* fmt, ...);

TW_HD uint32_t umulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}
// n / d with m = tile_walk_magic(d)
TW_HD int tile_walk_div(int n, uint32_t m) { return m ? (int)umulhi32((uint32_t)n, m) : n; }
inline uint32_t tile_walk_magic(int d) { return d > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)d - 1) / (uint64_t)d) : 0u; }   // 0 = divisor 1 (2^32 does not fit)

struct TileWalk {
    int act, n_above, n_upto;         // tiles of an image that run, ... above the rectangle, ... down to its last row
    int y0, y1, x0, w;                // the rectangle: tile rows [y0, y1) x tile columns [x0, x0 + w); none: all 0
    int bw;                           // tile columns beside it
    uint32_t magic_tx, magic_bw;      // tile_walk_magic(tiles_x), tile_walk_magic(bw)
    int xcd;                          // OMNI_CONV_XCD: xcd_block_id() (set by the launcher)
};

// the walk of a tiles_x x tiles_y grid without the rectangle [ty0, ty1) x [tx0, tx1) (empty: every tile runs); `who` names the launcher in the error
inline int tile_walk_plan(TileWalk& k, const char* who, int tiles_x, int tiles_y, int ty0, int ty1, int tx0, int tx1) {
    const bool skip = ty1 > ty0 && tx1 > tx0;
    if (skip && !(ty0 >= 0 && ty1 <= tiles_y && tx0 >= 0 && tx1 <= tiles_x)) {
        set_error("%s: skip rectangle outside the tile grid", who);
        return OMNI_ERR_INVALID;
    }
    k.y0 = skip ? ty0 : 0; k.y1 = skip ? ty1 : 0; k.x0 = skip ? tx0 : 0; k.w = skip ? tx1 - tx0 : 0;
    k.bw = tiles_x - k.w;
    k.act = tiles_x * tiles_y - (k.y1 - k.y0) * k.w;
    k.n_above = skip ? k.y0 * tiles_x : k.act;
    k.n_upto = k.n_above + (k.y1 - k.y0) * k.bw;
    if (k.act <= 0) {
        set_error("%s: the skip rectangle covers the whole image", who);
        return OMNI_ERR_INVALID;
    }
    if ((int64_t)tiles_x * tiles_y * tiles_x >= (1ll << 32)) {
        set_error("%s: %d x %d tiles: too many for the multiply-high division", who, tiles_x, tiles_y);
        return OMNI_ERR_INVALID;
    }
    k.magic_tx = tile_walk_magic(tiles_x); k.magic_bw = tile_walk_magic(k.bw);
    k.xcd = 0;
    return OMNI_OK;
}

// r -> (tile row, tile column).  MULHI = false divides by tiles_x and bw in hardware instead: the register-stationary cin = 128 kernels, which sit at
// the register limit (the two reciprocals are two more SGPRs there, and v4 spills)
template <bool MULHI = true>
TW_HD void tile_walk_rc(const TileWalk& k, int tiles_x, int r, int& ty, int& tx) {
    if (r < k.n_above || r >= k.n_upto) {                 // full tile rows above / below the rectangle
        int base = 0;
        if (r >= k.n_upto) { r -= k.n_upto; base = k.y1; }
        const int ry = MULHI ? tile_walk_div(r, k.magic_tx) : r / tiles_x;
        tx = r - ry * tiles_x; ty = ry + base;
    } else {                                              // its rows: the tiles left and right of it
        r -= k.n_above;
        const int q = MULHI ? tile_walk_div(r, k.magic_bw) : r / k.bw, c = r - q * k.bw;
        ty = k.y0 + q; tx = c < k.x0 ? c : c + k.w;
    }
}

// r -> its row-major number in the full grid (no division outside the rectangle's rows)
TW_HD int tile_walk_index(const TileWalk& k, int tiles_x, int r) {
    if (r < k.n_above) return r;
    if (r < k.n_upto) {
        r -= k.n_above;
        const int q = tile_walk_div(r, k.magic_bw), c = r - q * k.bw;
        return (k.y0 + q) * tiles_x + (c < k.x0 ? c : c + k.w);
    }
    return r - k.n_upto + k.y1 * tiles_x;
}

// workgroups per group (cout tile / group) of a persistent grid: one per CU, at least 1, at most `total` (the tiles to share)
inline int tile_walk_grid(int n_cu, int groups, int total) {
    int g = n_cu / groups;
    if (g < 1) g = 1;
    if (g > total) g = total;
    return g;
}

}  // namespace omni
