// The tile walk of the persistent kernels (omni-swarm_amd/csrc/tile_walk.h) on the host.  Arguments: tiles_x tiles_y batch, then rectangles
// ty0 ty1 tx0 tx1 (tile rows [ty0, ty1) x tile columns [tx0, tx1) left out).  Writes to stdout, per rectangle, little-endian uint16: the number n of
// tiles that run (batch x TileWalk::act; 65535: the plan refused the rectangle), then n triples in walk order t = 0 .. n - 1 -- the tile's number
// b x tiles_x x tiles_y + ty x tiles_x + tx in the full grid from tile_walk_rc (multiply-high), from tile_walk_rc<false> (hardware division), and
// from tile_walk_index; b = t / act by multiply-high as the kernels do.  tests/test_mask_skip_cpu.py enumerates what the walk must be.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../omni-swarm_amd/csrc/tile_walk.h"

namespace omni {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
}
}  // namespace omni

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 4) % 4 != 0) {
        fprintf(stderr, "usage: %s tiles_x tiles_y batch [ty0 ty1 tx0 tx1] ...\n", argv[0]);
        return 2;
    }
    const int tiles_x = atoi(argv[1]), tiles_y = atoi(argv[2]), batch = atoi(argv[3]), tiles_img = tiles_x * tiles_y;
    if ((int64_t)batch * tiles_img >= 65535) {
        fprintf(stderr, "grid too large for 16-bit output\n");
        return 2;
    }
    std::vector<uint16_t> out;
    for (int i = 4; i < argc; i += 4) {
        omni::TileWalk k;
        if (omni::tile_walk_plan(k, "tile_walk_pin", tiles_x, tiles_y, atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3])) != OMNI_OK) {
            out.push_back(65535);
            continue;
        }
        const int n = batch * k.act;
        const uint32_t m_act = omni::tile_walk_magic(k.act);
        out.push_back((uint16_t)n);
        for (int t = 0; t < n; ++t) {
            const int b = omni::tile_walk_div(t, m_act), r = t - b * k.act;
            int ty, tx, ty2, tx2;
            omni::tile_walk_rc(k, tiles_x, r, ty, tx);
            omni::tile_walk_rc<false>(k, tiles_x, r, ty2, tx2);
            out.push_back((uint16_t)(b * tiles_img + ty * tiles_x + tx));
            out.push_back((uint16_t)(b * tiles_img + ty2 * tiles_x + tx2));
            out.push_back((uint16_t)(b * tiles_img + omni::tile_walk_index(k, tiles_x, r)));
        }
    }
    fwrite(out.data(), 2, out.size(), stdout);
    return 0;
}
