// Pins omni-swarm_amd/csrc/cam_input.h: where a key-frame unit's input bytes go and in which order its steps run, for every way the frames arrive.  A stand-alone
// program: plain g++, nothing of the GPU library; tests/test_cam_input_plan_cpu.py builds it with -fsanitize=address,undefined and compares every field it writes
// with its own restatement of the rules.
//   cam_input_pin <cases> <out>
//   cases  int32 count; per case 19 x int32: form pre cams n W H n_cap src_w[2] src_h[2] stride frames first_view dirs fisheye_mask n_parts[2] lists, then (lists
//          != 0) the frames of camera 0's parts and of camera 1's, int32 each
//   out    per case int64s: ok (n_steps != 0); and if ok: gray_bytes raw_bytes gray_cam1 raw_cam1 stage n_parts[2], per camera and part (dst bytes rows), dec_images dec_stride
//          dec_w dec_h dec_max dec_cap pre_src pre_stride unit_src unit_stride unit_mask n_steps, per step (kind cam)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cam_input.h"

using namespace omni::ci;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fin = fopen(argv[1], "rb");
    FILE* fout = fopen(argv[2], "wb");
    if (!fin || !fout) return 3;
    int32_t count = 0;
    if (fread(&count, 4, 1, fin) != 1) return 4;
    for (int32_t i = 0; i < count; ++i) {
        int32_t h[19];
        if (fread(h, 4, 19, fin) != 19) return 5;
        CamInput in;
        in.form = h[0]; in.pre = h[1]; in.cams = h[2]; in.n = h[3]; in.W = h[4]; in.H = h[5]; in.n_cap = h[6];
        in.src_w[0] = h[7]; in.src_w[1] = h[8]; in.src_h[0] = h[9]; in.src_h[1] = h[10]; in.stride = h[11]; in.frames = h[12];
        in.first_view = h[13]; in.dirs = h[14]; in.fisheye_mask = h[15]; in.n_parts[0] = h[16]; in.n_parts[1] = h[17];
        std::vector<int32_t> lists[2];                                // (heap blocks of exactly the parts' count: a read past a list is the sanitizer's to find)
        for (int cam = 0; cam < 2 && h[18]; ++cam) {
            lists[cam].resize(in.n_parts[cam] > 0 ? in.n_parts[cam] : 0);
            if (!lists[cam].empty() && fread(lists[cam].data(), 4, lists[cam].size(), fin) != lists[cam].size()) return 6;
            in.part_frames[cam] = lists[cam].data();
        }
        CamInputPlan* p = new CamInputPlan(plan(in));                 // (on the heap too: a read past the plan's tables likewise)
        std::vector<int64_t> o;
        o.push_back(p->n_steps ? 1 : 0);
        if (o[0]) {
            for (size_t v : {p->gray_bytes, p->raw_bytes, p->gray_cam1, p->raw_cam1}) o.push_back((int64_t)v);
            for (int v : {p->stage, p->n_parts[0], p->n_parts[1]}) o.push_back(v);
            for (int cam = 0; cam < 2; ++cam)
                for (int k = 0; k < p->n_parts[cam]; ++k)
                    for (size_t v : {p->part[cam][k].dst, p->part[cam][k].bytes, p->part[cam][k].rows}) o.push_back((int64_t)v);
            for (int v : {p->dec_images, p->dec_stride, p->dec_w, p->dec_h, p->dec_max}) o.push_back(v);
            o.push_back(p->dec_cap);
            for (int v : {p->pre_src, p->pre_stride, p->unit_src, p->unit_stride, p->unit_mask, p->n_steps}) o.push_back(v);
            for (int k = 0; k < p->n_steps; ++k) { o.push_back(p->steps[k].kind); o.push_back(p->steps[k].cam); }
        }
        delete p;
        if (fwrite(o.data(), 8, o.size(), fout) != o.size()) return 7;
    }
    return fclose(fout) == 0 ? 0 : 8;
}
