// jpeg_plan_pin: csrc/jpeg_plan.h built with g++ alone (tests/test_jpeg_plan_cpu.py, tests/jpeg_cases.py).
//   jpeg_plan_pin <in> <out>
// in:  int32 n; per case int32 {w, h, stride, quality, zero_from_row, capacity} + stride * h bytes
// out: per case int32 {status, size} + capacity + 16 bytes: the output buffer, filled with 0xA5 before the call (the 16 behind the capacity are the guard)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jpeg_plan.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t n = 0;
    if (fread(&n, 4, 1, in) != 1) return 3;
    for (int i = 0; i < n; ++i) {
        int32_t a[6];
        if (fread(a, 4, 6, in) != 6) return 3;
        std::vector<uint8_t> img((size_t)a[2] * a[1]), buf((size_t)a[5] + 16, 0xA5);
        if (fread(img.data(), 1, img.size(), in) != img.size()) return 3;
        int64_t size = -1;
        const int32_t status = omni::jp::jpeg_encode_host(img.data(), a[2], a[0], a[1], a[3], a[4], buf.data(), a[5], &size);
        const int32_t r[2] = {status, (int32_t)size};
        fwrite(r, 4, 2, out);
        fwrite(buf.data(), 1, buf.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 4;
}
