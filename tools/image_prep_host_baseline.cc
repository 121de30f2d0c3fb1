// tools/image_prep_host_baseline.cc -- one-thread host statement of the image front end's arithmetic (include/orbx.h, "Image front end"), for
// tools/latency_image_prep.py: colour to grey, then the bilinear remap of the grey image through maps converted once to fixed point.
// Plain loops on plain arrays, no SIMD intrinsics (the compiler may vectorise the grey loop), no OpenCV: what a caller would write in front
// of the device batch path if the library did not do it.  NOT the reference's cvtColor / remap (the OpenCV stand-in has no remap): no reference timing.
//
//   image_prep_host_baseline scene.bin reps   ->   "image_prep <us per frame> <checksum>"
// scene.bin: int32 magic, w, h, channels, frames, rgb, rectify, shift; uint32 coef[3] (R, G, B); the frames (tight rows); with rectify: map_x, map_y (float, w * h each).
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static inline int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s scene.bin reps\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hd[8];
    uint32_t coef[3];
    if (fread(hd, 4, 8, f) != 8 || hd[0] != 0x494d4750 || fread(coef, 4, 3, f) != 3) { fprintf(stderr, "bad scene file\n"); return 2; }
    const int w = hd[1], h = hd[2], C = hd[3], n = hd[4], rgb = hd[5], rect = hd[6], shift = hd[7], reps = atoi(argv[2]);
    const size_t px = (size_t)w * h;
    std::vector<uint8_t> src(px * C * n), gray(px), out(px * n);
    std::vector<float> mx(rect ? px : 0), my(rect ? px : 0);
    if (fread(src.data(), 1, src.size(), f) != src.size() || (rect && (fread(mx.data(), 4, px, f) != px || fread(my.data(), 4, px, f) != px))) { fprintf(stderr, "short scene file\n"); return 2; }
    fclose(f);
    // the maps, once: sx = rint(map * 32) half to even, ix = saturate_int16(sx >> 5), fx = sx & 31
    std::vector<int16_t> ix(mx.size()), iy(mx.size());
    std::vector<uint16_t> fr(mx.size());
    for (size_t i = 0; i < mx.size(); i++) {
        const int sx = (int)fminf(fmaxf(rintf(mx[i] * 32.0f), -1073741824.0f), 1073741824.0f), sy = (int)fminf(fmaxf(rintf(my[i] * 32.0f), -1073741824.0f), 1073741824.0f);
        ix[i] = (int16_t)sat16(sx >> 5); iy[i] = (int16_t)sat16(sy >> 5);
        fr[i] = (uint16_t)((sx & 31) | (sy & 31) << 5);
    }
    const uint32_t c0 = rgb ? coef[0] : coef[2], c1 = coef[1], c2 = rgb ? coef[2] : coef[0], rnd = 1u << (shift - 1);
    const auto t0 = std::chrono::steady_clock::now();
    for (int rep = 0; rep < reps; rep++)
        for (int k = 0; k < n; k++) {
            const uint8_t *s = src.data() + px * C * k;
            uint8_t *o = out.data() + px * k;
            const uint8_t *g = s;
            if (C > 1) {
                uint8_t *gd = rect ? gray.data() : o;
                for (size_t i = 0; i < px; i++) gd[i] = (uint8_t)((c0 * s[C * i] + c1 * s[C * i + 1] + c2 * s[C * i + 2] + rnd) >> shift);
                g = gd;
            }
            if (!rect) {
                if (C == 1) for (size_t i = 0; i < px; i++) o[i] = s[i];
                continue;
            }
            for (size_t i = 0; i < px; i++) {
                const int x = ix[i], y = iy[i];
                const uint32_t fx = fr[i] & 31u, fy = fr[i] >> 5;
                uint32_t p00, p01, p10, p11;
                if ((unsigned)x < (unsigned)(w - 1) && (unsigned)y < (unsigned)(h - 1)) {
                    const uint8_t *p = g + (size_t)y * w + x;
                    p00 = p[0]; p01 = p[1]; p10 = p[w]; p11 = p[w + 1];
                } else {
                    const bool x0 = (unsigned)x < (unsigned)w, x1 = (unsigned)(x + 1) < (unsigned)w, y0 = (unsigned)y < (unsigned)h, y1 = (unsigned)(y + 1) < (unsigned)h;
                    p00 = y0 && x0 ? g[(size_t)y * w + x] : 0; p01 = y0 && x1 ? g[(size_t)y * w + x + 1] : 0;
                    p10 = y1 && x0 ? g[(size_t)(y + 1) * w + x] : 0; p11 = y1 && x1 ? g[(size_t)(y + 1) * w + x + 1] : 0;
                }
                o[i] = (uint8_t)(((32 - fx) * (32 - fy) * p00 + fx * (32 - fy) * p01 + (32 - fx) * fy * p10 + fx * fy * p11 + 512) >> 10);
            }
        }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / ((double)reps * n);
    uint64_t chk = 0;
    for (size_t i = 0; i < out.size(); i++) chk += (uint64_t)out[i] * (1 + i % 7);
    printf("image_prep %.3f %llu\n", us, (unsigned long long)chk);
    return 0;
}
