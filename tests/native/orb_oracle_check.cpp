// Stand-alone driver of the CPU oracle's ORB extractor (oracle/orb_oracle.cpp
// + oracle/cvprim.cpp) for a sanitizer build (tests/test_oracle_kat.py builds
// it with -fsanitize=address,undefined): the shapes the extractor must refuse
// return -2 with no keypoints and touch nothing out of bounds on the way, and
// the smallest accepted shapes run clean.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../oracle/oracle_api.h"

extern "C" int oracle_orb_extract(const uint8_t* img, int w, int h, int stride, int nfeatures, float scaleFactor,
                                  int nlevels, int iniTh, int minTh, int lap0, int lap1, plvi_keypoint* kps,
                                  uint8_t* desc, int cap, int* n);

struct Case {
    int w, h;
    float scale;
    int nlevels;
    bool refused;
};

int main() {
    const Case cases[] = {
        {70, 200, 1.2f, 1, true},   // nIni = round(38 / 168) = 0 octree roots
        {61, 61, 1.2f, 1, true},    // no 30-px cell
        {100, 80, 2.0f, 2, true},   // level 1 (50 x 40) has no cell
        {62, 62, 1.2f, 1, false},   // smallest legal level: one cell, one root
        {160, 120, 1.2f, 3, false},
    };
    const int cap = 4096;
    std::vector<plvi_keypoint> kps(cap);
    std::vector<uint8_t> desc((size_t)cap * 32);
    int bad = 0;
    for (const Case& c : cases) {
        // exact-size buffers: a read past the image is a heap overflow
        std::vector<uint8_t> img((size_t)c.w * c.h);
        for (int pass = 0; pass < 2; ++pass) {
            // pass 0: noise (corners everywhere); pass 1: 8-px blocks (few, strong corners)
            uint32_t s = 12345u;
            for (int y = 0; y < c.h; ++y)
                for (int x = 0; x < c.w; ++x) {
                    s = s * 1664525u + 1013904223u;
                    img[(size_t)y * c.w + x] = pass == 0 ? (uint8_t)(s >> 24) : (uint8_t)(((x / 8 + y / 8) % 3) * 100);
                }
            int n = -1;
            const int rc = oracle_orb_extract(img.data(), c.w, c.h, c.w, 1000, c.scale, c.nlevels, 20, 7, 0, 0,
                                              kps.data(), desc.data(), cap, &n);
            const bool ok = c.refused ? (rc == -2 && n == 0) : (rc >= 0 && n >= 0 && rc == n);
            std::printf("%dx%d scale %.1f levels %d pass %d: rc %d n %d %s\n", c.w, c.h, c.scale, c.nlevels, pass, rc,
                        n, ok ? "ok" : "BAD");
            bad += !ok;
        }
    }
    return bad ? 1 : 0;
}
