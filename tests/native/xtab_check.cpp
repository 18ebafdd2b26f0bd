// xtab_check -- the ORB pyramid kernels' packed column table (csrc/orb_xtab.h:
// append_xtab) against cv::resize's column coefficients, re-derived here for
// every (source width, level width) pair given on the command line:
//   * every column's sx / a0 / a1 / clampR unpack to the INTER_LINEAR values
//     (resize.cpp: fx = (float)((dx + 0.5) * scale_x - 0.5), cvFloor, the
//     border clamps, cvRound(... * 2048)), as the kernels unpack them
//     (a1 = 2047 - a0 + the 2-bit field);
//   * a level starts at a multiple of four entries and is padded to one with
//     copies of its last column;
//   * kPyrXtabWide sits on the first entry of every quad or of none, and a
//     level without it has every tap of every quad inside the 8 bytes from the
//     quad's first sx (what pyr_quad's window holds);
//   * the area tail flag sits on the columns from (sw / 2 / 8) * 8 on.
// usage: xtab_check sw:dw[:a] ...   (a: the level takes the INTER_AREA path)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orb_xtab.h"

int main(int argc, char** argv) {
    long checked = 0, mismatches = 0;
    std::vector<uint32_t> tab;
    for (int i = 1; i < argc; ++i) {
        int sw = 0, dw = 0;
        char a = 0;
        if (std::sscanf(argv[i], "%d:%d:%c", &sw, &dw, &a) < 2) return 2;
        const bool area = a == 'a';
        const size_t first = tab.size();
        if (plvi::append_xtab(tab, sw, dw, area) != PLVI_OK) {
            std::printf("refused %s\n", argv[i]);
            return 1;
        }
        auto bad = [&](const char* what, int dx) {
            ++mismatches;
            std::printf("%s: %s at column %d\n", argv[i], what, dx);
        };
        if (first % 4 || tab.size() % 4 || tab.size() - first != (size_t)((dw + 3) & ~3)) bad("padding", -1);
        const double scale_x = 1. / ((double)dw / sw);
        const int tail0 = area ? (sw / 2 / 8) * 8 : dw;
        const bool wide = tab[first] & plvi::kPyrXtabWide;
        for (int dx = 0; dx < (int)(tab.size() - first); ++dx) {
            const uint32_t e = tab[first + dx];
            const int cx = dx < dw ? dx : dw - 1;  // padding repeats the last column
            float fx = (float)((cx + 0.5) * scale_x - 0.5);
            int sx = (int)std::floor(fx);
            fx -= sx;
            if (sx < 0) { fx = 0; sx = 0; }
            const bool clampR = sx >= sw - 1;  // dx >= xmax: S[sx] * 2048 only
            if (clampR) { fx = 0; sx = sw - 1; }
            const int a0 = (int)std::lrint((1.f - fx) * 2048), a1 = (int)std::lrint(fx * 2048);
            const int ua0 = (e >> 10) & 4095, ua1 = 2047 - ua0 + ((e >> 22) & 3);
            if ((int)(e & 1023) != sx) bad("sx", dx);
            if (ua0 != a0 || ua1 != a1) bad("a0/a1", dx);
            if ((bool)((e >> 24) & 1) != clampR) bad("clampR", dx);
            if ((bool)(e & plvi::kPyrXtabAreaTail) != (cx >= tail0)) bad("area tail", dx);
            if ((bool)(e & plvi::kPyrXtabWide) != (wide && dx % 4 == 0)) bad("wide flag", dx);
            if (!wide) {
                const int sx0 = tab[first + (dx & ~3)] & 1023;
                if (sx < sx0 || sx - sx0 > 7 || (!clampR && sx + 1 - sx0 > 7)) bad("tap outside the 8-byte window", dx);
            }
            ++checked;
        }
    }
    std::printf("checked=%ld mismatches=%ld\n", checked, mismatches);
    return mismatches ? 1 : 0;
}
