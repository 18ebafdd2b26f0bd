// orb_xtab.h -- the packed column table of the ORB pyramid kernels: the entry
// format the kernels unpack (orb_kernels.hpp: pyr_quad) and the host code that
// builds it (orb_pipeline.hip).  Plain C++ on the host side, so that
// tests/native/xtab_check.cpp can build the table without a HIP compiler.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "plvi_frontend.h"

#if defined(__HIPCC__)
#define PLVI_XTAB_HD __host__ __device__
#else
#define PLVI_XTAB_HD
#endif

namespace plvi {

// packed column entry: sx (10 bits) | a0 (12 bits) << 10 | (a0 + a1 - 2047) (2 bits) << 22 | clampR << 24
// (a clampR column has a0 = 2048, a1 = 0: its second tap never counts).  Every
// level's entries start at a multiple of four and are padded to one with
// copies of the last column (append_xtab), so a quad is one 16-byte read.
PLVI_XTAB_HD inline uint32_t pyr_xtab_pack(int sx, int a0, int a1, bool clampR) {
    return (uint32_t)sx | ((uint32_t)a0 << 10) | ((uint32_t)(a0 + a1 - 2047) << 22) | ((uint32_t)clampR << 24);
}
// kPyrXtabAreaTail: a column of the INTER_AREA scalar tail (orb_kernels.hpp).
// kPyrXtabWide: on the first entry of every quad of a level in which some
// quad's taps span more than 8 source bytes (a scale well above 2): such a
// level takes the per-pixel path, never a window that misses a tap.
constexpr uint32_t kPyrXtabAreaTail = 1u << 25;
constexpr uint32_t kPyrXtabWide = 1u << 26;

static inline int cv_round_h(float v) { return (int)lrintf(v); }
static inline int cv_round_h(double v) { return (int)lrint(v); }
static inline int cv_floor_h(float v) { int i = (int)v; return i - (i > v); }
static inline int cv_ceil_h(float v) { int i = (int)v; return i + (i < v); }

// cv::resize INTER_LINEAR 8U column coefficients (imgproc/src/resize.cpp,
// OpenCV 4.2: scale_x = 1/inv_scale_x, fx = (float)((dx+0.5)*scale_x-0.5),
// sx = cvFloor(fx), border clamps, cvRound(... * INTER_RESIZE_COEF_SCALE)),
// packed for orb_pyramid_kernel; dx >= xmax columns use S[sx] * 2048 only.
// `area` (the level is exactly half of its source in both axes, so cv::resize
// takes the INTER_AREA fast path): columns of ResizeAreaFastVec_SIMD_8u's
// scalar tail, dx >= (sw / 2 / 8) * 8, carry kPyrXtabAreaTail; every other
// column of such a level has sx = 2 dx, a0 = a1 = 1024, the same result.
// The kernels take four columns at a time: a level's entries start at a
// multiple of four (16-byte aligned in LDS and in memory) and are padded to
// one with copies of the last column.  A quad's taps must lie in the 8 bytes
// from its first sx on; if one quad of the level does not (a scale well above
// 2), the first entry of every quad carries kPyrXtabWide and the level is
// built pixel by pixel.
static inline int append_xtab(std::vector<uint32_t>& tab, int sw, int dw, bool area) {
    const double scale_x = 1. / ((double)dw / sw);
    const int tail0 = area ? (sw / 2 / 8) * 8 : dw;
    if (sw < 8 || tab.size() % 4) return PLVI_E_BADARG;
    const size_t first = tab.size();
    for (int dx = 0; dx < dw; ++dx) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor_h(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        const bool clampR = sx + 1 >= sw;
        if (clampR && sx >= sw - 1) { fx = 0; sx = sw - 1; }
        const int a0 = cv_round_h((1.f - fx) * 2048), a1 = cv_round_h(fx * 2048);
        if (sx > 1023 || a0 + a1 < 2047 || a0 + a1 > 2049) return PLVI_E_BADARG;
        if (area && (sx != 2 * dx || a0 != 1024 || a1 != 1024 || clampR)) return PLVI_E_BADARG;
        // the kernels take a1 = 2047 - a0 + (a0 + a1 - 2047) for every column: a clampR column is (2048, 0)
        if (clampR && (a0 != 2048 || a1 != 0)) return PLVI_E_BADARG;
        tab.push_back(pyr_xtab_pack(sx, a0, a1, clampR) | (dx >= tail0 ? kPyrXtabAreaTail : 0u));
    }
    while (tab.size() % 4) tab.push_back(tab.back());
    bool wide = false;
    for (size_t q = first; q < tab.size(); q += 4) wide |= (tab[q + 3] & 1023u) - (tab[q] & 1023u) > 6;
    if (wide)
        for (size_t q = first; q < tab.size(); q += 4) tab[q] |= kPyrXtabWide;
    return PLVI_OK;
}

}  // namespace plvi
