// fuse_ref.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host restatement of the three Fuse functions, the expected values of
// tests/test_fuse.py (built -O2 -ffp-contract=off, loaded with ctypes):
//   ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false)    src/ORBmatcher.cc:1399-1610  (mode 0)
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)  src/ORBmatcher.cc:1612-1734  (mode 1)
//   LineMatcher::Fuse(pKF, vpMapLines, th)                    src/LineMatcher.cpp:373-485
// downstream of the caller's MapPoint / MapLine reads and cv::Mat products and
// up to the bestDist <= TH_LOW decision, with KeyFrame::GetFeaturesInArea
// (src/KeyFrame.cc:1200-1244) over a grid filled as Frame::AssignFeaturesToGrid
// fills it, KeyFrame::IsInImage and KeyFrame::GetLinesInArea (:1170-1198),
// written sequentially in the reference's own order (one loop over the list,
// vIndices built first, then scanned), not the way the HIP kernels are
// organised.  The fused multiply-adds are the ones the reference objects hold
// (tests/test_ref_objects_fuse.py); -DORACLE_NO_REF_FMA builds the unfused
// variant the tests use to find inputs on which the contraction decides.
//
// Every function reports why each candidate ended as it did, so a test can
// prove from the restatement alone which branch its input takes.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/plvi_frontend.h"
#include "../../oracle/ref_fma.h"

enum {
    FUSE_FLAG = 1,          // !pMP || isBad() || IsInKeyFrame(pKF) / spAlreadyFound.count(pMP); !pML || isBad()
    FUSE_DEPTH = 2,         // z < 0.0f (either endpoint for lines)
    FUSE_IMAGE = 3,         // !IsInImage (points)
    FUSE_DISTANCE = 4,      // dist < minDistance || dist > maxDistance
    FUSE_ANGLE = 5,         // dot < 0.5 * dist
    FUSE_LEVEL = 6,         // predicted level outside [0, nlevels): no scale factor (not reachable in the reference)
    FUSE_EMPTY_WINDOW = 7,  // vIndices.empty()
    FUSE_NO_CANDIDATE = 8,  // every index of vIndices fails the octave (and chi-square) filter: bestIdx stays -1
    FUSE_THRESHOLD = 9,     // bestDist > TH_LOW
    FUSE_ACCEPTED = 10,
    FUSE_BOUNDS_1 = 11,     // lines: the first endpoint outside [mnMin, mnMax]
    FUSE_BOUNDS_2 = 12,     // lines: the second endpoint
};

namespace {

const int TH_LOW = 50;
const int GRID_COLS = 64, GRID_ROWS = 48;  // FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h:47-48)

// ORBmatcher::DescriptorDistance
int descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// LineMatcher::DescriptorDistance (src/LineMatcher.cpp:487-499): the bit count
// of every 32-bit word ends with >> 25 where ORBmatcher's has >> 24, i.e. each
// word contributes half its count, rounded down (row a24 of DESIGN.md)
int line_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int w = 0; w < 8; ++w) {
        int bits = 0;
        for (int i = 4 * w; i < 4 * w + 4; ++i) bits += __builtin_popcount((unsigned)(a[i] ^ b[i]));
        dist += bits >> 1;
    }
    return dist;
}

}  // namespace

// fuse_idx / fuse_dist / code [n_pt]; returns nFused.
extern "C" int fuse_ref_points(const plvi_fuse_params* p, const plvi_keypoint* kps, const uint8_t* desc, int n_kp,
                               const float* uright, const uint8_t* flags, const float* x3dc, const float* dist3,
                               const double* dot, const int* level, const uint8_t* mp_desc, int n_pt, int* fuse_idx,
                               int* fuse_dist, int* code) {
    // Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:688-722, :1077-1089); the KeyFrame copies the grid
    std::vector<int> grid[GRID_COLS][GRID_ROWS];
    for (int i = 0; i < n_kp; ++i) {
        const int posX = (int)roundf((kps[i].x - p->min_x) * p->inv_w);
        const int posY = (int)roundf((kps[i].y - p->min_y) * p->inv_h);
        if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) continue;
        grid[posX][posY].push_back(i);
    }
    const float fx = p->fx, fy = p->fy, cx = p->cx, cy = p->cy, bf = p->bf, th = p->th;
    int nFused = 0;
    for (int i = 0; i < n_pt; ++i) {
        fuse_idx[i] = fuse_dist[i] = -1;
        if (!(flags[i] & 1)) { code[i] = FUSE_FLAG; continue; }
        const float x = x3dc[3 * i], y = x3dc[3 * i + 1], z = x3dc[3 * i + 2];
        if (z < 0.0f) { code[i] = FUSE_DEPTH; continue; }
        const float invz = 1 / z;
        // Pinhole::project (Pinhole.cpp:36-42), no fused operation
        const float u = fx * x / z + cx;
        const float v = fy * y / z + cy;
        if (!(u >= p->min_x && u < p->max_x && v >= p->min_y && v < p->max_y)) { code[i] = FUSE_IMAGE; continue; }
        const float ur = ref_fmaf(-bf, invz, u);  // uv.x - bf*invz: vfnmadd132ss
        const float dist3D = dist3[3 * i], minDistance = dist3[3 * i + 1], maxDistance = dist3[3 * i + 2];
        if (dist3D < minDistance || dist3D > maxDistance) { code[i] = FUSE_DISTANCE; continue; }
        if (dot[i] < 0.5 * dist3D) { code[i] = FUSE_ANGLE; continue; }
        const int nPredictedLevel = level[i];
        if (nPredictedLevel < 0 || nPredictedLevel >= p->nlevels) { code[i] = FUSE_LEVEL; continue; }
        const float radius = th * p->scale_factors[nPredictedLevel];

        // KeyFrame::GetFeaturesInArea(u, v, radius)
        std::vector<int> vIndices;
        do {
            const float r = radius;
            const int nMinCellX = std::max(0, (int)floor((u - p->min_x - r) * p->inv_w));
            if (nMinCellX >= GRID_COLS) break;
            const int nMaxCellX = std::min(GRID_COLS - 1, (int)ceil((u - p->min_x + r) * p->inv_w));
            if (nMaxCellX < 0) break;
            const int nMinCellY = std::max(0, (int)floor((v - p->min_y - r) * p->inv_h));
            if (nMinCellY >= GRID_ROWS) break;
            const int nMaxCellY = std::min(GRID_ROWS - 1, (int)ceil((v - p->min_y + r) * p->inv_h));
            if (nMaxCellY < 0) break;
            for (int ix = nMinCellX; ix <= nMaxCellX; ix++)
                for (int iy = nMinCellY; iy <= nMaxCellY; iy++)
                    for (int j : grid[ix][iy]) {
                        const float distx = kps[j].x - u;
                        const float disty = kps[j].y - v;
                        if (fabs(distx) < r && fabs(disty) < r) vIndices.push_back(j);
                    }
        } while (false);
        if (vIndices.empty()) { code[i] = FUSE_EMPTY_WINDOW; continue; }

        int bestDist = p->mode ? INT_MAX : 256;
        int bestIdx = -1;
        for (int idx : vIndices) {
            const int kpLevel = kps[idx].octave;
            if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
            if (p->mode == 0) {
                if (kpLevel < 0) continue;  // the reference would read mvInvLevelSigma2[-1]: no candidate here
                const float kpx = kps[idx].x, kpy = kps[idx].y;
                const float kpr = uright ? uright[idx] : -1.0f;
                const float ex = u - kpx;
                const float ey = v - kpy;
                if (kpr >= 0) {
                    const float er = ur - kpr;
                    const float e2 = ref_fmaf(er, er, ref_fmaf(ex, ex, ey * ey));  // ex*ex+ey*ey+er*er
                    if (e2 * p->inv_level_sigma2[kpLevel] > 7.8) continue;
                } else {
                    const float e2 = ref_fmaf(ex, ex, ey * ey);
                    if (e2 * p->inv_level_sigma2[kpLevel] > 5.99) continue;
                }
            }
            const int d = descriptor_distance(mp_desc + 32 * (size_t)i, desc + 32 * (size_t)idx);
            if (d < bestDist) {
                bestDist = d;
                bestIdx = idx;
            }
        }
        if (bestDist <= TH_LOW) {
            fuse_idx[i] = bestIdx;
            fuse_dist[i] = bestDist;
            code[i] = FUSE_ACCEPTED;
            nFused++;
        } else {
            code[i] = bestIdx < 0 ? FUSE_NO_CANDIDATE : FUSE_THRESHOLD;
        }
    }
    return nFused;
}

// fuse_idx / fuse_dist / code [n_ml]; returns nFused.
extern "C" int fuse_ref_lines(const plvi_fuse_line_params* p, const plvi_keyline* kl, const uint8_t* kl_desc, int n_kl,
                              const uint8_t* flags, const float* spc, const float* epc, const float* dist3,
                              const double* dot, const int* level, const uint8_t* ml_desc, int n_ml, int* fuse_idx,
                              int* fuse_dist, int* code) {
    const float fx = p->fx, fy = p->fy, cx = p->cx, cy = p->cy, th = p->th;
    int nFused = 0;
    for (int iML = 0; iML < n_ml; ++iML) {
        fuse_idx[iML] = fuse_dist[iML] = -1;
        if (!(flags[iML] & 1)) { code[iML] = FUSE_FLAG; continue; }
        const float SPcX = spc[3 * iML], SPcY = spc[3 * iML + 1], SpcZ = spc[3 * iML + 2];
        const float EPcX = epc[3 * iML], EPcY = epc[3 * iML + 1], EPcZ = epc[3 * iML + 2];
        if (SpcZ < 0.0f || EPcZ < 0.0f) { code[iML] = FUSE_DEPTH; continue; }
        const float invz1 = 1.0f / SpcZ;
        const float u1 = ref_fmaf(fx * SPcX, invz1, cx);  // fx * SPcX * invz1 + cx: vmulss, vfmadd132ss
        const float v1 = ref_fmaf(fy * SPcY, invz1, cy);
        if (u1 < p->min_x || u1 > p->max_x) { code[iML] = FUSE_BOUNDS_1; continue; }
        if (v1 < p->min_y || v1 > p->max_y) { code[iML] = FUSE_BOUNDS_1; continue; }
        const float invz2 = 1.0f / EPcZ;
        const float u2 = ref_fmaf(fx * EPcX, invz2, cx);
        const float v2 = ref_fmaf(fy * EPcY, invz2, cy);
        if (u2 < p->min_x || u2 > p->max_x) { code[iML] = FUSE_BOUNDS_2; continue; }
        if (v2 < p->min_y || v2 > p->max_y) { code[iML] = FUSE_BOUNDS_2; continue; }
        const float dist = dist3[3 * iML], minDistance = dist3[3 * iML + 1], maxDistance = dist3[3 * iML + 2];
        if (dist < minDistance || dist > maxDistance) { code[iML] = FUSE_DISTANCE; continue; }
        if (dot[iML] < 0.5 * dist) { code[iML] = FUSE_ANGLE; continue; }
        const int nPredictedLevel = level[iML];
        if (nPredictedLevel < 0 || nPredictedLevel >= p->nlevels) { code[iML] = FUSE_LEVEL; continue; }
        const float radius = th * p->scale_factors[nPredictedLevel];

        // KeyFrame::GetLinesInArea(u1, v1, u2, v2, radius, -1, -1): bCheckLevels is false
        std::vector<int> vIndices;
        {
            const float x1 = u1, y1 = v1, x2 = u2, y2 = v2, r = radius;
            for (int i = 0; i < n_kl; i++) {
                // (0.5 * (x1 + x2) - pt.x)^2 + (0.5 * (y1 + y2) - pt.y)^2 in double, as KeyFrame.cc.o fuses it
                const double dx = ref_fma(0.5, (double)(x1 + x2), -(double)kl[i].pt_x);
                const double dy = ref_fma(0.5, (double)(y1 + y2), -(double)kl[i].pt_y);
                const float distance = (float)ref_fma(dx, dx, dy * dy);
                if (distance > r * r) continue;
                const float slope = (y1 - y2) / (x1 - x2) - kl[i].angle;
                if (slope > r * 0.01) continue;
                vIndices.push_back(i);
            }
        }
        if (vIndices.empty()) { code[iML] = FUSE_EMPTY_WINDOW; continue; }

        int bestDist = INT_MAX;
        int bestIdx = -1;
        for (int idx : vIndices) {
            const int klLevel = kl[idx].octave;
            if (klLevel < nPredictedLevel - 1 || klLevel > nPredictedLevel) continue;
            const int d = line_descriptor_distance(ml_desc + 32 * (size_t)iML, kl_desc + 32 * (size_t)idx);
            if (d < bestDist) {
                bestDist = d;
                bestIdx = idx;
            }
        }
        if (bestDist <= TH_LOW) {
            fuse_idx[iML] = bestIdx;
            fuse_dist[iML] = bestDist;
            code[iML] = FUSE_ACCEPTED;
            nFused++;
        } else {
            code[iML] = bestIdx < 0 ? FUSE_NO_CANDIDATE : FUSE_THRESHOLD;
        }
    }
    return nFused;
}
