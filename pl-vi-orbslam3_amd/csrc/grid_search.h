// grid_search.h — the device pieces every grid-window matcher shares:
//   Frame::GetFeaturesInArea (src/Frame.cc:1006-1075): the cell-range clamps
//     (grid_window) and the candidate walk over the CSR grid (grid_walk)
//   ORBmatcher::DescriptorDistance (hamming256, block_prims.h)
//   ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:2304-2345) and the
//     rotation-histogram bin (three_maxima, rot_bin)
//   one image's keypoints and grid in LDS (GridSide, grid_side_load)
//   the rotation filter + match write-back of the one-camera histogram
//     matchers (rotation_filter_and_store)
// Users: proj.hip, init_match.hip, bow.hip, grid_match.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "block_prims.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kGridCols = 64, kGridRows = 48, kGridCells = kGridCols * kGridRows;  // include/Frame.h:47-48

// The cell range of GetFeaturesInArea(u, v, radius); false where the
// reference returns an empty vIndices early (:1013-1037, in its order).
struct GridWindow {
    int nMinCellX, nMaxCellX, nMinCellY, nMaxCellY;
};

__device__ __forceinline__ bool grid_window(float min_x, float min_y, float inv_w, float inv_h, float u, float v,
                                            float radius, GridWindow& w) {
    w.nMinCellX = max(0, (int)floorf((u - min_x - radius) * inv_w));
    if (w.nMinCellX >= kGridCols) return false;
    w.nMaxCellX = min(kGridCols - 1, (int)ceilf((u - min_x + radius) * inv_w));
    if (w.nMaxCellX < 0) return false;
    w.nMinCellY = max(0, (int)floorf((v - min_y - radius) * inv_h));
    if (w.nMinCellY >= kGridRows) return false;
    w.nMaxCellY = min(kGridRows - 1, (int)ceilf((v - min_y + radius) * inv_h));
    if (w.nMaxCellY < 0) return false;
    return true;
}

// ComputeThreeMaxima over hist[0, L): keep[] = the bins that survive (-1: none).
__device__ __forceinline__ void three_maxima(const int* hist, int L, int keep[3]) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int b = 0; b < L; b++) {
        const int c = hist[b];
        if (c > max1) {
            max3 = max2; max2 = max1; max1 = c;
            ind3 = ind2; ind2 = ind1; ind1 = b;
        } else if (c > max2) {
            max3 = max2; max2 = c;
            ind3 = ind2; ind2 = b;
        } else if (c > max3) {
            max3 = c;
            ind3 = b;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
    keep[0] = ind1; keep[1] = ind2; keep[2] = ind3;
}

// The rotation-histogram bin of an angle difference (factor = 1.0f / HISTO_LENGTH).
__device__ __forceinline__ int rot_bin(float rot, int L) {
    const float factor = 1.0f / L;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == L) bin = 0;
    return bin;
}

// One image's keypoints and grid in LDS, with the assignment state of the
// greedy matchers: `pre` = blocked on entry, `blocked` = blocked now,
// assign[i] = the point matched to keypoint i, nulled[i] = dropped by the
// rotation filter (only the kernels that have one carve it).
struct GridSide {
    float *kx, *ky;
    int *assign, *cell_off;
    unsigned short* cell_idx;
    unsigned char *koct, *blocked, *pre, *nulled;
    const plvi_keypoint* K;
    const uint8_t* desc;
    int n;
};

// The one-camera kernels keep their per-point tables between the side's
// arrays (after assign, after cell_idx): bytes[] in, at[] out.
struct GridGaps {
    size_t bytes[2];
    unsigned char* at[2];
};

// Image `img` of a batch ([img][cap] tables, blocked_all may be NULL) into d:
// carves d's arrays from q (advanced, 16-aligned) and loads them.
// kNormBlocked: entry flags stored as != 0.  The bytes taken are what the
// *_smem() formulas of proj.hip count.
template <bool kNulled, bool kNormBlocked>
__device__ __forceinline__ void grid_side_load(GridSide& d, unsigned char*& q, int img, int cap,
                                               const plvi_keypoint* kps_all, const uint8_t* desc_all, const int* n_all,
                                               const uint8_t* blocked_all, const int* cell_off_all,
                                               const int* cell_idx_all, int tid, GridGaps* gaps = nullptr) {
    d.n = min(n_all[img], cap);
    d.K = kps_all + (size_t)img * cap;
    d.desc = desc_all + (size_t)img * cap * 32;
    const uint8_t* blocked = blocked_all ? blocked_all + (size_t)img * cap : nullptr;
    const int* CO = cell_off_all + (size_t)img * (kGridCells + 1);
    const int* CI = cell_idx_all + (size_t)img * cap;
    d.kx = reinterpret_cast<float*>(q); q += 4 * cap;
    d.ky = reinterpret_cast<float*>(q); q += 4 * cap;
    d.assign = reinterpret_cast<int*>(q); q += 4 * cap;
    if (gaps) { gaps->at[0] = q; q += gaps->bytes[0]; }
    d.cell_off = reinterpret_cast<int*>(q); q += 4 * (kGridCells + 1);
    d.cell_idx = reinterpret_cast<unsigned short*>(q); q += 2 * cap;
    if (gaps) { gaps->at[1] = q; q += gaps->bytes[1]; }
    d.koct = q; q += cap;
    d.blocked = q; q += cap;
    d.pre = q; q += cap;
    d.nulled = nullptr;
    if (kNulled) { d.nulled = q; q += cap; }
    q = reinterpret_cast<unsigned char*>(((uintptr_t)q + 15) & ~(uintptr_t)15);
    for (int i = tid; i < d.n; i += 256) {
        d.kx[i] = d.K[i].x;
        d.ky[i] = d.K[i].y;
        d.koct[i] = (unsigned char)d.K[i].octave;
        const unsigned char b = blocked ? (kNormBlocked ? (unsigned char)(blocked[i] != 0) : blocked[i]) : 0;
        d.blocked[i] = b;
        d.pre[i] = b;
        if (kNulled) d.nulled[i] = 0;
        d.assign[i] = -1;
    }
    for (int c = tid; c <= kGridCells; c += 256) d.cell_off[c] = CO[c];
    const int ncell = CO[kGridCells];
    for (int k = tid; k < ncell; k += 256) d.cell_idx[k] = (unsigned short)CI[k];
}

// The accumulators of grid_walk: first argmin, or first argmin plus the
// first argmin of the rest (the scan order of GetFeaturesInArea).
struct BestOne {
    int dist = 256, idx = -1;
    __device__ __forceinline__ void operator()(int d, int i) {
        if (d < dist) {
            dist = d;
            idx = i;
        }
    }
};

struct BestTwo {
    int dist = 256, dist2 = 256, idx = -1, idx2 = -1;
    __device__ __forceinline__ void operator()(int d, int i) {
        if (d < dist) {
            dist2 = dist;
            idx2 = idx;
            dist = d;
            idx = i;
        } else if (d < dist2) {
            dist2 = d;
            idx2 = i;
        }
    }
};

// The extra rejections of grid_walk: none, or the mvuRight test of the
// stereo-rectified frames (|xr - mvuRight[i2]| > radius where mvuRight > 0).
struct NoReject {
    __device__ __forceinline__ bool operator()(int) const { return false; }
};

struct UrightReject {
    const float* uright;  // NULL: monocular
    float xr, radius;
    __device__ __forceinline__ bool operator()(int i2) const {
        return uright && uright[i2] > 0 && fabsf(xr - uright[i2]) > radius;
    }
};

// The keypoints of window w in GetFeaturesInArea's order (grid column by
// column, one CSR range each): the level filter (bCheckLevels as the
// reference computes it), the |dx|, |dy| < radius test -- a keypoint that
// passes both is in vIndices, the return value says whether one did -- then
// the caller's loop body: the blocked test, `reject`, and the descriptor
// distance to mpd handed to `acc`.
template <class Reject, class Acc>
__device__ __forceinline__ bool grid_walk(const GridSide& s, const unsigned char* blk, const GridWindow& w, float u,
                                          float v, float radius, bool bCheckLevels, int minLevel, int maxLevel,
                                          const uint8_t* __restrict__ mpd, const Reject& reject, Acc& acc) {
    const uint4* dm = reinterpret_cast<const uint4*>(mpd);
    const uint4 m0 = dm[0], m1 = dm[1];
    bool any = false;
    for (int ix = w.nMinCellX; ix <= w.nMaxCellX; ++ix) {
        const int k0 = s.cell_off[ix * kGridRows + w.nMinCellY], k1 = s.cell_off[ix * kGridRows + w.nMaxCellY + 1];
        for (int k = k0; k < k1; ++k) {
            const int i2 = s.cell_idx[k];
            if (bCheckLevels) {
                const int o = s.koct[i2];
                if (o < minLevel) continue;
                if (maxLevel >= 0 && o > maxLevel) continue;
            }
            const float distx = s.kx[i2] - u, disty = s.ky[i2] - v;
            if (!(fabsf(distx) < radius && fabsf(disty) < radius)) continue;
            any = true;
            if (blk[i2]) continue;
            if (reject(i2)) continue;
            acc(hamming256(m0, m1, s.desc + (size_t)32 * i2), i2);
        }
    }
    return any;
}

// Phase 3 of the one-camera histogram matchers: entries (ent[e] = keypoint,
// ent[ent_cap + e] = bin) in a dropped bin set mvpMapPoints[idx] = NULL;
// then match[] (-2: dropped, -1: none) and the live match count.
__device__ __forceinline__ void rotation_filter_and_store(const GridSide& s, bool check_orientation,
                                                          const unsigned short* ent, int ent_cap, const int* keep,
                                                          const int* ne, int* nm, int* __restrict__ M,
                                                          int* __restrict__ nmatches, int tid) {
    if (check_orientation) {
        const int n = *ne;
        int dropped = 0;
        for (int e = tid; e < n; e += 256) {
            const int bin = ent[ent_cap + e];
            if (bin != keep[0] && bin != keep[1] && bin != keep[2]) {
                s.nulled[ent[e]] = 1;
                ++dropped;
            }
        }
        if (dropped) atomicSub(nm, dropped);
        __syncthreads();
    }
    for (int i = tid; i < s.n; i += 256) M[i] = s.nulled[i] ? -2 : s.assign[i];
    if (tid == 0) *nmatches = *nm;
}

}  // namespace plvi
