// proj.hip — the steady-state frame-to-frame ORB matcher on the device:
//   Frame::AssignFeaturesToGrid (src/Frame.cc:644-675) + PosInGrid (:1077-1087)
//   Frame::GetFeaturesInArea (src/Frame.cc:1006-1075)
//   ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)
//     (src/ORBmatcher.cc:1962-2178, Nleft == -1 branch) + ComputeThreeMaxima
//   ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, ...)
//     (src/ORBmatcher.cc:44-145, the local-map search)
//   ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
//     (src/ORBmatcher.cc:2180-2300, the relocalization guided search)
//   ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, [vpPointsKFs,]
//     vpMatched, [vpMatchedKF,] th, ratioHamming) (src/ORBmatcher.cc:473-704,
//     the two Sim3-guided searches of loop closing)
// The pose product x3Dc = Rcw*x3Dw + tcw (cv::Mat float gemm) stays with the
// caller (drop-in shim); everything after it runs here.
//
// Grid kernel: one workgroup per frame; (cell << 13 | keypoint) keys sorted in
// LDS, so every cell lists its keypoints in index order as push_back does.
// CSR cell order = mGrid[ix][iy] with cell = ix * 48 + iy, so the cells of one
// grid column inside a search window are one contiguous index range.
//
// Matcher kernel: one workgroup per (CurrentFrame, LastFrame) pair.  The
// greedy assignment is sequential in LastFrame order only through one
// effect: a candidate that received a MapPoint with Observations() > 0 is
// skipped by later points (:2037-2039).  Phase 1 computes every point's best
// candidate in parallel (thread per point, the current frame's keypoints and
// grid in LDS) against the flags on entry; phase 2 walks the points in order
// and re-scans only a point whose best candidate was blocked meanwhile (the
// argmin over a subset that still contains it is unchanged otherwise);
// phase 3 is the rotation histogram filter.
//
// The window clamps, the candidate walk, the per-image LDS arrays, the
// histogram helpers and phase 3 are in grid_search.h; each matcher's scan
// below derives (u, v, radius, levels) and packs what the walk found.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_search.h"
#include "host_stage.h"
#include "plvi_common.h"
#include "plvi_math.h"

namespace plvi {

constexpr int kProjThHigh = 100, kProjHisto = 30;
constexpr int kGridKeyBits = 13;  // keypoint index bits in the grid sort key (cap <= 8192)

__device__ __forceinline__ int round_half_away(float v) { return (int)roundf(v); }

__global__ __launch_bounds__(256) void assign_grid_kernel(const plvi_keypoint* __restrict__ kps,
                                                          const int* __restrict__ counts, int cap, int P,
                                                          plvi_grid_params gp, int* __restrict__ cell_off,
                                                          int* __restrict__ cell_idx) {
    extern __shared__ __align__(16) unsigned s_key[];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[f], cap);
    const plvi_keypoint* K = kps + (size_t)f * cap;
    __shared__ int s_m;
    if (tid == 0) s_m = 0;
    __syncthreads();
    int cm = 0;
    for (int i = tid; i < P; i += 256) {
        unsigned key = 0xFFFFFFFFu;
        if (i < n) {
            // PosInGrid: std::round(float) of (pt - mnMin) * inv
            const int px = round_half_away((K[i].x - gp.min_x) * gp.inv_w);
            const int py = round_half_away((K[i].y - gp.min_y) * gp.inv_h);
            if (!(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows)) {
                key = ((unsigned)(px * kGridRows + py) << kGridKeyBits) | (unsigned)i;
                ++cm;
            }
        }
        s_key[i] = key;
    }
    atomicAdd(&s_m, cm);
    __syncthreads();
    bitonic_sort<256>(s_key, P, tid);
    const int m = s_m;
    int* CO = cell_off + (size_t)f * (kGridCells + 1);
    int* CI = cell_idx + (size_t)f * cap;
    for (int c = tid; c <= kGridCells; c += 256) {  // lower_bound of cell c among the m valid keys
        const unsigned t = (unsigned)c << kGridKeyBits;
        int lo = 0, hi = m;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_key[mid] < t) lo = mid + 1;
            else hi = mid;
        }
        CO[c] = lo;
    }
    for (int j = tid; j < m; j += 256) CI[j] = (int)(s_key[j] & ((1u << kGridKeyBits) - 1));
}

// What a scan returns: (bestDist << 16 | bestIdx2), or
constexpr unsigned kScanSkip = 0xFFFFFFFFu;  // the point is skipped (`continue`d before or at an empty window)
constexpr unsigned kScanNone = 0xFFFFFFFEu;  // window searched, no candidate (bestIdx2 == -1); two-camera scan only

__device__ __forceinline__ unsigned scan_pack(int dist, int idx) { return ((unsigned)dist << 16) | (unsigned)idx; }

// The octave range of SearchByProjection(Frame&, Frame&) (:2028-2035)
__device__ __forceinline__ void proj_levels(const plvi_proj_params& p, int nLastOctave, int& minLevel, int& maxLevel) {
    if (p.forward) { minLevel = nLastOctave; maxLevel = -1; }
    else if (p.backward) { minLevel = 0; maxLevel = nLastOctave; }
    else { minLevel = nLastOctave - 1; maxLevel = nLastOctave + 1; }
}

// GetFeaturesInArea + the candidate loop of SearchByProjection (:1992-2058)
// for LastFrame point i against the blocked flags `blk`.
__device__ unsigned proj_scan(const plvi_proj_params& p, const GridSide& s, const unsigned char* blk, int i,
                              const float* __restrict__ x3dc, const int* __restrict__ loct,
                              const uint8_t* __restrict__ mpdesc, const float* __restrict__ uright) {
    const float xc = x3dc[3 * i], yc = x3dc[3 * i + 1], zc = x3dc[3 * i + 2];
    const float invzc = (float)(1.0 / (double)zc);
    if (invzc < 0) return kScanSkip;
    const float u = p.fx * xc / zc + p.cx, v = p.fy * yc / zc + p.cy;  // Pinhole::project
    if (u < p.min_x || u > p.max_x) return kScanSkip;
    if (v < p.min_y || v > p.max_y) return kScanSkip;
    const int nLastOctave = loct[i];
    if (nLastOctave < 0 || nLastOctave >= p.nlevels) return kScanSkip;  // no scale factor: no candidate
    const float radius = p.th * p.scale_factors[nLastOctave];
    int minLevel, maxLevel;
    proj_levels(p, nLastOctave, minLevel, maxLevel);
    GridWindow w;
    if (!grid_window(p.min_x, p.min_y, p.inv_w, p.inv_h, u, v, radius, w)) return kScanSkip;
    const UrightReject stereo{uright, rfmaf(-p.mbf, invzc, u), radius};  // ur fused in ORBmatcher.cc.o
    BestOne best;
    grid_walk(s, blk, w, u, v, radius, (minLevel > 0) || (maxLevel >= 0), minLevel, maxLevel,
              mpdesc + (size_t)32 * i, stereo, best);
    if (best.idx < 0) return kScanSkip;
    return scan_pack(best.dist, best.idx);
}

__global__ __launch_bounds__(256) void search_by_projection_kernel(
    plvi_proj_params p, const plvi_keypoint* __restrict__ ckps, const uint8_t* __restrict__ cdesc_all,
    const int* __restrict__ cur_n, int cur_cap, const uint8_t* __restrict__ cblocked, const float* __restrict__ curight,
    const int* __restrict__ cell_off_all, const int* __restrict__ cell_idx_all, const float* __restrict__ x3dc_all,
    const int* __restrict__ loct_all, const float* __restrict__ lang_all, const uint8_t* __restrict__ mpdesc_all,
    const uint8_t* __restrict__ lflags_all, const int* __restrict__ last_n, int last_cap, int* __restrict__ match,
    int* __restrict__ nmatches) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const int nl = min(last_n[pr], last_cap);
    GridSide s;
    GridGaps g{{(size_t)(4 * last_cap), (size_t)(4 * last_cap)}, {}};
    unsigned char* q = lds;
    grid_side_load<true, false>(s, q, pr, cur_cap, ckps, cdesc_all, cur_n, cblocked, cell_off_all, cell_idx_all, tid,
                                &g);
    int* best = reinterpret_cast<int*>(g.at[0]);                        // [last_cap]
    unsigned short* ent = reinterpret_cast<unsigned short*>(g.at[1]);  // [last_cap] idx, [last_cap] bin
    __shared__ int s_hist[kProjHisto], s_keep[3], s_ne, s_nm;
    const float* ur = curight ? curight + (size_t)pr * cur_cap : nullptr;
    if (tid < kProjHisto) s_hist[tid] = 0;
    __syncthreads();
    const float* x3dc = x3dc_all + (size_t)pr * last_cap * 3;
    const int* loct = loct_all + (size_t)pr * last_cap;
    const uint8_t* mpdesc = mpdesc_all + (size_t)pr * last_cap * 32;
    const uint8_t* lflags = lflags_all + (size_t)pr * last_cap;
    // phase 1: every point against the flags on entry
    for (int i = tid; i < nl; i += 256)
        best[i] = (lflags[i] & 1) ? (int)proj_scan(p, s, s.pre, i, x3dc, loct, mpdesc, ur) : -1;
    __syncthreads();
    // phase 2: the greedy assignment in LastFrame order (:2060-2083)
    if (tid == 0) {
        const float* lang = lang_all + (size_t)pr * last_cap;
        int nm = 0, ne = 0;
        for (int i = 0; i < nl; ++i) {
            unsigned b = (unsigned)best[i];
            if (b == kScanSkip) continue;
            if (s.blocked[b & 0xFFFFu] != s.pre[b & 0xFFFFu])  // its best was taken meanwhile: re-scan
                b = proj_scan(p, s, s.blocked, i, x3dc, loct, mpdesc, ur);
            if (b == kScanSkip || (int)(b >> 16) > kProjThHigh) continue;
            const int i2 = (int)(b & 0xFFFFu);
            s.assign[i2] = i;
            s.blocked[i2] = (lflags[i] & 2) ? 1 : 0;  // the stored MapPoint's Observations() > 0
            ++nm;
            if (p.check_orientation) {
                const int bin = rot_bin(lang[i] - s.K[i2].angle, kProjHisto);
                ent[last_cap + ne] = (unsigned short)bin;
                ent[ne++] = (unsigned short)i2;
                s_hist[bin]++;
            }
        }
        s_ne = ne;
        s_nm = nm;
        three_maxima(s_hist, kProjHisto, s_keep);
    }
    __syncthreads();
    // phase 3: entries in dropped bins set mvpMapPoints[idx] = NULL (:2164-2174)
    rotation_filter_and_store(s, p.check_orientation, ent, last_cap, s_keep, &s_ne, &s_nm,
                              match + (size_t)pr * cur_cap, nmatches + pr, tid);
}

// ---------------------------------------------------------------------------
// SearchByProjection(CurrentFrame, LastFrame, th, bMono) on a two-camera
// CurrentFrame (CurrentFrame.Nleft != -1, :1985-2153): every LastFrame point
// is projected with CurrentFrame.mpCamera into the left image (x3Dc) and,
// when the left pass did not `continue` (:2000-2026: behind the camera,
// outside the image bounds, empty window), into the right image (x3Dr =
// mTrl * x3Dc, no bounds test, mGridRight); no mvuRight test.  Both
// assignments feed one rotation histogram (right entries at idx + Nleft).
// mpCamera is Pinhole (:30-33) or KannalaBrandt8 (:33-48 of
// CameraModels/KannalaBrandt8.cpp, glibc atan2f / cosf / sinf restated in
// plvi_math.h).  Same schedule as the one-camera kernel, per side.
struct CamModel {
    int kb;  // 0 = Pinhole, 1 = KannalaBrandt8 (k1..k4 below)
    float k0, k1, k2, k3;
};

__device__ __forceinline__ void cam_project(const plvi_proj_params& p, const CamModel& cm, float x, float y, float z,
                                            float& u, float& v) {
    if (!cm.kb) {  // Pinhole::project
        u = p.fx * x / z + p.cx;
        v = p.fy * y / z + p.cy;
        return;
    }
    // KannalaBrandt8::project(const cv::Point3f&); its 7 fused multiply-adds
    // as in KannalaBrandt8.cpp.o (x*x + y*y, the four r terms, u, v)
    const float x2_plus_y2 = rfmaf(x, x, y * y);
    const float theta = plvi::plvi_atan2f(__builtin_sqrtf(x2_plus_y2), z);
    const float psi = plvi::plvi_atan2f(y, x);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = rfmaf(cm.k3, theta9, rfmaf(cm.k2, theta7, rfmaf(cm.k1, theta5, rfmaf(cm.k0, theta3, theta))));
    u = rfmaf(p.fx * r, plvi::plvi_cosf(psi), p.cx);
    v = rfmaf(p.fy * r, plvi::plvi_sinf(psi), p.cy);
}

// GetFeaturesInArea(u, v, radius, levels, bRight) + the candidate loop
// (:2033-2058 / :2109-2125) of point i on one side.  An empty vIndices2
// `continue`s the left pass (kScanSkip) but only ends the right one.
__device__ unsigned proj2_scan(const plvi_proj_params& p, const GridSide& s, const unsigned char* blk, float u, float v,
                               int nLastOctave, const uint8_t* __restrict__ mpd, bool left) {
    const unsigned empty = left ? kScanSkip : kScanNone;
    if (nLastOctave < 0 || nLastOctave >= p.nlevels) return empty;  // no scale factor
    const float radius = p.th * p.scale_factors[nLastOctave];
    int minLevel, maxLevel;
    proj_levels(p, nLastOctave, minLevel, maxLevel);
    GridWindow w;
    if (!grid_window(p.min_x, p.min_y, p.inv_w, p.inv_h, u, v, radius, w)) return empty;
    BestOne best;
    const bool any = grid_walk(s, blk, w, u, v, radius, (minLevel > 0) || (maxLevel >= 0), minLevel, maxLevel, mpd,
                               NoReject{}, best);  // any: vIndices2 non-empty
    if (!any) return empty;
    if (best.idx < 0) return kScanNone;
    return scan_pack(best.dist, best.idx);
}

__global__ __launch_bounds__(256) void search_by_projection2_kernel(
    plvi_proj_params p, CamModel cm, const plvi_keypoint* __restrict__ lkps, const uint8_t* __restrict__ ldesc_all,
    const int* __restrict__ l_n, int l_cap, const uint8_t* __restrict__ lblocked, const int* __restrict__ lcell_off_all,
    const int* __restrict__ lcell_idx_all, const plvi_keypoint* __restrict__ rkps, const uint8_t* __restrict__ rdesc_all,
    const int* __restrict__ r_n, int r_cap, const uint8_t* __restrict__ rblocked, const int* __restrict__ rcell_off_all,
    const int* __restrict__ rcell_idx_all, const float* __restrict__ x3dc_all, const float* __restrict__ x3dr_all,
    const int* __restrict__ loct_all, const float* __restrict__ lang_all, const uint8_t* __restrict__ mpdesc_all,
    const uint8_t* __restrict__ lflags_all, const int* __restrict__ last_n, int last_cap, int* __restrict__ match_l,
    int* __restrict__ match_r, int* __restrict__ nmatches) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const int nl = min(last_n[pr], last_cap);
    GridSide S[2];
    unsigned* best;          // [2][last_cap]
    unsigned short* ent;     // [2 * last_cap] keypoint, [2 * last_cap] bin | side << 15
    {
        unsigned char* q = lds;
        best = reinterpret_cast<unsigned*>(q); q += 8 * (size_t)last_cap;
        ent = reinterpret_cast<unsigned short*>(q); q += 8 * (size_t)last_cap;
        grid_side_load<true, true>(S[0], q, pr, l_cap, lkps, ldesc_all, l_n, lblocked, lcell_off_all, lcell_idx_all,
                                   tid);
        grid_side_load<true, true>(S[1], q, pr, r_cap, rkps, rdesc_all, r_n, rblocked, rcell_off_all, rcell_idx_all,
                                   tid);
    }
    __shared__ int s_hist[kProjHisto], s_keep[3], s_ne, s_nm;
    if (tid < kProjHisto) s_hist[tid] = 0;
    __syncthreads();
    const float* x3dc = x3dc_all + (size_t)pr * last_cap * 3;
    const float* x3dr = x3dr_all + (size_t)pr * last_cap * 3;
    const int* loct = loct_all + (size_t)pr * last_cap;
    const uint8_t* mpdesc = mpdesc_all + (size_t)pr * last_cap * 32;
    const uint8_t* lflags = lflags_all + (size_t)pr * last_cap;
    // the projections of point i (left pass exits: invzc < 0, outside the bounds)
    auto project = [&](int i, float& ul, float& vl, float& ur, float& vr) -> bool {
        const float xc = x3dc[3 * i], yc = x3dc[3 * i + 1], zc = x3dc[3 * i + 2];
        const float invzc = (float)(1.0 / (double)zc);
        if (invzc < 0) return false;
        cam_project(p, cm, xc, yc, zc, ul, vl);
        if (ul < p.min_x || ul > p.max_x) return false;
        if (vl < p.min_y || vl > p.max_y) return false;
        cam_project(p, cm, x3dr[3 * i], x3dr[3 * i + 1], x3dr[3 * i + 2], ur, vr);
        return true;
    };
    // phase 1: both sides of every point against the flags on entry
    for (int i = tid; i < nl; i += 256) {
        unsigned bl = kScanSkip, br = kScanSkip;
        float ul, vl, ur, vr;
        if ((lflags[i] & 1) && project(i, ul, vl, ur, vr)) {
            const uint8_t* mpd = mpdesc + (size_t)32 * i;
            bl = proj2_scan(p, S[0], S[0].pre, ul, vl, loct[i], mpd, true);
            if (bl != kScanSkip) br = proj2_scan(p, S[1], S[1].pre, ur, vr, loct[i], mpd, false);
        }
        best[i] = bl;
        best[last_cap + i] = br;
    }
    __syncthreads();
    // phase 2: LastFrame order, left (:2060-2083) then right (:2127-2148)
    if (tid == 0) {
        const float* lang = lang_all + (size_t)pr * last_cap;
        int nm = 0, ne = 0;
        for (int i = 0; i < nl; ++i) {
            if (best[i] == kScanSkip) continue;
            // a side whose best was taken meanwhile is re-scanned (the sides'
            // flags are separate, so both are known here); one projection for
            // both, and the side loop unrolled: S[c] by constant index stays
            // in registers
            bool stale[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned b = best[c * last_cap + i];
                stale[c] = b != kScanSkip && b != kScanNone && S[c].blocked[b & 0xFFFFu] != S[c].pre[b & 0xFFFFu];
            }
            float ul, vl, ur, vr;
            if (stale[0] || stale[1]) project(i, ul, vl, ur, vr);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                GridSide& A = S[c];
                unsigned b = best[c * last_cap + i];
                if (b == kScanSkip || b == kScanNone) continue;  // no unblocked candidate stays so
                if (stale[c]) {
                    b = proj2_scan(p, A, A.blocked, c ? ur : ul, c ? vr : vl, loct[i], mpdesc + (size_t)32 * i, c == 0);
                    if (b == kScanSkip || b == kScanNone) continue;
                }
                if ((int)(b >> 16) > kProjThHigh) continue;
                const int i2 = (int)(b & 0xFFFFu);
                A.assign[i2] = i;
                A.blocked[i2] = (lflags[i] & 2) ? 1 : 0;  // the stored MapPoint's Observations() > 0
                ++nm;
                if (p.check_orientation) {
                    const int bin = rot_bin(lang[i] - A.K[i2].angle, kProjHisto);
                    ent[2 * last_cap + ne] = (unsigned short)(bin | c << 15);
                    ent[ne++] = (unsigned short)i2;
                    s_hist[bin]++;
                }
            }
        }
        s_ne = ne;
        s_nm = nm;
        three_maxima(s_hist, kProjHisto, s_keep);
    }
    __syncthreads();
    // phase 3: entries in dropped bins set mvpMapPoints[idx] = NULL (:2155-2175)
    if (p.check_orientation) {
        const int ne = s_ne;
        int dropped = 0;
        for (int e = tid; e < ne; e += 256) {
            const int code = ent[2 * last_cap + e], bin = code & 0x7FFF;
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) {
                unsigned char* nulled = (code >> 15) ? S[1].nulled : S[0].nulled;
                nulled[ent[e]] = 1;
                ++dropped;
            }
        }
        if (dropped) atomicSub(&s_nm, dropped);
        __syncthreads();
    }
    int* ML = match_l + (size_t)pr * l_cap;
    int* MR = match_r + (size_t)pr * r_cap;
    for (int i = tid; i < S[0].n; i += 256) ML[i] = S[0].nulled[i] ? -2 : S[0].assign[i];
    for (int i = tid; i < S[1].n; i += 256) MR[i] = S[1].nulled[i] ? -2 : S[1].assign[i];
    if (tid == 0) nmatches[pr] = s_nm;
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th,
// bFarPoints, thFarPoints) (src/ORBmatcher.cc:44-145, F.Nleft == -1): the
// local-map search of Tracking::SearchLocalPoints (Tracking.cc:5119/5211).
// Same schedule as above: phase 1 scans every MapPoint's window in parallel
// against the flags on entry and keeps its best and second candidate
// (first argmin, then first argmin of the rest -- the scan order of
// GetFeaturesInArea); phase 2 walks the MapPoints in vector order and
// re-scans only one whose best or second candidate was blocked meanwhile
// (removing any other candidate leaves both unchanged), then applies the
// level-aware ratio test and the assignment.
// fbit: the MapPoint flag that enables this scan; use_th: the radius is
// scaled by th (the left camera's branch only, :69-70 -- not :148)
__device__ void local_scan(const plvi_local_params& p, const GridSide& s, const unsigned char* blk, int m,
                           const unsigned char* __restrict__ fl, const float* __restrict__ proj,
                           const int* __restrict__ lvl, const uint8_t* __restrict__ mpdesc,
                           const float* __restrict__ uright, unsigned* b1, unsigned* b2, unsigned char fbit = 1,
                           bool use_th = true) {
    *b1 = *b2 = kScanSkip;
    if (!(fl[m] & fbit)) return;
    const float x = proj[4 * m], y = proj[4 * m + 1], xr = proj[4 * m + 2], vcos = proj[4 * m + 3];
    const int L = lvl[m];
    if (L < 0 || L >= p.nlevels) return;  // no scale factor for that level: no candidate
    float r = vcos > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos (:216-222)
    if (use_th && p.th != 1.0) r *= p.th;
    const float radius = r * p.scale_factors[L];
    const int minLevel = L - 1, maxLevel = L;
    GridWindow w;
    if (!grid_window(p.min_x, p.min_y, p.inv_w, p.inv_h, x, y, radius, w)) return;
    BestTwo best;
    grid_walk(s, blk, w, x, y, radius, (minLevel > 0) || (maxLevel >= 0), minLevel, maxLevel,
              mpdesc + (size_t)32 * m, UrightReject{uright, xr, radius}, best);
    if (best.idx < 0) return;
    *b1 = scan_pack(best.dist, best.idx);
    if (best.idx2 >= 0) *b2 = scan_pack(best.dist2, best.idx2);
}

__global__ __launch_bounds__(256) void search_local_kernel(
    plvi_local_params p, const plvi_keypoint* __restrict__ ckps, const uint8_t* __restrict__ cdesc_all,
    const int* __restrict__ cur_n, int cur_cap, const uint8_t* __restrict__ cblocked, const float* __restrict__ curight,
    const int* __restrict__ cell_off_all, const int* __restrict__ cell_idx_all, const uint8_t* __restrict__ flags_all,
    const float* __restrict__ proj_all, const int* __restrict__ level_all, const uint8_t* __restrict__ mpdesc_all,
    const int* __restrict__ mp_n, int mp_cap, int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int fr = blockIdx.x, tid = threadIdx.x;
    const int nm = min(mp_n[fr], mp_cap);
    GridSide s;
    GridGaps g{{(size_t)(8 * mp_cap), 0}, {}};
    unsigned char* q = lds;
    grid_side_load<false, false>(s, q, fr, cur_cap, ckps, cdesc_all, cur_n, cblocked, cell_off_all, cell_idx_all, tid,
                                 &g);
    unsigned* best1 = reinterpret_cast<unsigned*>(g.at[0]);  // [mp_cap]
    unsigned* best2 = best1 + mp_cap;                        // [mp_cap]
    const float* ur = curight ? curight + (size_t)fr * cur_cap : nullptr;
    __syncthreads();
    const unsigned char* fl = flags_all + (size_t)fr * mp_cap;
    const float* proj = proj_all + (size_t)fr * mp_cap * 4;
    const int* lvl = level_all + (size_t)fr * mp_cap;
    const uint8_t* mpdesc = mpdesc_all + (size_t)fr * mp_cap * 32;
    // phase 1: every MapPoint against the flags on entry
    for (int m = tid; m < nm; m += 256) local_scan(p, s, s.pre, m, fl, proj, lvl, mpdesc, ur, &best1[m], &best2[m]);
    __syncthreads();
    // phase 2: the assignment in vpMapPoints order (:98-117)
    if (tid == 0) {
        int nmt = 0;
        for (int m = 0; m < nm; ++m) {
            unsigned b1 = best1[m], b2 = best2[m];
            if (b1 == kScanSkip) continue;
            const int i1 = (int)(b1 & 0xFFFFu), i2 = b2 == kScanSkip ? -1 : (int)(b2 & 0xFFFFu);
            if (s.blocked[i1] != s.pre[i1] || (i2 >= 0 && s.blocked[i2] != s.pre[i2])) {
                local_scan(p, s, s.blocked, m, fl, proj, lvl, mpdesc, ur, &b1, &b2);  // blocked meanwhile
                if (b1 == kScanSkip) continue;
            }
            const int bestDist = (int)(b1 >> 16), bestIdx = (int)(b1 & 0xFFFFu);
            const int bestDist2 = b2 == kScanSkip ? 256 : (int)(b2 >> 16);
            const int bestLevel = s.koct[bestIdx], bestLevel2 = b2 == kScanSkip ? -1 : s.koct[b2 & 0xFFFFu];
            if (bestDist <= kProjThHigh) {
                if (bestLevel == bestLevel2 && bestDist > p.nnratio * bestDist2) continue;
                if (bestLevel != bestLevel2 || bestDist <= p.nnratio * bestDist2) {
                    s.assign[bestIdx] = m;
                    s.blocked[bestIdx] = (fl[m] & 2) ? 1 : 0;  // the stored MapPoint's Observations() > 0
                    ++nmt;
                }
            }
        }
        nmatches[fr] = nmt;
    }
    __syncthreads();
    int* M = match + (size_t)fr * cur_cap;
    for (int i = tid; i < s.n; i += 256) M[i] = s.assign[i];
}

// ---------------------------------------------------------------------------
// The same search on a two-camera Frame (F.Nleft != -1: the KannalaBrandt8
// stereo rigs, ORBmatcher.cc:44-214).  Left keypoints mvKeys [0, Nleft) with
// grid mGrid, right keypoints mvKeysRight with mGridRight (right-relative
// indices, Frame.cc:661-674); a MapPoint is searched in the left image when
// mbTrackInView (flag bit0) and in the right image when mbTrackInViewR (bit2)
// -- the right radius is not scaled by th (:148) and there is no mvuRight
// test.  Assignments follow the stereo pairs: a left match also stores the
// MapPoint at mvLeftToRightMatch[idx] + Nleft (:132-136), a right match at
// mvRightToLeftMatch[idx] (:199-203), and both block those keypoints for the
// later MapPoints.  A left ratio-test failure skips the MapPoint's right
// search too (the `continue` at :127).  Same schedule: phase 1 scans both
// sides of every MapPoint in parallel against the entry flags, phase 2 walks
// the MapPoints in order, left then right, re-scanning a side whose best or
// second candidate was blocked meanwhile.
__global__ __launch_bounds__(256) void search_local2_kernel(
    plvi_local_params p, const plvi_keypoint* __restrict__ lkps, const uint8_t* __restrict__ ldesc_all,
    const int* __restrict__ l_n, int l_cap, const uint8_t* __restrict__ lblocked, const int* __restrict__ l2r_all,
    const int* __restrict__ lcell_off_all, const int* __restrict__ lcell_idx_all, const plvi_keypoint* __restrict__ rkps,
    const uint8_t* __restrict__ rdesc_all, const int* __restrict__ r_n, int r_cap, const uint8_t* __restrict__ rblocked,
    const int* __restrict__ r2l_all, const int* __restrict__ rcell_off_all, const int* __restrict__ rcell_idx_all,
    const uint8_t* __restrict__ flags_all, const float* __restrict__ proj_all, const int* __restrict__ level_all,
    const float* __restrict__ projr_all, const int* __restrict__ levelr_all, const uint8_t* __restrict__ mpdesc_all,
    const int* __restrict__ mp_n, int mp_cap, int* __restrict__ match_l, int* __restrict__ match_r,
    int* __restrict__ nmatches) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int fr = blockIdx.x, tid = threadIdx.x;
    const int nm = min(mp_n[fr], mp_cap);
    GridSide S[2];
    // mvLeftToRightMatch / mvRightToLeftMatch (NULL = none)
    const int* pair[2] = {l2r_all ? l2r_all + (size_t)fr * l_cap : nullptr,
                          r2l_all ? r2l_all + (size_t)fr * r_cap : nullptr};
    unsigned* best;  // [4][mp_cap]: left best / second, right best / second
    {
        unsigned char* q = lds;
        best = reinterpret_cast<unsigned*>(q); q += 16 * (size_t)mp_cap;
        grid_side_load<false, false>(S[0], q, fr, l_cap, lkps, ldesc_all, l_n, lblocked, lcell_off_all, lcell_idx_all,
                                     tid);
        grid_side_load<false, false>(S[1], q, fr, r_cap, rkps, rdesc_all, r_n, rblocked, rcell_off_all, rcell_idx_all,
                                     tid);
    }
    __syncthreads();
    const unsigned char* fl = flags_all + (size_t)fr * mp_cap;
    const float* proj[2] = {proj_all + (size_t)fr * mp_cap * 4, projr_all + (size_t)fr * mp_cap * 4};
    const int* lvl[2] = {level_all + (size_t)fr * mp_cap, levelr_all + (size_t)fr * mp_cap};
    const uint8_t* mpdesc = mpdesc_all + (size_t)fr * mp_cap * 32;
    const unsigned char fbit[2] = {1, 4};
    // phase 1: both sides of every MapPoint against the flags on entry
    for (int m = tid; m < nm; m += 256)
        for (int c = 0; c < 2; ++c)
            local_scan(p, S[c], S[c].pre, m, fl, proj[c], lvl[c], mpdesc, nullptr, &best[(2 * c) * mp_cap + m],
                       &best[(2 * c + 1) * mp_cap + m], fbit[c], c == 0);
    __syncthreads();
    // phase 2: vpMapPoints order, left (:62-143) then right (:145-211)
    // A stereo partner is overwritten unchecked (:133, :200), so a keypoint
    // blocked on entry can become a candidate again (stored MapPoint without
    // observations): from then on every scan of that image is redone (rare).
    if (tid == 0) {
        int nmt = 0;
        bool unblocked[2] = {false, false};
        for (int m = 0; m < nm; ++m) {
            const unsigned char obs = (fl[m] & 2) ? 1 : 0;  // the stored MapPoint's Observations() > 0
            for (int c = 0; c < 2; ++c) {
                GridSide& A = S[c];
                GridSide& B = S[1 - c];
                unsigned b1 = best[(2 * c) * mp_cap + m], b2 = best[(2 * c + 1) * mp_cap + m];
                if (b1 == kScanSkip && !unblocked[c]) continue;
                const int i1 = (int)(b1 & 0xFFFFu), i2 = b2 == kScanSkip ? -1 : (int)(b2 & 0xFFFFu);
                if (unblocked[c] || A.blocked[i1] != A.pre[i1] || (i2 >= 0 && A.blocked[i2] != A.pre[i2])) {
                    local_scan(p, A, A.blocked, m, fl, proj[c], lvl[c], mpdesc, nullptr, &b1, &b2, fbit[c],
                               c == 0);  // blocked meanwhile
                    if (b1 == kScanSkip) continue;
                }
                const int bestDist = (int)(b1 >> 16), bestIdx = (int)(b1 & 0xFFFFu);
                const int bestDist2 = b2 == kScanSkip ? 256 : (int)(b2 >> 16);
                const int bestLevel = A.koct[bestIdx], bestLevel2 = b2 == kScanSkip ? -1 : A.koct[b2 & 0xFFFFu];
                if (bestDist > kProjThHigh) continue;
                if (bestLevel == bestLevel2 && bestDist > p.nnratio * bestDist2) break;  // :127 / :197: next MapPoint
                A.assign[bestIdx] = m;
                A.blocked[bestIdx] = obs;
                ++nmt;
                const int o = pair[c] ? pair[c][bestIdx] : -1;
                if (o >= 0 && o < B.n) {  // the stereo observation in the other image
                    B.assign[o] = m;
                    if (B.blocked[o] && !obs) unblocked[1 - c] = true;
                    B.blocked[o] = obs;
                    ++nmt;
                }
            }
        }
        nmatches[fr] = nmt;
    }
    __syncthreads();
    int* ML = match_l + (size_t)fr * l_cap;
    int* MR = match_r + (size_t)fr * r_cap;
    for (int i = tid; i < S[0].n; i += 256) ML[i] = S[0].assign[i];
    for (int i = tid; i < S[1].n; i += 256) MR[i] = S[1].assign[i];
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF,
// const set<MapPoint*>& sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2180-2300),
// the relocalization guided search (Tracking.cc:5857, 5871).  Same schedule as
// the frame-to-frame matcher: phase 1 finds every KF MapPoint's best candidate
// in parallel against the NULL / non-NULL mvpMapPoints on entry; phase 2
// walks the MapPoints in KF order -- every assignment blocks its keypoint for
// the later points (:2240-2242), so a point whose best was taken meanwhile is
// re-scanned -- and phase 3 is the rotation filter.
__device__ unsigned reloc_scan(const plvi_reloc_params& p, const GridSide& s, const unsigned char* blk, int i,
                               const float* __restrict__ x3dc, const float* __restrict__ dist,
                               const int* __restrict__ lvl, const uint8_t* __restrict__ mpdesc) {
    const float xc = x3dc[3 * i], yc = x3dc[3 * i + 1], zc = x3dc[3 * i + 2];
    const float u = p.fx * xc / zc + p.cx, v = p.fy * yc / zc + p.cy;  // Pinhole::project (no depth test here)
    if (u < p.min_x || u > p.max_x) return kScanSkip;
    if (v < p.min_y || v > p.max_y) return kScanSkip;
    const float dist3D = dist[3 * i], minDistance = dist[3 * i + 1], maxDistance = dist[3 * i + 2];
    if (dist3D < minDistance || dist3D > maxDistance) return kScanSkip;
    const int L = lvl[i];
    if (L < 0 || L >= p.nlevels) return kScanSkip;  // PredictScale clamps to [0, mnScaleLevels)
    const float radius = p.th * p.scale_factors[L];
    GridWindow w;
    if (!grid_window(p.min_x, p.min_y, p.inv_w, p.inv_h, u, v, radius, w)) return kScanSkip;
    BestOne best;
    grid_walk(s, blk, w, u, v, radius, true, L - 1, L + 1, mpdesc + (size_t)32 * i, NoReject{},
              best);  // bCheckLevels holds: maxLevel >= 0
    if (best.idx < 0) return kScanSkip;
    return scan_pack(best.dist, best.idx);
}

__global__ __launch_bounds__(256) void search_reloc_kernel(
    plvi_reloc_params p, const plvi_keypoint* __restrict__ ckps, const uint8_t* __restrict__ cdesc_all,
    const int* __restrict__ cur_n, int cur_cap, const uint8_t* __restrict__ cblocked,
    const int* __restrict__ cell_off_all, const int* __restrict__ cell_idx_all, const uint8_t* __restrict__ kflags_all,
    const float* __restrict__ x3dc_all, const float* __restrict__ dist_all, const int* __restrict__ lvl_all,
    const float* __restrict__ kang_all, const uint8_t* __restrict__ mpdesc_all, const int* __restrict__ kf_n,
    int kf_cap, int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const int nk = min(kf_n[pr], kf_cap);
    GridSide s;
    GridGaps g{{(size_t)(4 * kf_cap), (size_t)(4 * kf_cap)}, {}};
    unsigned char* q = lds;
    grid_side_load<true, true>(s, q, pr, cur_cap, ckps, cdesc_all, cur_n, cblocked, cell_off_all, cell_idx_all, tid,
                               &g);
    int* best = reinterpret_cast<int*>(g.at[0]);                        // [kf_cap]
    unsigned short* ent = reinterpret_cast<unsigned short*>(g.at[1]);  // [kf_cap] idx, [kf_cap] bin
    __shared__ int s_hist[kProjHisto], s_keep[3], s_ne, s_nm;
    if (tid < kProjHisto) s_hist[tid] = 0;
    __syncthreads();
    const float* x3dc = x3dc_all + (size_t)pr * kf_cap * 3;
    const float* dist = dist_all + (size_t)pr * kf_cap * 3;
    const int* lvl = lvl_all + (size_t)pr * kf_cap;
    const uint8_t* mpdesc = mpdesc_all + (size_t)pr * kf_cap * 32;
    const uint8_t* kfl = kflags_all + (size_t)pr * kf_cap;
    // phase 1: every KF MapPoint against mvpMapPoints on entry
    for (int i = tid; i < nk; i += 256)
        best[i] = (kfl[i] & 1) ? (int)reloc_scan(p, s, s.pre, i, x3dc, dist, lvl, mpdesc) : -1;
    __syncthreads();
    // phase 2: the assignment in KF order (:2260-2277)
    if (tid == 0) {
        const float* kang = kang_all + (size_t)pr * kf_cap;
        int nm = 0, ne = 0;
        for (int i = 0; i < nk; ++i) {
            unsigned b = (unsigned)best[i];
            if (b == kScanSkip) continue;
            if (s.blocked[b & 0xFFFFu] != s.pre[b & 0xFFFFu])  // its best was taken meanwhile: re-scan
                b = reloc_scan(p, s, s.blocked, i, x3dc, dist, lvl, mpdesc);
            if (b == kScanSkip || (int)(b >> 16) > p.orb_dist) continue;
            const int i2 = (int)(b & 0xFFFFu);
            s.assign[i2] = i;
            s.blocked[i2] = 1;
            ++nm;
            if (p.check_orientation) {
                const int bin = rot_bin(kang[i] - s.K[i2].angle, kProjHisto);
                ent[kf_cap + ne] = (unsigned short)bin;
                ent[ne++] = (unsigned short)i2;
                s_hist[bin]++;
            }
        }
        s_ne = ne;
        s_nm = nm;
        three_maxima(s_hist, kProjHisto, s_keep);
    }
    __syncthreads();
    // phase 3: entries in dropped bins set mvpMapPoints[idx] = NULL (:2284-2296)
    rotation_filter_and_store(s, p.check_orientation, ent, kf_cap, s_keep, &s_ne, &s_nm, match + (size_t)pr * cur_cap,
                              nmatches + pr, tid);
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints,
// vpMatched, th, ratioHamming) (src/ORBmatcher.cc:473-586) and the overload
// with vpPointsKFs / vpMatchedKF (:588-704), the loop-closing guided searches
// (LoopClosing.cc:954, :1207 and :929).  The greedy two-phase schedule of the
// relocalization matcher without a rotation filter: phase 1 finds every
// point's best keypoint in parallel against vpMatched on entry; phase 2 walks
// the points in order -- every assignment blocks its keypoint for the later
// points (:558 / :675), so a point whose best was taken meanwhile is
// re-scanned.  The two overloads differ in the projection only: :519 calls
// Pinhole::project ((fx*x)/z + cx, no fused operation), :631-636 multiply by
// 1/z and the reference object fuses fx*x + cx and fy*y + cy.
__device__ unsigned sim3_scan(const plvi_sim3_proj_params& p, const GridSide& s, const unsigned char* blk, int i,
                              const float* __restrict__ x3dc, const float* __restrict__ dist,
                              const double* __restrict__ dot, const int* __restrict__ lvl,
                              const uint8_t* __restrict__ mpdesc) {
    const float xc = x3dc[3 * (size_t)i], yc = x3dc[3 * (size_t)i + 1], zc = x3dc[3 * (size_t)i + 2];
    if (zc < 0.0f) return kScanSkip;  // depth must be positive (:511 / :627)
    float u, v;
    if (p.projection) {
        const float invz = 1 / zc;
        const float x = xc * invz, y = yc * invz;
        u = rfmaf(x, p.fx, p.cx);
        v = rfmaf(y, p.fy, p.cy);
    } else {
        u = p.fx * xc / zc + p.cx;
        v = p.fy * yc / zc + p.cy;
    }
    // KeyFrame::IsInImage (KeyFrame.cc:1246-1249): the upper bounds are strict
    if (!(u >= p.min_x && u < p.max_x && v >= p.min_y && v < p.max_y)) return kScanSkip;
    const float d3 = dist[3 * (size_t)i], minDistance = dist[3 * (size_t)i + 1], maxDistance = dist[3 * (size_t)i + 2];
    if (d3 < minDistance || d3 > maxDistance) return kScanSkip;
    if (dot[i] < 0.5 * (double)d3) return kScanSkip;  // viewing angle (:537 / :654), a double compare
    const int L = lvl[i];
    if (L < 0 || L >= p.nlevels) return kScanSkip;  // PredictScale clamps to [0, mnScaleLevels)
    const float radius = (float)p.th * p.scale_factors[L];
    GridWindow w;
    if (!grid_window(p.min_x, p.min_y, p.inv_w, p.inv_h, u, v, radius, w)) return kScanSkip;
    BestOne best;
    // kpLevel < L-1 || kpLevel > L (:563 / :680); KeyFrame::GetFeaturesInArea itself has no level filter
    grid_walk(s, blk, w, u, v, radius, true, L - 1, L, mpdesc + (size_t)32 * i, NoReject{}, best);
    if (best.idx < 0) return kScanSkip;
    return scan_pack(best.dist, best.idx);
}

__global__ __launch_bounds__(256) void search_sim3_proj_kernel(
    plvi_sim3_proj_params p, const plvi_keypoint* __restrict__ kps_all, const uint8_t* __restrict__ desc_all,
    const int* __restrict__ kp_n, int kp_cap, const uint8_t* __restrict__ matched_all,
    const int* __restrict__ cell_off_all, const int* __restrict__ cell_idx_all, const uint8_t* __restrict__ flags_all,
    const float* __restrict__ x3dc_all, const float* __restrict__ dist_all, const double* __restrict__ dot_all,
    const int* __restrict__ lvl_all, const uint8_t* __restrict__ mpdesc_all, const int* __restrict__ pt_n, int pt_cap,
    int* __restrict__ match, int* __restrict__ nmatches) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const int np = max(min(pt_n[pr], pt_cap), 0);
    GridSide s;
    GridGaps g{{(size_t)4 * pt_cap, 0}, {}};
    unsigned char* q = lds;
    grid_side_load<false, true>(s, q, pr, kp_cap, kps_all, desc_all, kp_n, matched_all, cell_off_all, cell_idx_all, tid,
                                &g);
    unsigned* best = reinterpret_cast<unsigned*>(g.at[0]);  // [pt_cap]
    __syncthreads();
    const float* x3dc = x3dc_all + (size_t)pr * pt_cap * 3;
    const float* dist = dist_all + (size_t)pr * pt_cap * 3;
    const double* dot = dot_all + (size_t)pr * pt_cap;
    const int* lvl = lvl_all + (size_t)pr * pt_cap;
    const uint8_t* mpdesc = mpdesc_all + (size_t)pr * pt_cap * 32;
    const uint8_t* fl = flags_all + (size_t)pr * pt_cap;
    // phase 1: every point against vpMatched on entry
    for (int i = tid; i < np; i += 256)
        best[i] = (fl[i] & 1) ? sim3_scan(p, s, s.pre, i, x3dc, dist, dot, lvl, mpdesc) : kScanSkip;
    __syncthreads();
    // phase 2: the assignment in vpPoints order (:577-581 / :694-699)
    if (tid == 0) {
        const float thr = 50.0f * p.ratio_hamming;  // TH_LOW * ratioHamming, a float product
        int nm = 0;
        for (int i = 0; i < np; ++i) {
            unsigned b = best[i];
            if (b == kScanSkip) continue;
            if (s.blocked[b & 0xFFFFu] != s.pre[b & 0xFFFFu])  // its best was taken meanwhile: re-scan
                b = sim3_scan(p, s, s.blocked, i, x3dc, dist, dot, lvl, mpdesc);
            if (b == kScanSkip || thr < (float)(int)(b >> 16)) continue;  // bestDist <= thr, as the object compares
            const int i2 = (int)(b & 0xFFFFu);
            s.assign[i2] = i;
            s.blocked[i2] = 1;
            ++nm;
        }
        nmatches[pr] = nm;
    }
    __syncthreads();
    int* M = match + (size_t)pr * kp_cap;
    for (int i = tid; i < s.n; i += 256) M[i] = s.assign[i];
}

// Dynamic LDS of the kernels above: grid_side_load's arrays per image (with
// or without `nulled`), the per-point tables, 64 bytes of slack.
static size_t side_smem(int cap, bool nulled) {
    return (size_t)cap * (4 + 4 + 4 + 2 + 1 + 1 + 1 + (nulled ? 1 : 0)) + 4 * (kGridCells + 1);
}
static size_t align16(size_t n) { return (n + 15) & ~size_t(15); }

static size_t local_smem(int cur_cap, int mp_cap) { return side_smem(cur_cap, false) + (size_t)mp_cap * 8 + 64; }

static size_t local2_smem(int l_cap, int r_cap, int mp_cap) {
    return 16 * (size_t)mp_cap + align16(side_smem(l_cap, false)) + align16(side_smem(r_cap, false)) + 64;
}

static size_t proj2_smem(int l_cap, int r_cap, int last_cap) {
    return 16 * (size_t)last_cap + align16(side_smem(l_cap, true)) + align16(side_smem(r_cap, true)) + 64;
}

static size_t proj_smem(int cur_cap, int last_cap) {
    return side_smem(cur_cap, true) + (size_t)last_cap * (4 + 4) + 64;
}

static size_t sim3_smem(int kp_cap, int pt_cap) { return side_smem(kp_cap, false) + (size_t)pt_cap * 4 + 64; }

}  // namespace plvi

using namespace plvi;

extern "C" int plvi_assign_grid_batch(const plvi_keypoint* d_kps, const int* d_count, int cap, int n_frames,
                                      const plvi_grid_params* gp, int* d_cell_off, int* d_cell_idx, void* stream) {
    if (!gp || cap < 1 || cap > (1 << kGridKeyBits) || n_frames < 0) return PLVI_E_BADARG;
    if (n_frames == 0) return PLVI_OK;
    const int P = pow2_at_least(cap, 256);
    return launch_lds<assign_grid_kernel>(
        dim3(n_frames), dim3(256), (size_t)4 * P, (hipStream_t)stream, d_kps, d_count, cap, P, *gp, d_cell_off,
        d_cell_idx);
}

// One staged image: keypoints, descriptors, the blocked flags (NULL: none) and
// the slots of its grid.
struct StagedImage {
    Staged<plvi_keypoint> k;
    Staged<uint8_t> d, b;
    Staged<int> co, ci;
};

static StagedImage stage_image(HostStage& st, const plvi_keypoint* kps, const uint8_t* desc, const uint8_t* blocked,
                               int n, int cap) {
    return {st.in_or_zero(kps, n), st.in_or_zero(desc, n, 32), st.in_or_zero(blocked, n),
            st.scratch<int>(kGridCells + 1), st.scratch<int>(cap)};
}

// The grid of a staged image (count at d_n), with the matcher's own image bounds.
template <class Params>
static int stage_grid(const HostStage& st, const Params* p, const StagedImage& im, const int* d_n, int cap) {
    const plvi_grid_params gp{p->min_x, p->min_y, p->inv_w, p->inv_h};
    return plvi_assign_grid_batch(st.dev(im.k), d_n, cap, 1, &gp, st.dev(im.co), st.dev(im.ci), nullptr);
}

extern "C" int plvi_search_by_projection_batch(int n_pairs, const plvi_proj_params* p, const plvi_keypoint* d_cur_kps,
                                               const uint8_t* d_cur_desc, const int* d_cur_n, int cur_cap,
                                               const uint8_t* d_cur_blocked, const float* d_cur_uright,
                                               const int* d_cell_off, const int* d_cell_idx, const float* d_x3dc,
                                               const int* d_last_octave, const float* d_last_angle,
                                               const uint8_t* d_mp_desc, const uint8_t* d_last_flags,
                                               const int* d_last_n, int last_cap, int* d_match, int* d_nmatches,
                                               void* stream) {
    if (!p || n_pairs < 0 || cur_cap < 1 || last_cap < 1 || cur_cap > 65535 || last_cap > 65535) return PLVI_E_BADARG;
    if (p->nlevels < 1 || p->nlevels > 16) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    return launch_lds<search_by_projection_kernel>(
        dim3(n_pairs), dim3(256), proj_smem(cur_cap, last_cap), (hipStream_t)stream, *p, d_cur_kps, d_cur_desc,
        d_cur_n, cur_cap, d_cur_blocked, d_cur_uright, d_cell_off, d_cell_idx, d_x3dc, d_last_octave, d_last_angle,
        d_mp_desc, d_last_flags, d_last_n, last_cap, d_match, d_nmatches);
}

// One pair from host memory, synchronous (grid built on the device too).
// Returns nmatches (>= 0) or an error.
extern "C" int plvi_search_by_projection(const plvi_proj_params* p, const plvi_keypoint* cur_kps,
                                         const uint8_t* cur_desc, int n_cur, const uint8_t* cur_blocked,
                                         const float* cur_uright, const float* x3dc, const int* last_octave,
                                         const float* last_angle, const uint8_t* mp_desc, const uint8_t* last_flags,
                                         int n_last, int* match) {
    if (!p || n_cur < 0 || n_last < 0 || (n_cur > 0 && (!cur_kps || !cur_desc || !match))) return PLVI_E_BADARG;
    if (n_cur == 0) return 0;
    const int cc = n_cur, lc = std::max(n_last, 1);
    int counts[3] = {n_cur, n_last, 0};  // [2]: nmatches
    HostStage st;
    const StagedImage im = stage_image(st, cur_kps, cur_desc, cur_blocked, n_cur, cc);
    const auto U = st.in(cur_uright, cc), X = st.in_or_zero(x3dc, n_last, 3), LA = st.in_or_zero(last_angle, n_last);
    const auto MD = st.in_or_zero(mp_desc, n_last, 32), LF = st.in_or_zero(last_flags, n_last);
    const auto LO = st.in_or_zero(last_octave, n_last), M = st.out(match, cc), N = st.inout(counts, 3);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = stage_grid(st, p, im, dN, cc)) return rc;
    if (int rc = plvi_search_by_projection_batch(1, p, st.dev(im.k), st.dev(im.d), dN, cc, st.dev(im.b), st.dev(U),
                                                 st.dev(im.co), st.dev(im.ci), st.dev(X), st.dev(LO), st.dev(LA),
                                                 st.dev(MD), st.dev(LF), dN + 1, lc, st.dev(M), dN + 2, nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[2];
}

extern "C" int plvi_search_reloc_batch(int n_pairs, const plvi_reloc_params* p, const plvi_keypoint* d_cur_kps,
                                       const uint8_t* d_cur_desc, const int* d_cur_n, int cur_cap,
                                       const uint8_t* d_cur_blocked, const int* d_cell_off, const int* d_cell_idx,
                                       const uint8_t* d_kf_flags, const float* d_x3dc, const float* d_dist,
                                       const int* d_level, const float* d_kf_angle, const uint8_t* d_mp_desc,
                                       const int* d_kf_n, int kf_cap, int* d_match, int* d_nmatches, void* stream) {
    if (!p || n_pairs < 0 || cur_cap < 1 || kf_cap < 1 || cur_cap > 65535 || kf_cap > 65535) return PLVI_E_BADARG;
    if (p->nlevels < 1 || p->nlevels > 16 || p->orb_dist < 0 || p->orb_dist > 255) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    // same carve-up as the frame-to-frame matcher
    return launch_lds<search_reloc_kernel>(
        dim3(n_pairs), dim3(256), proj_smem(cur_cap, kf_cap), (hipStream_t)stream, *p, d_cur_kps, d_cur_desc, d_cur_n,
        cur_cap, d_cur_blocked, d_cell_off, d_cell_idx, d_kf_flags, d_x3dc, d_dist, d_level, d_kf_angle, d_mp_desc,
        d_kf_n, kf_cap, d_match, d_nmatches);
}

// One pair from host memory, synchronous (grid built on the device).
extern "C" int plvi_search_reloc(const plvi_reloc_params* p, const plvi_keypoint* cur_kps, const uint8_t* cur_desc,
                                 int n_cur, const uint8_t* cur_blocked, const uint8_t* kf_flags, const float* x3dc,
                                 const float* dist, const int* level, const float* kf_angle, const uint8_t* mp_desc,
                                 int n_kf, int* match) {
    if (!p || n_cur < 0 || n_kf < 0 || (n_cur > 0 && (!cur_kps || !cur_desc || !match))) return PLVI_E_BADARG;
    if (n_kf > 0 && (!kf_flags || !x3dc || !dist || !level || !kf_angle || !mp_desc)) return PLVI_E_BADARG;
    if (p->nlevels < 1 || p->nlevels > 16 || p->orb_dist < 0 || p->orb_dist > 255) return PLVI_E_BADARG;
    if (n_cur == 0) return 0;
    const int cc = n_cur, kc = std::max(n_kf, 1);
    int counts[3] = {n_cur, n_kf, 0};  // [2]: nmatches
    HostStage st;
    const StagedImage im = stage_image(st, cur_kps, cur_desc, cur_blocked, n_cur, cc);
    const auto X = st.in_or_zero(x3dc, n_kf, 3), S = st.in_or_zero(dist, n_kf, 3), A = st.in_or_zero(kf_angle, n_kf);
    const auto F = st.in_or_zero(kf_flags, n_kf), MD = st.in_or_zero(mp_desc, n_kf, 32);
    const auto L = st.in_or_zero(level, n_kf), M = st.out(match, cc), N = st.inout(counts, 3);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = stage_grid(st, p, im, dN, cc)) return rc;
    if (int rc = plvi_search_reloc_batch(1, p, st.dev(im.k), st.dev(im.d), dN, cc, st.dev(im.b), st.dev(im.co),
                                         st.dev(im.ci), st.dev(F), st.dev(X), st.dev(S), st.dev(L), st.dev(A),
                                         st.dev(MD), dN + 1, kc, st.dev(M), dN + 2, nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[2];
}

// 50 * ratioHamming >= 256 would accept the bestDist = 256 of a search without
// a candidate and index vpMatched[-1] in the reference (NaN refused too)
static bool sim3_params_ok(const plvi_sim3_proj_params* p) {
    return p && p->nlevels >= 1 && p->nlevels <= 16 && (p->projection == 0 || p->projection == 1) &&
           50.0f * p->ratio_hamming < 256.0f;
}

extern "C" int plvi_search_sim3_projection_batch(int n_pairs, const plvi_sim3_proj_params* p,
                                                 const plvi_keypoint* d_kps, const uint8_t* d_desc, const int* d_kp_n,
                                                 int kp_cap, const uint8_t* d_matched, const int* d_cell_off,
                                                 const int* d_cell_idx, const uint8_t* d_flags, const float* d_x3dc,
                                                 const float* d_dist, const double* d_dot, const int* d_level,
                                                 const uint8_t* d_mp_desc, const int* d_pt_n, int pt_cap, int* d_match,
                                                 int* d_nmatches, void* stream) {
    if (!sim3_params_ok(p) || n_pairs < 0 || kp_cap < 1 || pt_cap < 1 || kp_cap > 65535) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    if (!d_kps || !d_desc || !d_kp_n || !d_cell_off || !d_cell_idx || !d_flags || !d_x3dc || !d_dist || !d_dot ||
        !d_level || !d_mp_desc || !d_pt_n || !d_match || !d_nmatches)
        return PLVI_E_BADARG;
    return launch_lds<search_sim3_proj_kernel>(
        dim3(n_pairs), dim3(256), sim3_smem(kp_cap, pt_cap), (hipStream_t)stream, *p, d_kps, d_desc, d_kp_n, kp_cap,
        d_matched, d_cell_off, d_cell_idx, d_flags, d_x3dc, d_dist, d_dot, d_level, d_mp_desc, d_pt_n, pt_cap,
        d_match, d_nmatches);
}

// One pair from host memory, synchronous (grid built on the device).
extern "C" int plvi_search_sim3_projection(const plvi_sim3_proj_params* p, const plvi_keypoint* kps,
                                           const uint8_t* desc, int n_kp, const uint8_t* matched, const uint8_t* flags,
                                           const float* x3dc, const float* dist, const double* dot, const int* level,
                                           const uint8_t* mp_desc, int n_pt, int* match) {
    if (!sim3_params_ok(p) || n_kp < 0 || n_pt < 0 || (n_kp > 0 && (!kps || !desc || !match))) return PLVI_E_BADARG;
    if (n_pt > 0 && (!flags || !x3dc || !dist || !dot || !level || !mp_desc)) return PLVI_E_BADARG;
    if (n_kp == 0) return 0;
    const int kc = n_kp, pc = std::max(n_pt, 1);
    int counts[3] = {n_kp, n_pt, 0};  // [2]: nmatches
    HostStage st;
    const StagedImage im = stage_image(st, kps, desc, matched, n_kp, kc);
    const auto X = st.in_or_zero(x3dc, n_pt, 3), S = st.in_or_zero(dist, n_pt, 3);
    const auto T = st.in_or_zero(dot, n_pt);
    const auto F = st.in_or_zero(flags, n_pt), MD = st.in_or_zero(mp_desc, n_pt, 32);
    const auto L = st.in_or_zero(level, n_pt), M = st.out(match, kc), N = st.inout(counts, 3);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = stage_grid(st, p, im, dN, kc)) return rc;
    if (int rc = plvi_search_sim3_projection_batch(1, p, st.dev(im.k), st.dev(im.d), dN, kc, st.dev(im.b),
                                                   st.dev(im.co), st.dev(im.ci), st.dev(F), st.dev(X), st.dev(S),
                                                   st.dev(T), st.dev(L), st.dev(MD), dN + 1, pc, st.dev(M), dN + 2,
                                                   nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[2];
}

extern "C" int plvi_search_local_batch(int n_frames, const plvi_local_params* p, const plvi_keypoint* d_kps,
                                       const uint8_t* d_desc, const int* d_n, int cap, const uint8_t* d_blocked,
                                       const float* d_uright, const int* d_cell_off, const int* d_cell_idx,
                                       const uint8_t* d_mp_flags, const float* d_mp_proj, const int* d_mp_level,
                                       const uint8_t* d_mp_desc, const int* d_mp_n, int mp_cap, int* d_match,
                                       int* d_nmatches, void* stream) {
    if (!p || n_frames < 0 || cap < 1 || mp_cap < 1 || cap > 65535) return PLVI_E_BADARG;
    if (p->nlevels < 1 || p->nlevels > 16) return PLVI_E_BADARG;
    if (n_frames == 0) return PLVI_OK;
    return launch_lds<search_local_kernel>(
        dim3(n_frames), dim3(256), local_smem(cap, mp_cap), (hipStream_t)stream, *p, d_kps, d_desc, d_n, cap,
        d_blocked, d_uright, d_cell_off, d_cell_idx, d_mp_flags, d_mp_proj, d_mp_level, d_mp_desc, d_mp_n, mp_cap,
        d_match, d_nmatches);
}

// One frame from host memory, synchronous (grid built on the device).
extern "C" int plvi_search_local(const plvi_local_params* p, const plvi_keypoint* kps, const uint8_t* desc, int n,
                                 const uint8_t* blocked, const float* uright, const uint8_t* mp_flags,
                                 const float* mp_proj, const int* mp_level, const uint8_t* mp_desc, int n_mp,
                                 int* match) {
    if (!p || n < 0 || n_mp < 0 || (n > 0 && (!kps || !desc || !match))) return PLVI_E_BADARG;
    if (n == 0) return 0;
    const int cc = n, mc = std::max(n_mp, 1);
    int counts[3] = {n, n_mp, 0};  // [2]: nmatches
    HostStage st;
    const StagedImage im = stage_image(st, kps, desc, blocked, n, cc);
    const auto U = st.in(uright, cc), P = st.in_or_zero(mp_proj, n_mp, 4);
    const auto F = st.in_or_zero(mp_flags, n_mp), MD = st.in_or_zero(mp_desc, n_mp, 32);
    const auto L = st.in_or_zero(mp_level, n_mp), M = st.out(match, cc), N = st.inout(counts, 3);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = stage_grid(st, p, im, dN, cc)) return rc;
    if (int rc = plvi_search_local_batch(1, p, st.dev(im.k), st.dev(im.d), dN, cc, st.dev(im.b), st.dev(U),
                                         st.dev(im.co), st.dev(im.ci), st.dev(F), st.dev(P), st.dev(L), st.dev(MD),
                                         dN + 1, mc, st.dev(M), dN + 2, nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[2];
}

extern "C" int plvi_search_local_stereo_batch(
    int n_frames, const plvi_local_params* p, const plvi_keypoint* d_kps, const uint8_t* d_desc, const int* d_n,
    int cap, const uint8_t* d_blocked, const int* d_l2r, const int* d_cell_off, const int* d_cell_idx,
    const plvi_keypoint* d_kps_r, const uint8_t* d_desc_r, const int* d_n_r, int cap_r, const uint8_t* d_blocked_r,
    const int* d_r2l, const int* d_cell_off_r, const int* d_cell_idx_r, const uint8_t* d_mp_flags,
    const float* d_mp_proj, const int* d_mp_level, const float* d_mp_proj_r, const int* d_mp_level_r,
    const uint8_t* d_mp_desc, const int* d_mp_n, int mp_cap, int* d_match, int* d_match_r, int* d_nmatches,
    void* stream) {
    if (!p || n_frames < 0 || cap < 1 || cap_r < 1 || mp_cap < 1 || cap > 65535 || cap_r > 65535)
        return PLVI_E_BADARG;
    if (p->nlevels < 1 || p->nlevels > 16) return PLVI_E_BADARG;
    if (n_frames == 0) return PLVI_OK;
    return launch_lds<search_local2_kernel>(
        dim3(n_frames), dim3(256), local2_smem(cap, cap_r, mp_cap), (hipStream_t)stream, *p, d_kps, d_desc, d_n, cap,
        d_blocked, d_l2r, d_cell_off, d_cell_idx, d_kps_r, d_desc_r, d_n_r, cap_r, d_blocked_r, d_r2l, d_cell_off_r,
        d_cell_idx_r, d_mp_flags, d_mp_proj, d_mp_level, d_mp_proj_r, d_mp_level_r, d_mp_desc, d_mp_n, mp_cap,
        d_match, d_match_r, d_nmatches);
}

// One two-camera frame from host memory, synchronous (both grids built on the device).
extern "C" int plvi_search_local_stereo(const plvi_local_params* p, const plvi_keypoint* kps, const uint8_t* desc,
                                        int n, const uint8_t* blocked, const int* l2r, const plvi_keypoint* kps_r,
                                        const uint8_t* desc_r, int n_r, const uint8_t* blocked_r, const int* r2l,
                                        const uint8_t* mp_flags, const float* mp_proj, const int* mp_level,
                                        const float* mp_proj_r, const int* mp_level_r, const uint8_t* mp_desc,
                                        int n_mp, int* match, int* match_r) {
    if (!p || n < 0 || n_r < 0 || n_mp < 0) return PLVI_E_BADARG;
    if ((n > 0 && (!kps || !desc || !match)) || (n_r > 0 && (!kps_r || !desc_r || !match_r))) return PLVI_E_BADARG;
    if (n_mp > 0 && (!mp_flags || !mp_proj || !mp_level || !mp_proj_r || !mp_level_r || !mp_desc))
        return PLVI_E_BADARG;
    if (n + n_r == 0) return 0;
    const int cl = std::max(n, 1), cr = std::max(n_r, 1), mc = std::max(n_mp, 1);
    const std::vector<int> none(std::max(n, n_r), -1);  // no stereo pairs = every entry -1
    int counts[4] = {n, n_r, n_mp, 0};                  // [3]: nmatches
    HostStage st;
    const StagedImage il = stage_image(st, kps, desc, blocked, n, cl);
    const StagedImage ir = stage_image(st, kps_r, desc_r, blocked_r, n_r, cr);
    const auto P2 = st.in_or_zero(l2r ? l2r : none.data(), n), P2R = st.in_or_zero(r2l ? r2l : none.data(), n_r);
    const auto P = st.in_or_zero(mp_proj, n_mp, 4), PR = st.in_or_zero(mp_proj_r, n_mp, 4);
    const auto F = st.in_or_zero(mp_flags, n_mp), MD = st.in_or_zero(mp_desc, n_mp, 32);
    const auto L = st.in_or_zero(mp_level, n_mp), LR = st.in_or_zero(mp_level_r, n_mp);
    const auto M = st.out_or_scratch(match, n), MR = st.out_or_scratch(match_r, n_r), N = st.inout(counts, 4);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = stage_grid(st, p, il, dN, cl)) return rc;
    if (int rc = stage_grid(st, p, ir, dN + 1, cr)) return rc;
    if (int rc = plvi_search_local_stereo_batch(
            1, p, st.dev(il.k), st.dev(il.d), dN, cl, st.dev(il.b), st.dev(P2), st.dev(il.co), st.dev(il.ci),
            st.dev(ir.k), st.dev(ir.d), dN + 1, cr, st.dev(ir.b), st.dev(P2R), st.dev(ir.co), st.dev(ir.ci), st.dev(F),
            st.dev(P), st.dev(L), st.dev(PR), st.dev(LR), st.dev(MD), dN + 2, mc, st.dev(M), st.dev(MR), dN + 3,
            nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[3];
}

extern "C" int plvi_search_by_projection_stereo_batch(
    int n_pairs, const plvi_proj_params* p, const float* kb8, const plvi_keypoint* d_kps, const uint8_t* d_desc,
    const int* d_n, int cap, const uint8_t* d_blocked, const int* d_cell_off, const int* d_cell_idx,
    const plvi_keypoint* d_kps_r, const uint8_t* d_desc_r, const int* d_n_r, int cap_r, const uint8_t* d_blocked_r,
    const int* d_cell_off_r, const int* d_cell_idx_r, const float* d_x3dc, const float* d_x3dr,
    const int* d_last_octave, const float* d_last_angle, const uint8_t* d_mp_desc, const uint8_t* d_last_flags,
    const int* d_last_n, int last_cap, int* d_match, int* d_match_r, int* d_nmatches, void* stream) {
    if (!p || n_pairs < 0 || cap < 1 || cap_r < 1 || last_cap < 1 || cap > 65535 || cap_r > 65535 ||
        last_cap > 65535)
        return PLVI_E_BADARG;
    if (p->nlevels < 1 || p->nlevels > 16) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    CamModel cm{0, 0.f, 0.f, 0.f, 0.f};
    if (kb8) cm = CamModel{1, kb8[0], kb8[1], kb8[2], kb8[3]};
    return launch_lds<search_by_projection2_kernel>(
        dim3(n_pairs), dim3(256), proj2_smem(cap, cap_r, last_cap), (hipStream_t)stream, *p, cm, d_kps, d_desc, d_n,
        cap, d_blocked, d_cell_off, d_cell_idx, d_kps_r, d_desc_r, d_n_r, cap_r, d_blocked_r, d_cell_off_r,
        d_cell_idx_r, d_x3dc, d_x3dr, d_last_octave, d_last_angle, d_mp_desc, d_last_flags, d_last_n, last_cap,
        d_match, d_match_r, d_nmatches);
}

// One pair from host memory, synchronous (both grids built on the device).
extern "C" int plvi_search_by_projection_stereo(const plvi_proj_params* p, const float* kb8, const plvi_keypoint* kps,
                                                const uint8_t* desc, int n, const uint8_t* blocked,
                                                const plvi_keypoint* kps_r, const uint8_t* desc_r, int n_r,
                                                const uint8_t* blocked_r, const float* x3dc, const float* x3dr,
                                                const int* last_octave, const float* last_angle,
                                                const uint8_t* mp_desc, const uint8_t* last_flags, int n_last,
                                                int* match, int* match_r) {
    if (!p || n < 0 || n_r < 0 || n_last < 0) return PLVI_E_BADARG;
    if ((n > 0 && (!kps || !desc || !match)) || (n_r > 0 && (!kps_r || !desc_r || !match_r))) return PLVI_E_BADARG;
    if (n_last > 0 && (!x3dc || !x3dr || !last_octave || !last_angle || !mp_desc || !last_flags)) return PLVI_E_BADARG;
    const int cl = std::max(n, 1), cr = std::max(n_r, 1), lc = std::max(n_last, 1);
    int counts[4] = {n, n_r, n_last, 0};  // [3]: nmatches
    HostStage st;
    const StagedImage il = stage_image(st, kps, desc, blocked, n, cl);
    const StagedImage ir = stage_image(st, kps_r, desc_r, blocked_r, n_r, cr);
    const auto X = st.in_or_zero(x3dc, n_last, 3), XR = st.in_or_zero(x3dr, n_last, 3);
    const auto A = st.in_or_zero(last_angle, n_last);
    const auto MD = st.in_or_zero(mp_desc, n_last, 32), F = st.in_or_zero(last_flags, n_last);
    const auto O = st.in_or_zero(last_octave, n_last);
    const auto M = st.out_or_scratch(match, n), MR = st.out_or_scratch(match_r, n_r), N = st.inout(counts, 4);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = stage_grid(st, p, il, dN, cl)) return rc;
    if (int rc = stage_grid(st, p, ir, dN + 1, cr)) return rc;
    if (int rc = plvi_search_by_projection_stereo_batch(
            1, p, kb8, st.dev(il.k), st.dev(il.d), dN, cl, st.dev(il.b), st.dev(il.co), st.dev(il.ci), st.dev(ir.k),
            st.dev(ir.d), dN + 1, cr, st.dev(ir.b), st.dev(ir.co), st.dev(ir.ci), st.dev(X), st.dev(XR), st.dev(O),
            st.dev(A), st.dev(MD), st.dev(F), dN + 2, lc, st.dev(M), st.dev(MR), dN + 3, nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[3];
}
