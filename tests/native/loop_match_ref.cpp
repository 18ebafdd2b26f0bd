// loop_match_ref.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host restatement of the loop-closing matchers, the expected values of
// tests/test_loop_match.py (built -ffp-contract=off, loaded with ctypes):
//   ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12)
//     src/ORBmatcher.cc:823-963, single-camera branch
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th,
//     ratioHamming)                       src/ORBmatcher.cc:473-586
//   the overload with vpPointsKFs / vpMatchedKF   src/ORBmatcher.cc:588-704
//     both downstream of the caller's MapPoint reads and cv::Mat products,
//     with KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:1200-1244) over a grid
//     filled as Frame::AssignFeaturesToGrid fills it, and KeyFrame::IsInImage
// written sequentially in the reference's own order (one loop over the shared
// nodes / over vpPoints, vbMatched2 / vpMatched updated as it goes), not the
// way the HIP kernels are organised.  The two fused multiply-adds are the
// ones the reference object holds in the :588 overload
// (tests/test_ref_objects_loop.py).
//
// Both functions also report why each KF1 keypoint / each point ended as it
// did, so a test can prove from the restatement alone which branch its input
// takes.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/plvi_frontend.h"
#include "../../oracle/ref_fma.h"

enum {
    BOW_NOT_LIVE = 1,        // !pMP1 || pMP1->isBad() (:863-866)
    BOW_NO_SHARED_NODE = 2,  // its node is absent from KF2's FeatureVector (or it is in no node at all)
    BOW_NO_CANDIDATE = 3,    // every KF2 entry of the node was matched, not live or absent: bestDist1 stays 256
    BOW_TH_LOW = 4,          // bestDist1 >= TH_LOW (:906)
    BOW_RATIO = 5,           // the ratio test (:908)
    BOW_ACCEPTED = 6,
    BOW_HISTOGRAM = 7,       // accepted, then removed by the rotation filter (:942-960)
};

enum {
    SIM3_FLAG = 1,          // isBad() || spAlreadyFound.count(pMP) (:501)
    SIM3_DEPTH = 2,         // z < 0.0 (:511)
    SIM3_IMAGE = 3,         // !IsInImage (:522)
    SIM3_DISTANCE = 4,      // dist < minDistance || dist > maxDistance (:531)
    SIM3_ANGLE = 5,         // PO.dot(Pn) < 0.5 * dist (:537)
    SIM3_LEVEL = 6,         // predicted level outside [0, nlevels): no scale factor (not reachable in the reference)
    SIM3_EMPTY_WINDOW = 7,  // vIndices.empty() (:547)
    SIM3_NO_CANDIDATE = 8,  // every keypoint of the window is matched or at another level: bestDist stays 256
    SIM3_THRESHOLD = 9,     // bestDist > TH_LOW * ratioHamming (:577)
    SIM3_ACCEPTED = 10,
};

namespace {

const int TH_LOW = 50, HISTO_LENGTH = 30;
const int GRID_COLS = 64, GRID_ROWS = 48;  // FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h:47-48)

int descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// first position in [lo, n) whose id is not below `id` (std::map::lower_bound over the sorted ids)
int lower_bound_from(const int* node, int lo, int n, int id) {
    return (int)(std::lower_bound(node + lo, node + n, id) - node);
}

void three_maxima(const int* hist, int L, int& ind1, int& ind2, int& ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    ind1 = ind2 = ind3 = -1;
    for (int i = 0; i < L; ++i) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
}

}  // namespace

// matches12 [n1] (KF2 keypoint index or -1), code [n1]; returns nmatches.
extern "C" int loop_ref_bow_kf(float nnratio, int check_orientation, const uint8_t* desc1, const float* angle1,
                               const uint8_t* live1, int n1, const int* node1, const int* off1, int nnodes1,
                               const int* idx1v, const uint8_t* desc2, const float* angle2, const uint8_t* live2,
                               int n2, const int* node2, const int* off2, int nnodes2, const int* idx2v,
                               int* matches12, int* code) {
    for (int i = 0; i < n1; ++i) {
        matches12[i] = -1;
        code[i] = live1[i] ? BOW_NO_SHARED_NODE : BOW_NOT_LIVE;
    }
    std::vector<char> vbMatched2(std::max(n2, 1), 0);
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;
    int nmatches = 0;
    int f1 = 0, f2 = 0;
    while (f1 < nnodes1 && f2 < nnodes2) {
        if (node1[f1] == node2[f2]) {
            for (int i1 = off1[f1]; i1 < off1[f1 + 1]; ++i1) {
                const int idx1 = idx1v[i1];
                if (idx1 < 0 || idx1 >= n1) continue;  // not a keypoint of KF1
                if (!live1[idx1]) continue;
                int bestDist1 = 256, bestIdx2 = -1, bestDist2 = 256;
                for (int i2 = off2[f2]; i2 < off2[f2 + 1]; ++i2) {
                    const int idx2 = idx2v[i2];
                    if (idx2 < 0 || idx2 >= n2) continue;
                    if (vbMatched2[idx2] || !live2[idx2]) continue;
                    const int dist = descriptor_distance(desc1 + 32 * (size_t)idx1, desc2 + 32 * (size_t)idx2);
                    if (dist < bestDist1) {
                        bestDist2 = bestDist1;
                        bestDist1 = dist;
                        bestIdx2 = idx2;
                    } else if (dist < bestDist2) {
                        bestDist2 = dist;
                    }
                }
                if (bestIdx2 < 0) {
                    code[idx1] = BOW_NO_CANDIDATE;
                } else if (bestDist1 < TH_LOW) {
                    if ((float)bestDist1 < nnratio * (float)bestDist2) {
                        matches12[idx1] = bestIdx2;
                        vbMatched2[bestIdx2] = 1;
                        code[idx1] = BOW_ACCEPTED;
                        if (check_orientation) {
                            float rot = angle1[idx1] - angle2[bestIdx2];
                            if (rot < 0.0) rot += 360.0f;
                            int bin = (int)roundf(rot * factor);
                            if (bin == HISTO_LENGTH) bin = 0;
                            rotHist[bin].push_back(idx1);
                        }
                        nmatches++;
                    } else {
                        code[idx1] = BOW_RATIO;
                    }
                } else {
                    code[idx1] = BOW_TH_LOW;
                }
            }
            ++f1;
            ++f2;
        } else if (node1[f1] < node2[f2]) {
            f1 = lower_bound_from(node1, f1, nnodes1, node2[f2]);
        } else {
            f2 = lower_bound_from(node2, f2, nnodes2, node1[f1]);
        }
    }
    if (check_orientation) {
        int hist[HISTO_LENGTH], ind1, ind2, ind3;
        for (int i = 0; i < HISTO_LENGTH; ++i) hist[i] = (int)rotHist[i].size();
        three_maxima(hist, HISTO_LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; ++i) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (int idx1 : rotHist[i]) {
                matches12[idx1] = -1;
                code[idx1] = BOW_HISTOGRAM;
                nmatches--;
            }
        }
    }
    return nmatches;
}

// match [n_kp] (point index or -1), code [n_pt], uv [n_pt][2] (the projection of every point that got as far
// as IsInImage, else untouched); returns nmatches.
extern "C" int loop_ref_sim3_projection(const plvi_sim3_proj_params* p, const plvi_keypoint* kps, const uint8_t* desc,
                                        int n_kp, const uint8_t* matched, const uint8_t* flags, const float* x3dc,
                                        const float* dist3, const double* dot, const int* level,
                                        const uint8_t* mp_desc, int n_pt, int* match, int* code, float* uv) {
    // Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:688-722, :1077-1089); the KeyFrame copies the grid
    std::vector<int> grid[GRID_COLS][GRID_ROWS];
    for (int i = 0; i < n_kp; ++i) {
        const int posX = (int)roundf((kps[i].x - p->min_x) * p->inv_w);
        const int posY = (int)roundf((kps[i].y - p->min_y) * p->inv_h);
        if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) continue;
        grid[posX][posY].push_back(i);
    }
    std::vector<char> vpMatched(std::max(n_kp, 1), 0);
    for (int i = 0; i < n_kp; ++i) {
        vpMatched[i] = matched && matched[i];
        match[i] = -1;
    }
    int nmatches = 0;
    for (int iMP = 0; iMP < n_pt; ++iMP) {
        if (!(flags[iMP] & 1)) { code[iMP] = SIM3_FLAG; continue; }
        const float X = x3dc[3 * iMP], Y = x3dc[3 * iMP + 1], Z = x3dc[3 * iMP + 2];
        if (Z < 0.0) { code[iMP] = SIM3_DEPTH; continue; }
        float u, v;
        if (p->projection) {  // :631-636, fused as in the reference object
            const float invz = 1 / Z;
            const float x = X * invz;
            const float y = Y * invz;
            u = ref_fmaf(p->fx, x, p->cx);
            v = ref_fmaf(p->fy, y, p->cy);
        } else {  // Pinhole::project (Pinhole.cpp:36-42), no fused operation
            u = p->fx * X / Z + p->cx;
            v = p->fy * Y / Z + p->cy;
        }
        if (uv) {
            uv[2 * iMP] = u;
            uv[2 * iMP + 1] = v;
        }
        if (!(u >= p->min_x && u < p->max_x && v >= p->min_y && v < p->max_y)) { code[iMP] = SIM3_IMAGE; continue; }
        const float dist = dist3[3 * iMP], minDistance = dist3[3 * iMP + 1], maxDistance = dist3[3 * iMP + 2];
        if (dist < minDistance || dist > maxDistance) { code[iMP] = SIM3_DISTANCE; continue; }
        if (dot[iMP] < 0.5 * dist) { code[iMP] = SIM3_ANGLE; continue; }
        const int nPredictedLevel = level[iMP];
        if (nPredictedLevel < 0 || nPredictedLevel >= p->nlevels) { code[iMP] = SIM3_LEVEL; continue; }
        const float radius = p->th * p->scale_factors[nPredictedLevel];

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
        if (vIndices.empty()) { code[iMP] = SIM3_EMPTY_WINDOW; continue; }

        int bestDist = 256, bestIdx = -1;
        for (int idx : vIndices) {
            if (vpMatched[idx]) continue;
            const int kpLevel = kps[idx].octave;
            if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;
            const int d = descriptor_distance(mp_desc + 32 * (size_t)iMP, desc + 32 * (size_t)idx);
            if (d < bestDist) {
                bestDist = d;
                bestIdx = idx;
            }
        }
        if (bestDist <= TH_LOW * p->ratio_hamming) {
            if (bestIdx < 0) return -1;  // the reference would write vpMatched[-1]: 50 * ratio >= 256 is refused
            vpMatched[bestIdx] = 1;
            match[bestIdx] = iMP;
            code[iMP] = SIM3_ACCEPTED;
            nmatches++;
        } else {
            code[iMP] = bestIdx < 0 ? SIM3_NO_CANDIDATE : SIM3_THRESHOLD;
        }
    }
    return nmatches;
}
