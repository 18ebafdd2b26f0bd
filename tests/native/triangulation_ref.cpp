// triangulation_ref.cpp — TEST INFRASTRUCTURE ONLY.
//
// Host restatement of the two triangulation-candidate searches, the expected
// values of tests/test_triangulation.py (built -ffp-contract=off, loaded with
// ctypes):
//   ORBmatcher::SearchForTriangulation   src/ORBmatcher.cc:965-1206, the
//     single-camera Pinhole branch, with Pinhole::epipolarConstrain
//     (src/CameraModels/Pinhole.cpp:143-156) downstream of F12
//   LineMatcher::SearchForTriangulation  src/LineMatcher.cpp:142-171 with
//     knnMatch(k = 2) and Frame::lineDescriptorMAD (src/Frame.cc:1089-1112)
// written sequentially in the reference's own order (the merge walk with its
// lower_bound jumps, the candidate loop with bestDist), not the way the HIP
// kernels are organised.  The fused multiply-adds are the ones the reference
// objects hold (tests/test_ref_objects_triangulation.py).
//
// tri_ref_points also reports why each KF1 keypoint ended as it did, so a
// test can prove from the restatement alone which branch its input takes.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/plvi_frontend.h"
#include "../../oracle/ref_fma.h"

enum {
    TRI_HAS_POINT = 1,      // pMP1 (:1036)
    TRI_STEREO_FILTERED = 2,  // bOnlyStereo && !bStereo1 (:1043-1045)
    TRI_NO_SHARED_NODE = 3,  // its node is absent from KF2's FeatureVector (or it is in no node at all)
    TRI_NO_CANDIDATE = 4,   // no KF2 entry of the node got past :1067-1081
    TRI_EPIPOLE = 5,        // every candidate that got there fell to the epipole test (:1089-1097)
    TRI_EPILINE = 6,        // none accepted, at least one refused by epipolarConstrain
    TRI_ACCEPTED = 7,
    TRI_HISTOGRAM = 8,      // accepted, then removed by the rotation filter (:1174-1193)
};

namespace {

const int TH_LOW = 50, HISTO_LENGTH = 30;

int descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

// first position in [lo, n) whose id is not below `id` (std::map::lower_bound over the sorted ids)
int lower_bound_from(const int* node, int lo, int n, int id) {
    return (int)(std::lower_bound(node + lo, node + n, id) - node);
}

bool epipolar_constrain(const float* F, const plvi_keypoint& kp1, const plvi_keypoint& kp2, float unc) {
    const float a = ref_fmaf(kp1.x, F[0], kp1.y * F[3]) + F[6];
    const float b = ref_fmaf(kp1.x, F[1], kp1.y * F[4]) + F[7];
    const float c = ref_fmaf(kp1.y, F[5], kp1.x * F[2]) + F[8];
    const float num = ref_fmaf(b, kp2.y, a * kp2.x) + c;
    const float den = ref_fmaf(a, a, b * b);
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return (double)dsqr < 3.84 * (double)unc;
}

int clampi(int v, int lo, int hi) { return std::min(std::max(v, lo), hi); }

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

extern "C" int tri_ref_points(const plvi_triangulation_pair* P, const plvi_keypoint* kps1, const uint8_t* desc1,
                              int n1, const int* node1, const int* off1, int nn1, const int* idx1,
                              const uint8_t* has1, const float* ur1, const plvi_keypoint* kps2, const uint8_t* desc2,
                              int n2, const int* node2, const int* off2, int nn2, const int* idx2,
                              const uint8_t* has2, const float* ur2, int* matches12, int* codes) {
    int nmatches = 0;
    std::vector<int> rotHist[HISTO_LENGTH];
    const float factor = 1.0f / HISTO_LENGTH;
    for (int i = 0; i < n1; ++i) {
        matches12[i] = -1;
        codes[i] = TRI_NO_SHARED_NODE;
    }
    const int nsig = clampi(P->n_sigma2, 1, 16), nsf = clampi(P->n_scale_factors, 1, 16);
    int f1 = 0, f2 = 0;
    while (f1 < nn1 && f2 < nn2) {
        if (node1[f1] == node2[f2]) {
            for (int a = off1[f1]; a < off1[f1 + 1]; ++a) {
                const int i1 = idx1[a];
                if (i1 < 0 || i1 >= n1) continue;
                if (has1[i1]) {
                    codes[i1] = TRI_HAS_POINT;
                    continue;
                }
                const bool bStereo1 = ur1[i1] >= 0;
                if (P->only_stereo && !bStereo1) {
                    codes[i1] = TRI_STEREO_FILTERED;
                    continue;
                }
                const plvi_keypoint& kp1 = kps1[i1];
                int bestDist = TH_LOW, bestIdx2 = -1;
                int reached = 0, by_line = 0;
                for (int b = off2[f2]; b < off2[f2 + 1]; ++b) {
                    const int i2 = idx2[b];
                    if (i2 < 0 || i2 >= n2) continue;
                    if (has2[i2]) continue;  // vbMatched2 is never set
                    const bool bStereo2 = ur2[i2] >= 0;
                    if (P->only_stereo && !bStereo2) continue;
                    const int dist = descriptor_distance(desc1 + 32 * (size_t)i1, desc2 + 32 * (size_t)i2);
                    if (dist > TH_LOW || dist > bestDist) continue;
                    ++reached;
                    const plvi_keypoint& kp2 = kps2[i2];
                    if (!bStereo1 && !bStereo2) {
                        const float distex = P->ep[0] - kp2.x;
                        const float distey = P->ep[1] - kp2.y;
                        if (ref_fmaf(distex, distex, distey * distey) <
                            100 * P->scale_factors[clampi(kp2.octave, 0, nsf - 1)])
                            continue;
                    }
                    if (epipolar_constrain(P->F12, kp1, kp2, P->sigma2[clampi(kp2.octave, 0, nsig - 1)]) ||
                        P->coarse) {
                        bestIdx2 = i2;
                        bestDist = dist;
                    } else {
                        ++by_line;
                    }
                }
                if (bestIdx2 >= 0) {
                    matches12[i1] = bestIdx2;
                    codes[i1] = TRI_ACCEPTED;
                    ++nmatches;
                    if (P->check_orientation) {
                        float rot = kp1.angle - kps2[bestIdx2].angle;
                        if (rot < 0.0) rot += 360.0f;
                        int bin = (int)roundf(rot * factor);
                        if (bin == HISTO_LENGTH) bin = 0;
                        rotHist[bin].push_back(i1);
                    }
                } else {
                    codes[i1] = !reached ? TRI_NO_CANDIDATE : by_line ? TRI_EPILINE : TRI_EPIPOLE;
                }
            }
            ++f1;
            ++f2;
        } else if (node1[f1] < node2[f2]) {
            f1 = lower_bound_from(node1, f1, nn1, node2[f2]);
        } else {
            f2 = lower_bound_from(node2, f2, nn2, node1[f1]);
        }
    }
    if (P->check_orientation) {
        int hist[HISTO_LENGTH], ind1, ind2, ind3;
        for (int i = 0; i < HISTO_LENGTH; ++i) hist[i] = (int)rotHist[i].size();
        three_maxima(hist, HISTO_LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; ++i) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (size_t j = 0; j < rotHist[i].size(); ++j) {
                matches12[rotHist[i][j]] = -1;
                codes[rotHist[i][j]] = TRI_HISTOGRAM;
                --nmatches;
            }
        }
    }
    return nmatches;
}

// pairs: (query, train) rows in query order; mad: {nn_mad, nn12_mad}.  n1 = 0 or n2 < 2: 0 pairs
// (the reference indexes lmatches[0] and [i][1] there; the product documents 0 matches).
extern "C" int tri_ref_lines(const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, const uint8_t* has1,
                             const uint8_t* has2, double th_factor, int* pairs, double* mad) {
    mad[0] = mad[1] = 0.0;
    if (n1 <= 0 || n2 < 2) return 0;
    // knnMatch(k = 2): train rows ascending, a later row replaces only on a strictly smaller distance
    std::vector<int> i0(n1);
    std::vector<float> d0(n1), d1(n1);
    for (int q = 0; q < n1; ++q) {
        int b0 = -1, bd0 = 1 << 30, bd1 = 1 << 30;
        for (int t = 0; t < n2; ++t) {
            const int d = descriptor_distance(desc1 + 32 * (size_t)q, desc2 + 32 * (size_t)t);
            if (d < bd0) {
                bd1 = bd0;
                bd0 = d;
                b0 = t;
            } else if (d < bd1) {
                bd1 = d;
            }
        }
        i0[q] = b0;
        d0[q] = (float)bd0;
        d1[q] = (float)bd1;
    }
    // lineDescriptorMAD: medians as element n/2 of the sorted lists
    const size_t mid = (size_t)(n1 / 2);
    std::vector<float> v(d0);
    std::sort(v.begin(), v.end());
    const double nn_median = v[mid];
    for (int q = 0; q < n1; ++q) v[q] = fabsf((float)(d0[q] - nn_median));
    std::sort(v.begin(), v.end());
    mad[0] = 1.4826 * v[mid];
    std::vector<float> w(n1);
    for (int q = 0; q < n1; ++q) w[q] = d1[q] - d0[q];
    std::sort(w.begin(), w.end(), [](float x, float y) { return x > y; });
    const double nn12_median = w[mid];
    for (int q = 0; q < n1; ++q) v[q] = fabsf((float)(d1[q] - d0[q] - nn12_median));
    std::sort(v.begin(), v.end());
    mad[1] = 1.4826 * v[mid];
    const double th = mad[1] * th_factor;
    int n = 0;
    for (int q = 0; q < n1; ++q) {
        if ((has1 && has1[q]) || (has2 && has2[i0[q]])) continue;
        const double dist_12 = d1[q] - d0[q];
        if (dist_12 > th) {
            pairs[2 * n] = q;
            pairs[2 * n + 1] = i0[q];
            ++n;
        }
    }
    return n;
}
