// triangulation.hip — ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12,
// vMatchedPairs, bOnlyStereo, bCoarse) (src/ORBmatcher.cc:965-1206), the
// candidate search of LocalMapping::CreateNewMapPoints (LocalMapping.cc:804),
// single-camera branch (no mpCamera2, NLeft == -1, Pinhole), batched over
// (KF1, KF2) pairs.
//
// The reference allocates vbMatched2 (:1011), reads it (:1067) and never
// writes it, and bestDist only moves when a candidate passes the geometric
// tests (:1132-1136), so every KF1 keypoint is independent: its result is the
// candidate of its node's KF2 list that passes the tests with the smallest
// distance <= TH_LOW, the latest in list order among equal distances (the
// skip is `dist > bestDist`, :1080).  Several KF1 keypoints may take the same
// KF2 keypoint.
//
// Kernels (per call): tri_fill_kernel sets rows [0, n1) of matches12 to -1;
// tri_match_kernel, grid (pair, slice), stages the pair's KF2 FeatureVector
// list in LDS in list order (descriptor, x, y, 3.84-test sigma2, 100 * scale
// factor, index | stereo bit; -1 for an entry the reference skips before the
// distance) with both node tables, then every thread owns positions of KF1's
// list: its node's KF2 range is found by binary search of the node id (the
// lower_bound merge walk of :1025-1172 visits exactly the ids present in both
// sorted lists), its descriptor and epipolar line (a, b, c, den) stay in
// registers and it replays the reference's loop over the range -- lanes of
// one node read the same LDS slots (broadcast).  tri_finish_kernel, one
// workgroup per pair: rotation histogram, ComputeThreeMaxima, the filter and
// nmatches.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "grid_search.h"
#include "host_stage.h"
#include "plvi_common.h"
#include "plvi_math.h"

namespace plvi {
namespace {

constexpr int kTriTHLow = 50, kTriHisto = 30;  // ORBmatcher::TH_LOW, HISTO_LENGTH
constexpr int kTriThreads = 512;
constexpr int kTriSkip = -1, kTriStereoBit = 1 << 30;

struct TriLds {
    uint4* desc;   // [2 * cap2] the KF2 list's descriptors, list order
    float4* geo;   // [cap2] x, y, mvLevelSigma2[octave], 100 * mvScaleFactors[octave]
    int* idx;      // [cap2] KF2 keypoint index | kTriStereoBit, or kTriSkip
    int *node1, *off1, *node2, *off2;  // [node_cap], [node_cap + 1] each side
};

__device__ __forceinline__ TriLds tri_carve(unsigned char* q, int cap2, int node_cap) {
    TriLds s;
    s.desc = reinterpret_cast<uint4*>(q); q += (size_t)32 * cap2;
    s.geo = reinterpret_cast<float4*>(q); q += (size_t)16 * cap2;
    s.idx = reinterpret_cast<int*>(q); q += (size_t)4 * cap2;
    s.node1 = reinterpret_cast<int*>(q); q += (size_t)4 * node_cap;
    s.off1 = reinterpret_cast<int*>(q); q += (size_t)4 * (node_cap + 1);
    s.node2 = reinterpret_cast<int*>(q); q += (size_t)4 * node_cap;
    s.off2 = reinterpret_cast<int*>(q);
    return s;
}

size_t tri_smem(int cap2, int node_cap) { return (size_t)52 * cap2 + (size_t)16 * node_cap + 8; }

}  // namespace

__global__ __launch_bounds__(256) void tri_fill_kernel(const int* __restrict__ n1_all, int cap1,
                                                       int* __restrict__ m12_all) {
    const int p = blockIdx.x, n1 = clampi(n1_all[p], 0, cap1);
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i < n1) m12_all[(size_t)p * cap1 + i] = -1;
}

__global__ __launch_bounds__(kTriThreads) void tri_match_kernel(
    const plvi_triangulation_pair* __restrict__ pairs, int cap1, int cap2, int node_cap,
    const plvi_keypoint* __restrict__ kps1_all, const uint8_t* __restrict__ desc1_all, const int* __restrict__ n1_all,
    const int* __restrict__ node1_all, const int* __restrict__ off1_all, const int* __restrict__ nnodes1_all,
    const int* __restrict__ idx1_all, const uint8_t* __restrict__ has1_all, const float* __restrict__ ur1_all,
    const plvi_keypoint* __restrict__ kps2_all, const uint8_t* __restrict__ desc2_all, const int* __restrict__ n2_all,
    const int* __restrict__ node2_all, const int* __restrict__ off2_all, const int* __restrict__ nnodes2_all,
    const int* __restrict__ idx2_all, const uint8_t* __restrict__ has2_all, const float* __restrict__ ur2_all,
    int* __restrict__ m12_all) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int p = blockIdx.x, tid = threadIdx.x;
    const TriLds s = tri_carve(lds, cap2, node_cap);
    const plvi_triangulation_pair& P = pairs[p];
    const int n1 = clampi(n1_all[p], 0, cap1), n2 = clampi(n2_all[p], 0, cap2);
    const int nn1 = clampi(nnodes1_all[p], 0, node_cap), nn2 = clampi(nnodes2_all[p], 0, node_cap);
    const int* O1 = off1_all + (size_t)p * (node_cap + 1);
    const int* O2 = off2_all + (size_t)p * (node_cap + 1);
    // list lengths: an offset outside [0, cap] is read as clamped, like a count
    const int len1 = nn1 ? clampi(O1[nn1], 0, cap1) : 0, len2 = nn2 ? clampi(O2[nn2], 0, cap2) : 0;
    if (len1 == 0 || len2 == 0 || n1 == 0 || n2 == 0) return;  // rows stay -1 (tri_fill_kernel)
    const bool onlyStereo = P.only_stereo != 0, coarse = P.coarse != 0;
    const int nsig = clampi(P.n_sigma2, 1, 16), nsf = clampi(P.n_scale_factors, 1, 16);

    for (int i = tid; i < nn1; i += kTriThreads) s.node1[i] = node1_all[(size_t)p * node_cap + i];
    for (int i = tid; i <= nn1; i += kTriThreads) s.off1[i] = clampi(O1[i], 0, len1);
    for (int i = tid; i < nn2; i += kTriThreads) s.node2[i] = node2_all[(size_t)p * node_cap + i];
    for (int i = tid; i <= nn2; i += kTriThreads) s.off2[i] = clampi(O2[i], 0, len2);
    const plvi_keypoint* K2 = kps2_all + (size_t)p * cap2;
    const uint8_t* D2 = desc2_all + (size_t)p * cap2 * 32;
    const uint8_t* H2 = has2_all + (size_t)p * cap2;
    const float* U2 = ur2_all + (size_t)p * cap2;
    const int* I2 = idx2_all + (size_t)p * cap2;
    for (int b = tid; b < len2; b += kTriThreads) {
        const int i2 = I2[b];
        int tag = kTriSkip;
        if (i2 >= 0 && i2 < n2 && !H2[i2]) {  // pMP2 (:1067)
            const bool stereo2 = U2[i2] >= 0;  // bStereo2 (:1070)
            if (!onlyStereo || stereo2) {      // (:1072-1074)
                const plvi_keypoint k = K2[i2];
                const uint4* d = reinterpret_cast<const uint4*>(D2 + (size_t)32 * i2);
                s.desc[2 * b] = d[0];
                s.desc[2 * b + 1] = d[1];
                s.geo[b] = make_float4(k.x, k.y, P.sigma2[clampi(k.octave, 0, nsig - 1)],
                                       100 * P.scale_factors[clampi(k.octave, 0, nsf - 1)]);
                tag = i2 | (stereo2 ? kTriStereoBit : 0);
            }
        }
        s.idx[b] = tag;
    }
    __syncthreads();

    const plvi_keypoint* K1 = kps1_all + (size_t)p * cap1;
    const uint8_t* D1 = desc1_all + (size_t)p * cap1 * 32;
    const uint8_t* H1 = has1_all + (size_t)p * cap1;
    const float* U1 = ur1_all + (size_t)p * cap1;
    const int* I1 = idx1_all + (size_t)p * cap1;
    int* M = m12_all + (size_t)p * cap1;
    const float epx = P.ep[0], epy = P.ep[1];
    for (int a = blockIdx.y * kTriThreads + tid; a < len1; a += gridDim.y * kTriThreads) {
        if (a < s.off1[0]) continue;  // before the first node's list
        const int i1 = I1[a];
        if (i1 < 0 || i1 >= n1 || H1[i1]) continue;  // pMP1 (:1036)
        const bool stereo1 = U1[i1] >= 0;            // bStereo1 (:1041)
        if (onlyStereo && !stereo1) continue;
        // KF1 node of list position a: the last node whose offset is <= a
        int lo = 0, hi = nn1;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s.off1[mid] <= a) lo = mid; else hi = mid;
        }
        const int id = s.node1[lo];
        // the same node id in KF2's sorted list
        int l2 = 0, h2 = nn2;
        while (l2 < h2) {
            const int mid = (l2 + h2) >> 1;
            if (s.node2[mid] < id) l2 = mid + 1; else h2 = mid;
        }
        if (l2 >= nn2 || s.node2[l2] != id) continue;
        const int f0 = s.off2[l2], f1 = s.off2[l2 + 1];

        const plvi_keypoint k1 = K1[i1];
        const uint4* dq = reinterpret_cast<const uint4*>(D1 + (size_t)32 * i1);
        const uint4 q0 = dq[0], q1 = dq[1];
        // Pinhole::epipolarConstrain (Pinhole.cpp:143-149) as the reference object fuses it:
        // l = x1' F12 = [a b c]
        const float x1 = k1.x, y1 = k1.y;
        const float la = rfmaf(x1, P.F12[0], y1 * P.F12[3]) + P.F12[6];
        const float lb = rfmaf(x1, P.F12[1], y1 * P.F12[4]) + P.F12[7];
        const float lc = rfmaf(y1, P.F12[5], x1 * P.F12[2]) + P.F12[8];
        const float den = rfmaf(la, la, lb * lb);

        int bestDist = kTriTHLow, bestIdx2 = -1;
        for (int b = f0; b < f1; ++b) {
            const int tag = s.idx[b];
            if (tag == kTriSkip) continue;
            const uint4 t0 = s.desc[2 * b], t1 = s.desc[2 * b + 1];
            const int dist = hamming256(q0, q1, t0, t1);
            if (dist > bestDist) continue;  // dist > TH_LOW || dist > bestDist (:1080), bestDist <= TH_LOW
            const float4 g = s.geo[b];
            if (!stereo1 && !(tag & kTriStereoBit)) {  // (:1089-1097)
                const float distex = epx - g.x, distey = epy - g.y;
                if (rfmaf(distex, distex, distey * distey) < g.w) continue;
            }
            bool ok = coarse;
            if (!ok && !(den == 0)) {
                const float num = lc + rfmaf(lb, g.y, la * g.x);
                const float dsqr = num * num / den;
                ok = (double)dsqr < 3.84 * (double)g.z;
            }
            if (ok) {
                bestIdx2 = tag & ~kTriStereoBit;
                bestDist = dist;
            }
        }
        if (bestIdx2 >= 0) M[i1] = bestIdx2;
    }
}

// Rotation histogram (:1147-1157), ComputeThreeMaxima and the filter
// (:1174-1193), nmatches; one workgroup per pair over rows [0, n1).
__global__ __launch_bounds__(256) void tri_finish_kernel(const plvi_triangulation_pair* __restrict__ pairs, int cap1,
                                                         int cap2, const plvi_keypoint* __restrict__ kps1_all,
                                                         const int* __restrict__ n1_all,
                                                         const plvi_keypoint* __restrict__ kps2_all,
                                                         int* __restrict__ m12_all, int* __restrict__ nmatches) {
    __shared__ int s_hist[kTriHisto], s_keep[3], s_count;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n1 = clampi(n1_all[p], 0, cap1);
    const bool ori = pairs[p].check_orientation != 0;
    const plvi_keypoint* K1 = kps1_all + (size_t)p * cap1;
    const plvi_keypoint* K2 = kps2_all + (size_t)p * cap2;
    int* M = m12_all + (size_t)p * cap1;
    if (tid < kTriHisto) s_hist[tid] = 0;
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (ori) {
        for (int i = tid; i < n1; i += 256) {
            const int m = M[i];
            if (m >= 0) atomicAdd(&s_hist[rot_bin(K1[i].angle - K2[m].angle, kTriHisto)], 1);
        }
        __syncthreads();
        if (tid == 0) three_maxima(s_hist, kTriHisto, s_keep);
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < n1; i += 256) {
        const int m = M[i];
        if (m < 0) continue;
        if (ori) {
            const int bin = rot_bin(K1[i].angle - K2[m].angle, kTriHisto);
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) {
                M[i] = -1;
                continue;
            }
        }
        ++cnt;
    }
    if (cnt) atomicAdd(&s_count, cnt);
    __syncthreads();
    if (tid == 0) nmatches[p] = s_count;
}

}  // namespace plvi

using namespace plvi;

extern "C" int plvi_search_for_triangulation_batch(
    int n_pairs, const plvi_triangulation_pair* d_pairs, int cap1, int cap2, int node_cap,
    const plvi_keypoint* d_kps1, const uint8_t* d_desc1, const int* d_n1, const int* d_node1, const int* d_off1,
    const int* d_nnodes1, const int* d_idx1, const uint8_t* d_has_point1, const float* d_uright1,
    const plvi_keypoint* d_kps2, const uint8_t* d_desc2, const int* d_n2, const int* d_node2, const int* d_off2,
    const int* d_nnodes2, const int* d_idx2, const uint8_t* d_has_point2, const float* d_uright2, int* d_matches12,
    int* d_nmatches, void* stream) {
    if (n_pairs < 0 || cap1 < 1 || cap2 < 1 || node_cap < 1) return PLVI_E_BADARG;
    if (cap1 >= kTriStereoBit || cap2 >= kTriStereoBit) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    if (!d_pairs || !d_kps1 || !d_desc1 || !d_n1 || !d_node1 || !d_off1 || !d_nnodes1 || !d_idx1 || !d_has_point1 ||
        !d_uright1 || !d_kps2 || !d_desc2 || !d_n2 || !d_node2 || !d_off2 || !d_nnodes2 || !d_idx2 ||
        !d_has_point2 || !d_uright2 || !d_matches12 || !d_nmatches)
        return PLVI_E_BADARG;
    const size_t smem = tri_smem(cap2, node_cap);
    if (!lds_fits<tri_match_kernel>(smem)) return PLVI_E_CAPACITY;  // before tri_fill_kernel is enqueued
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tri_fill_kernel, dim3(n_pairs, (cap1 + 255) / 256), dim3(256), 0, st, d_n1, cap1, d_matches12);
    // slices of KF1's list per pair: enough workgroups to cover the chip when
    // the batch alone does not, never more than the list has 512-thread strides
    const int strides = (cap1 + kTriThreads - 1) / kTriThreads;
    const int slices = std::max(1, std::min(strides, (512 + n_pairs - 1) / n_pairs));
    if (int rc = launch_lds<tri_match_kernel>(dim3(n_pairs, slices), dim3(kTriThreads), smem, st, d_pairs, cap1, cap2,
                                              node_cap, d_kps1, d_desc1, d_n1, d_node1, d_off1, d_nnodes1, d_idx1,
                                              d_has_point1, d_uright1, d_kps2, d_desc2, d_n2, d_node2, d_off2,
                                              d_nnodes2, d_idx2, d_has_point2, d_uright2, d_matches12))
        return rc;
    hipLaunchKernelGGL(tri_finish_kernel, dim3(n_pairs), dim3(256), 0, st, d_pairs, cap1, cap2, d_kps1, d_n1, d_kps2,
                       d_matches12, d_nmatches);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

// Single pair from host memory, synchronous.  Returns nmatches (>= 0) or an error.
extern "C" int plvi_search_for_triangulation(const plvi_triangulation_pair* pair, const plvi_keypoint* kps1,
                                             const uint8_t* desc1, int n1, const int* node1, const int* off1,
                                             int nnodes1, const int* idx1, const uint8_t* has_point1,
                                             const float* uright1, const plvi_keypoint* kps2, const uint8_t* desc2,
                                             int n2, const int* node2, const int* off2, int nnodes2, const int* idx2,
                                             const uint8_t* has_point2, const float* uright2, int* matches12) {
    if (!pair || n1 < 0 || n2 < 0 || nnodes1 < 0 || nnodes2 < 0) return PLVI_E_BADARG;
    if (n1 == 0) return 0;
    const int cap1 = n1, cap2 = std::max(n2, 1), node_cap = std::max(std::max(nnodes1, nnodes2), 1);
    const int len1 = nnodes1 ? off1[nnodes1] : 0, len2 = nnodes2 ? off2[nnodes2] : 0;
    if (len1 < 0 || len1 > cap1 || len2 < 0 || len2 > cap2) return PLVI_E_BADARG;
    int counts[5] = {n1, n2, nnodes1, nnodes2, 0};  // [4]: nmatches
    HostStage h;
    const auto P = h.in(pair, 1);
    const auto Cnt = h.inout(counts, 5);
    // one side: keypoints, descriptors, the feature vector (node, off, idx), has_point and uright
    struct Side {
        Staged<plvi_keypoint> k;
        Staged<uint8_t> d;
        Staged<int> node, off, idx;
        Staged<uint8_t> has;
        Staged<float> ur;
    };
    auto side = [&](const plvi_keypoint* kps, const uint8_t* desc, int n, const int* node, const int* off, int nnodes,
                    const int* idx, int len, const uint8_t* has_point, const float* uright) -> Side {
        return {h.in_or_zero(kps, n), h.in_or_zero(desc, n, 32), h.in_or_zero(node, nnodes, 1, node_cap),
                h.in_or_zero(off, nnodes ? nnodes + 1 : 0, 1, node_cap + 1), h.in_or_zero(idx, len, 1, n),
                h.in_or_zero(has_point, n), h.in_or_zero(uright, n)};
    };
    const Side a = side(kps1, desc1, n1, node1, off1, nnodes1, idx1, len1, has_point1, uright1);
    const Side b = side(kps2, desc2, n2, node2, off2, nnodes2, idx2, len2, has_point2, uright2);
    const auto M = h.out_or_scratch(matches12, n1);
    if (int rc = h.commit()) return rc;
    int* cnt = h.dev(Cnt);
    if (int rc = plvi_search_for_triangulation_batch(
            1, h.dev(P), cap1, cap2, node_cap, h.dev(a.k), h.dev(a.d), cnt, h.dev(a.node), h.dev(a.off), cnt + 2,
            h.dev(a.idx), h.dev(a.has), h.dev(a.ur), h.dev(b.k), h.dev(b.d), cnt + 1, h.dev(b.node), h.dev(b.off),
            cnt + 3, h.dev(b.idx), h.dev(b.has), h.dev(b.ur), h.dev(M), cnt + 4, nullptr))
        return rc;
    if (int rc = h.fetch()) return rc;
    return counts[4];
}
