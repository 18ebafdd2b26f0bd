// bow.hip — ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
// (src/ORBmatcher.cc:269-471) + ComputeThreeMaxima (:2304-2345), both the
// single-camera branch (F.Nleft == -1) and the two-camera one (:321-420: a
// best / second pair per camera, the right camera's match taken -- without
// its ratio test (`|| true`, :411) -- only when the left best passed TH_LOW,
// the enclosing `if` of the reference), batched over (KF, F) pairs.
//
// The two FeatureVectors (std::map<NodeId, vector<unsigned>>) arrive as CSR
// arrays sorted by node id.  Each F keypoint lives in exactly one node, so
// shared nodes are independent; the only sequential dependency is inside a
// node (a KF keypoint skips F keypoints already matched by an earlier KF
// keypoint of the same node).  Kernel: one workgroup (4 waves) per pair;
// thread 0 walks the two sorted node lists (the reference's lower_bound
// merge); the waves take shared nodes round-robin and walk each node's KF
// keypoints in order, the lanes evaluating the node's F keypoints in
// parallel (best / second with the reference's strict-< first-wins rule as
// a wave reduction).  Matches and the 30-bin rotation histogram live in
// LDS; ComputeThreeMaxima and the 10 % bin filter run at the end.
//
// ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)
// (:823-963) is search_by_bow_kf_kernel below, the same schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "grid_search.h"
#include "host_stage.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kBowTHLow = 50, kBowHisto = 30;

struct BowBest {
    int b1, p1, b2;  // best distance, its position in the node's F list, second best
};

__device__ __forceinline__ BowBest bow_combine(BowBest x, BowBest y) {
    BowBest r;
    const bool takeY = y.b1 < x.b1 || (y.b1 == x.b1 && y.p1 < x.p1);
    r.b1 = takeY ? y.b1 : x.b1;
    r.p1 = takeY ? y.p1 : x.p1;
    r.b2 = min(min(x.b2, y.b2), max(x.b1, y.b1));
    return r;
}

__global__ __launch_bounds__(256) void search_by_bow_kernel(
    float nnratio, int check_orientation, int kf_cap, int f_cap, int node_cap, const uint8_t* __restrict__ kf_desc,
    const float* __restrict__ kf_angle, const uint8_t* __restrict__ kf_live, const int* __restrict__ kf_node,
    const int* __restrict__ kf_off, const int* __restrict__ kf_nnodes, const int* __restrict__ kf_idx,
    const uint8_t* __restrict__ f_desc, const float* __restrict__ f_angle, const int* __restrict__ f_n,
    const int* __restrict__ f_node, const int* __restrict__ f_off, const int* __restrict__ f_nnodes,
    const int* __restrict__ f_idx, const int* __restrict__ f_nleft, int* __restrict__ match_kf,
    int* __restrict__ nmatches) {
    extern __shared__ __align__(16) int lds[];
    const int p = blockIdx.x;
    int* s_mk = lds;  // [f_cap] matched KF index or -1
    // [node_cap] shared (KF node, F node), carved at the next 8-byte boundary (bow_smem)
    int2* s_pairs = reinterpret_cast<int2*>(lds + ((f_cap + 1) & ~1));
    __shared__ int s_hist[kBowHisto], s_npairs, s_count, s_keep[3];
    const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int nF = min(f_n[p], f_cap);  // count contract (plvi_frontend.h)
    // F.Nleft (-1: one camera, every keypoint is "left")
    const int nLeft = (f_nleft && f_nleft[p] >= 0) ? f_nleft[p] : 0x7fffffff;
    const uint8_t* KD = kf_desc + (size_t)p * kf_cap * 32;
    const float* KA = kf_angle + (size_t)p * kf_cap;
    const uint8_t* KL = kf_live + (size_t)p * kf_cap;
    const int* KN = kf_node + (size_t)p * node_cap;
    const int* KO = kf_off + (size_t)p * (node_cap + 1);
    const int* KI = kf_idx + (size_t)p * kf_cap;
    const uint8_t* FD = f_desc + (size_t)p * f_cap * 32;
    const float* FA = f_angle + (size_t)p * f_cap;
    const int* FN = f_node + (size_t)p * node_cap;
    const int* FO = f_off + (size_t)p * (node_cap + 1);
    const int* FI = f_idx + (size_t)p * f_cap;
    for (int i = tid; i < nF; i += 256) s_mk[i] = -1;
    if (tid < kBowHisto) s_hist[tid] = 0;
    if (tid == 0) {
        // merge walk with the reference's lower_bound jumps (:289-448)
        const int nK = min(kf_nnodes[p], node_cap), nFn = min(f_nnodes[p], node_cap);
        int a = 0, b = 0, n = 0;
        while (a < nK && b < nFn) {
            const int ka = KN[a], fb = FN[b];
            if (ka == fb) {
                s_pairs[n++] = make_int2(a, b);
                ++a;
                ++b;
            } else if (ka < fb) {
                int lo = a, hi = nK;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (KN[mid] < fb) lo = mid + 1; else hi = mid; }
                a = lo;
            } else {
                int lo = b, hi = nFn;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (FN[mid] < ka) lo = mid + 1; else hi = mid; }
                b = lo;
            }
        }
        s_npairs = n;
        s_count = 0;
    }
    __syncthreads();
    const int npairs = s_npairs;
    for (int q = wv; q < npairs; q += 4) {
        const int2 pr = s_pairs[q];
        const int k0 = KO[pr.x], k1 = KO[pr.x + 1];
        const int f0 = FO[pr.y], nfn = FO[pr.y + 1] - f0;
        for (int a = k0; a < k1; ++a) {
            const int realIdxKF = KI[a];
            if (!KL[realIdxKF]) continue;
            const uint4* dk = reinterpret_cast<const uint4*>(KD + (size_t)realIdxKF * 32);
            const uint4 x0 = dk[0], x1 = dk[1];
            BowBest bb{256, 0x7fffffff, 256}, br{256, 0x7fffffff, 256};  // left / right camera
            for (int j = lane; j < nfn; j += 64) {
                const int realIdxF = FI[f0 + j];
                if (s_mk[realIdxF] >= 0) continue;
                const int d = hamming256(x0, x1, FD + (size_t)realIdxF * 32);
                // lane-local scan in list order with the reference's update rule
                BowBest& t = realIdxF < nLeft ? bb : br;
                if (d < t.b1) {
                    t.b2 = t.b1;
                    t.b1 = d;
                    t.p1 = j;
                } else if (d < t.b2) {
                    t.b2 = d;
                }
            }
            for (int s = 32; s > 0; s >>= 1) {
                BowBest o;
                o.b1 = __shfl_xor(bb.b1, s);
                o.p1 = __shfl_xor(bb.p1, s);
                o.b2 = __shfl_xor(bb.b2, s);
                bb = bow_combine(bb, o);
                if (nLeft != 0x7fffffff) {
                    o.b1 = __shfl_xor(br.b1, s);
                    o.p1 = __shfl_xor(br.p1, s);
                    o.b2 = __shfl_xor(br.b2, s);
                    br = bow_combine(br, o);
                }
            }
            if (bb.b1 <= kBowTHLow && lane == 0) {
                if ((float)bb.b1 < nnratio * (float)bb.b2) s_mk[FI[f0 + bb.p1]] = realIdxKF;
                // the right camera's best, inside the left TH_LOW test, no ratio test (:404-430)
                if (nLeft != 0x7fffffff && br.b1 <= kBowTHLow) s_mk[FI[f0 + br.p1]] = realIdxKF;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    // rotation histogram (:409-419) and ComputeThreeMaxima + filter (:450-468)
    if (check_orientation) {
        for (int i = tid; i < nF; i += 256) {
            const int k = s_mk[i];
            if (k < 0) continue;
            atomicAdd(&s_hist[rot_bin(KA[k] - FA[i], kBowHisto)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            three_maxima(s_hist, kBowHisto, s_keep);
        }
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < nF; i += 256) {
        int k = s_mk[i];
        if (k >= 0 && check_orientation) {
            const int bin = rot_bin(KA[k] - FA[i], kBowHisto);
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) k = -1;
        }
        match_kf[(size_t)p * f_cap + i] = k;
        cnt += k >= 0;
    }
    atomicAdd(&s_count, cnt);
    __syncthreads();
    if (tid == 0) nmatches[p] = s_count;
}

// s_mk rounded up to the int2 alignment of s_pairs; an odd f_cap makes 4*f_cap + 8*node_cap
// at most 65532, so the header's 65536 rule still bounds the rounded size
static size_t bow_smem(int f_cap, int node_cap) {
    return (size_t)((f_cap + 1) & ~1) * 4 + (size_t)node_cap * 8;
}

// ---------------------------------------------------------------------------
// ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>&
// vpMatches12) (src/ORBmatcher.cc:823-963), the loop-closing candidate search
// (LoopClosing.cc:823), single-camera branch (NLeft == -1 on both sides).
// Same schedule as above with the roles renamed: the table indexed by the
// result is KF1's (vpMatches12[idx1] = KF2 keypoint), the flags a match sets
// are KF2's (vbMatched2, :911) and both sides have a live byte.  What differs
// from the KF-Frame function, as the reference object shows: bestDist1 <
// TH_LOW is strict (cmp $0x31 / jg) and there is no second camera.
// LDS: matches12 [cap1] ints, the shared node pairs [node_cap] int2, one byte
// per KF2 keypoint (!live2 on entry, then vbMatched2 or-ed in).
__global__ __launch_bounds__(256) void search_by_bow_kf_kernel(
    float nnratio, int check_orientation, int cap1, int cap2, int node_cap, const uint8_t* __restrict__ desc1_all,
    const float* __restrict__ angle1_all, const uint8_t* __restrict__ live1_all, const int* __restrict__ n1_all,
    const int* __restrict__ node1_all, const int* __restrict__ off1_all, const int* __restrict__ nnodes1_all,
    const int* __restrict__ idx1_all, const uint8_t* __restrict__ desc2_all, const float* __restrict__ angle2_all,
    const uint8_t* __restrict__ live2_all, const int* __restrict__ n2_all, const int* __restrict__ node2_all,
    const int* __restrict__ off2_all, const int* __restrict__ nnodes2_all, const int* __restrict__ idx2_all,
    int* __restrict__ matches12, int* __restrict__ nmatches) {
    extern __shared__ __align__(16) int lds[];
    const int p = blockIdx.x;
    int* s_m12 = lds;                                                      // [cap1] KF2 index or -1
    int2* s_pairs = reinterpret_cast<int2*>(lds + ((cap1 + 1) & ~1));     // [node_cap] shared (KF1 node, KF2 node)
    unsigned char* s_skip2 = reinterpret_cast<unsigned char*>(s_pairs + node_cap);  // [cap2] !live2 | vbMatched2
    __shared__ int s_hist[kBowHisto], s_npairs, s_count, s_keep[3];
    const int tid = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    // count contract (plvi_frontend.h)
    const int n1 = min(max(n1_all[p], 0), cap1), n2 = min(max(n2_all[p], 0), cap2);
    const int nn1 = min(max(nnodes1_all[p], 0), node_cap), nn2 = min(max(nnodes2_all[p], 0), node_cap);
    const uint8_t* D1 = desc1_all + (size_t)p * cap1 * 32;
    const float* A1 = angle1_all + (size_t)p * cap1;
    const uint8_t* L1 = live1_all + (size_t)p * cap1;
    const int* N1 = node1_all + (size_t)p * node_cap;
    const int* O1 = off1_all + (size_t)p * (node_cap + 1);
    const int* I1 = idx1_all + (size_t)p * cap1;
    const uint8_t* D2 = desc2_all + (size_t)p * cap2 * 32;
    const float* A2 = angle2_all + (size_t)p * cap2;
    const uint8_t* L2 = live2_all + (size_t)p * cap2;
    const int* N2 = node2_all + (size_t)p * node_cap;
    const int* O2 = off2_all + (size_t)p * (node_cap + 1);
    const int* I2 = idx2_all + (size_t)p * cap2;
    // list lengths: an offset outside [0, length] is read as clamped, like a count
    const int len1 = nn1 ? min(max(O1[nn1], 0), cap1) : 0, len2 = nn2 ? min(max(O2[nn2], 0), cap2) : 0;
    for (int i = tid; i < n1; i += 256) s_m12[i] = -1;
    for (int i = tid; i < n2; i += 256) s_skip2[i] = L2[i] == 0;
    if (tid < kBowHisto) s_hist[tid] = 0;
    if (tid == 0) {
        // merge walk with the reference's lower_bound jumps (:851-940)
        int a = 0, b = 0, n = 0;
        while (a < nn1 && b < nn2) {
            const int ka = N1[a], kb = N2[b];
            if (ka == kb) {
                s_pairs[n++] = make_int2(a, b);
                ++a;
                ++b;
            } else if (ka < kb) {
                int lo = a, hi = nn1;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (N1[mid] < kb) lo = mid + 1; else hi = mid; }
                a = lo;
            } else {
                int lo = b, hi = nn2;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (N2[mid] < ka) lo = mid + 1; else hi = mid; }
                b = lo;
            }
        }
        s_npairs = n;
        s_count = 0;
    }
    __syncthreads();
    const int npairs = s_npairs;
    for (int q = wv; q < npairs; q += 4) {
        const int2 pr = s_pairs[q];
        const int k0 = min(max(O1[pr.x], 0), len1), k1 = min(max(O1[pr.x + 1], 0), len1);
        const int f0 = min(max(O2[pr.y], 0), len2), nfn = min(max(O2[pr.y + 1], 0), len2) - f0;
        for (int a = k0; a < k1; ++a) {
            const int idx1 = __builtin_amdgcn_readfirstlane(I1[a]);
            if (idx1 < 0 || idx1 >= n1 || !L1[idx1]) continue;  // not a keypoint / !pMP1 / isBad (:862-866)
            const uint4* dk = reinterpret_cast<const uint4*>(D1 + (size_t)idx1 * 32);
            const uint4 x0 = dk[0], x1 = dk[1];
            BowBest bb{256, 0x7fffffff, 256};
            for (int j = lane; j < nfn; j += 64) {
                const int idx2 = I2[f0 + j];
                if (idx2 < 0 || idx2 >= n2 || s_skip2[idx2]) continue;  // vbMatched2 || !pMP2 || isBad (:884-888)
                const int d = hamming256(x0, x1, D2 + (size_t)idx2 * 32);
                if (d < bb.b1) {
                    bb.b2 = bb.b1;
                    bb.b1 = d;
                    bb.p1 = j;
                } else if (d < bb.b2) {
                    bb.b2 = d;
                }
            }
            for (int s = 32; s > 0; s >>= 1) {
                BowBest o;
                o.b1 = __shfl_xor(bb.b1, s);
                o.p1 = __shfl_xor(bb.p1, s);
                o.b2 = __shfl_xor(bb.b2, s);
                bb = bow_combine(bb, o);
            }
            if (lane == 0 && bb.b1 < kBowTHLow && (float)bb.b1 < nnratio * (float)bb.b2) {  // (:906-911)
                const int bestIdx2 = I2[f0 + bb.p1];
                s_m12[idx1] = bestIdx2;
                s_skip2[bestIdx2] = 1;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    // rotation histogram (:913-923) and ComputeThreeMaxima + filter (:942-960)
    if (check_orientation) {
        for (int i = tid; i < n1; i += 256) {
            const int k = s_m12[i];
            if (k < 0) continue;
            atomicAdd(&s_hist[rot_bin(A1[i] - A2[k], kBowHisto)], 1);
        }
        __syncthreads();
        if (tid == 0) three_maxima(s_hist, kBowHisto, s_keep);
        __syncthreads();
    }
    int cnt = 0;
    for (int i = tid; i < n1; i += 256) {
        int k = s_m12[i];
        if (k >= 0 && check_orientation) {
            const int bin = rot_bin(A1[i] - A2[k], kBowHisto);
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) k = -1;
        }
        matches12[(size_t)p * cap1 + i] = k;
        cnt += k >= 0;
    }
    atomicAdd(&s_count, cnt);
    __syncthreads();
    if (tid == 0) nmatches[p] = s_count;
}

// matches12 rounded up to the int2 alignment of the node pairs
static size_t bow_kf_smem(int cap1, int cap2, int node_cap) {
    return (size_t)((cap1 + 1) & ~1) * 4 + (size_t)node_cap * 8 + (size_t)cap2;
}

}  // namespace plvi

using namespace plvi;

extern "C" int plvi_search_by_bow_stereo_batch(int n_pairs, float nnratio, int check_orientation, int kf_cap,
                                               int f_cap, int node_cap, const uint8_t* d_kf_desc,
                                               const float* d_kf_angle, const uint8_t* d_kf_live, const int* d_kf_node,
                                               const int* d_kf_off, const int* d_kf_nnodes, const int* d_kf_idx,
                                               const uint8_t* d_f_desc, const float* d_f_angle, const int* d_f_n,
                                               const int* d_f_node, const int* d_f_off, const int* d_f_nnodes,
                                               const int* d_f_idx, const int* d_f_nleft, int* d_match_kf,
                                               int* d_nmatches, void* stream) {
    if (n_pairs < 0 || kf_cap < 1 || f_cap < 1 || node_cap < 1) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    const size_t smem = bow_smem(f_cap, node_cap);
    if (smem > 64 * 1024) return PLVI_E_CAPACITY;
    return launch_lds<search_by_bow_kernel>(dim3(n_pairs), dim3(256), smem, (hipStream_t)stream, nnratio,
                                            check_orientation, kf_cap, f_cap, node_cap, d_kf_desc, d_kf_angle,
                                            d_kf_live, d_kf_node, d_kf_off, d_kf_nnodes, d_kf_idx, d_f_desc, d_f_angle,
                                            d_f_n, d_f_node, d_f_off, d_f_nnodes, d_f_idx, d_f_nleft, d_match_kf,
                                            d_nmatches);
}

extern "C" int plvi_search_by_bow_batch(int n_pairs, float nnratio, int check_orientation, int kf_cap, int f_cap,
                                        int node_cap, const uint8_t* d_kf_desc, const float* d_kf_angle,
                                        const uint8_t* d_kf_live, const int* d_kf_node, const int* d_kf_off,
                                        const int* d_kf_nnodes, const int* d_kf_idx, const uint8_t* d_f_desc,
                                        const float* d_f_angle, const int* d_f_n, const int* d_f_node,
                                        const int* d_f_off, const int* d_f_nnodes, const int* d_f_idx,
                                        int* d_match_kf, int* d_nmatches, void* stream) {
    return plvi_search_by_bow_stereo_batch(n_pairs, nnratio, check_orientation, kf_cap, f_cap, node_cap, d_kf_desc,
                                           d_kf_angle, d_kf_live, d_kf_node, d_kf_off, d_kf_nnodes, d_kf_idx, d_f_desc,
                                           d_f_angle, d_f_n, d_f_node, d_f_off, d_f_nnodes, d_f_idx, nullptr,
                                           d_match_kf, d_nmatches, stream);
}

// Single pair from host memory, synchronous.  Returns nmatches (>= 0) or an error.
extern "C" int plvi_search_by_bow_stereo(float nnratio, int check_orientation, const uint8_t* kf_desc,
                                         const float* kf_angle, const uint8_t* kf_live, int kf_n, const int* kf_node,
                                         const int* kf_off, int kf_nnodes, const int* kf_idx, const uint8_t* f_desc,
                                         const float* f_angle, int f_n, const int* f_node, const int* f_off,
                                         int f_nnodes, const int* f_idx, int f_nleft, int* match_kf) {
    if (f_nleft < -1 || f_nleft > f_n) return PLVI_E_BADARG;
    if (kf_n < 0 || f_n < 0 || kf_nnodes < 0 || f_nnodes < 0) return PLVI_E_BADARG;
    if (f_n == 0) return 0;
    const int kf_cap = std::max(kf_n, 1), f_cap = f_n, node_cap = std::max(std::max(kf_nnodes, f_nnodes), 1);
    const int nkf_idx = kf_nnodes ? kf_off[kf_nnodes] : 0, nf_idx = f_nnodes ? f_off[f_nnodes] : 0;
    if (nkf_idx > kf_cap || nf_idx > f_cap) return PLVI_E_BADARG;
    int counts[5] = {kf_nnodes, f_nnodes, f_n, f_nleft, 0};  // [4]: nmatches
    HostStage h;
    const auto KD = h.in_or_zero(kf_desc, kf_n, 32), KL = h.in_or_zero(kf_live, kf_n);
    const auto FD = h.in_or_zero(f_desc, f_n, 32);
    const auto KA = h.in_or_zero(kf_angle, kf_n), FA = h.in_or_zero(f_angle, f_n);
    const auto KN = h.in_or_zero(kf_node, kf_nnodes, 1, node_cap), FN = h.in_or_zero(f_node, f_nnodes, 1, node_cap);
    const auto KO = h.in_or_zero(kf_off, kf_nnodes + 1, 1, node_cap + 1);
    const auto FO = h.in_or_zero(f_off, f_nnodes + 1, 1, node_cap + 1);
    const auto KI = h.in_or_zero(kf_idx, nkf_idx, 1, kf_cap), FI = h.in_or_zero(f_idx, nf_idx, 1, f_cap);
    const auto M = h.out_or_scratch(match_kf, f_n), Cnt = h.inout(counts, 5);
    if (int rc = h.commit()) return rc;
    int* cnt = h.dev(Cnt);
    if (int rc = plvi_search_by_bow_stereo_batch(1, nnratio, check_orientation, kf_cap, f_cap, node_cap, h.dev(KD),
                                                 h.dev(KA), h.dev(KL), h.dev(KN), h.dev(KO), cnt, h.dev(KI), h.dev(FD),
                                                 h.dev(FA), cnt + 2, h.dev(FN), h.dev(FO), cnt + 1, h.dev(FI), cnt + 3,
                                                 h.dev(M), cnt + 4, nullptr))
        return rc;
    if (int rc = h.fetch()) return rc;
    return counts[4];
}

extern "C" int plvi_search_by_bow(float nnratio, int check_orientation, const uint8_t* kf_desc, const float* kf_angle,
                                  const uint8_t* kf_live, int kf_n, const int* kf_node, const int* kf_off,
                                  int kf_nnodes, const int* kf_idx, const uint8_t* f_desc, const float* f_angle,
                                  int f_n, const int* f_node, const int* f_off, int f_nnodes, const int* f_idx,
                                  int* match_kf) {
    return plvi_search_by_bow_stereo(nnratio, check_orientation, kf_desc, kf_angle, kf_live, kf_n, kf_node, kf_off,
                                     kf_nnodes, kf_idx, f_desc, f_angle, f_n, f_node, f_off, f_nnodes, f_idx, -1,
                                     match_kf);
}

extern "C" int plvi_search_by_bow_kf_batch(int n_pairs, float nnratio, int check_orientation, int cap1, int cap2,
                                           int node_cap, const uint8_t* d_desc1, const float* d_angle1,
                                           const uint8_t* d_live1, const int* d_n1, const int* d_node1,
                                           const int* d_off1, const int* d_nnodes1, const int* d_idx1,
                                           const uint8_t* d_desc2, const float* d_angle2, const uint8_t* d_live2,
                                           const int* d_n2, const int* d_node2, const int* d_off2,
                                           const int* d_nnodes2, const int* d_idx2, int* d_matches12, int* d_nmatches,
                                           void* stream) {
    if (n_pairs < 0 || cap1 < 1 || cap2 < 1 || node_cap < 1) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    if (!d_desc1 || !d_angle1 || !d_live1 || !d_n1 || !d_node1 || !d_off1 || !d_nnodes1 || !d_idx1 || !d_desc2 ||
        !d_angle2 || !d_live2 || !d_n2 || !d_node2 || !d_off2 || !d_nnodes2 || !d_idx2 || !d_matches12 || !d_nmatches)
        return PLVI_E_BADARG;
    const size_t smem = bow_kf_smem(cap1, cap2, node_cap);
    return launch_lds<search_by_bow_kf_kernel>(dim3(n_pairs), dim3(256), smem, (hipStream_t)stream, nnratio,
                                               check_orientation, cap1, cap2, node_cap, d_desc1, d_angle1, d_live1,
                                               d_n1, d_node1, d_off1, d_nnodes1, d_idx1, d_desc2, d_angle2, d_live2,
                                               d_n2, d_node2, d_off2, d_nnodes2, d_idx2, d_matches12, d_nmatches);
}

// Single pair from host memory, synchronous.  Returns nmatches (>= 0) or an error.
extern "C" int plvi_search_by_bow_kf(float nnratio, int check_orientation, const uint8_t* desc1, const float* angle1,
                                     const uint8_t* live1, int n1, const int* node1, const int* off1, int nnodes1,
                                     const int* idx1, const uint8_t* desc2, const float* angle2, const uint8_t* live2,
                                     int n2, const int* node2, const int* off2, int nnodes2, const int* idx2,
                                     int* matches12) {
    if (n1 < 0 || n2 < 0 || nnodes1 < 0 || nnodes2 < 0) return PLVI_E_BADARG;
    if (n1 > 0 && !matches12) return PLVI_E_BADARG;
    if (n1 == 0 || n2 == 0) {  // nothing to match: vpMatches12 is all NULL
        std::fill(matches12, matches12 + n1, -1);
        return 0;
    }
    if (!desc1 || !angle1 || !live1 || !desc2 || !angle2 || !live2) return PLVI_E_BADARG;
    if ((nnodes1 && (!node1 || !off1 || !idx1)) || (nnodes2 && (!node2 || !off2 || !idx2))) return PLVI_E_BADARG;
    const int node_cap = std::max(std::max(nnodes1, nnodes2), 1);
    const int len1 = nnodes1 ? off1[nnodes1] : 0, len2 = nnodes2 ? off2[nnodes2] : 0;
    if (len1 < 0 || len1 > n1 || len2 < 0 || len2 > n2) return PLVI_E_BADARG;
    int counts[5] = {n1, n2, nnodes1, nnodes2, 0};  // [4]: nmatches
    HostStage h;
    const auto D1 = h.in(desc1, n1, 32), L1 = h.in(live1, n1), D2 = h.in(desc2, n2, 32), L2 = h.in(live2, n2);
    const auto A1 = h.in(angle1, n1), A2 = h.in(angle2, n2);
    const auto N1 = h.in_or_zero(node1, nnodes1, 1, node_cap), N2 = h.in_or_zero(node2, nnodes2, 1, node_cap);
    const auto O1 = h.in_or_zero(off1, nnodes1 ? nnodes1 + 1 : 0, 1, node_cap + 1);
    const auto O2 = h.in_or_zero(off2, nnodes2 ? nnodes2 + 1 : 0, 1, node_cap + 1);
    const auto I1 = h.in_or_zero(idx1, len1, 1, n1), I2 = h.in_or_zero(idx2, len2, 1, n2);
    const auto M = h.out(matches12, n1), Cnt = h.inout(counts, 5);
    if (int rc = h.commit()) return rc;
    int* cnt = h.dev(Cnt);
    if (int rc = plvi_search_by_bow_kf_batch(1, nnratio, check_orientation, n1, n2, node_cap, h.dev(D1), h.dev(A1),
                                             h.dev(L1), cnt, h.dev(N1), h.dev(O1), cnt + 2, h.dev(I1), h.dev(D2),
                                             h.dev(A2), h.dev(L2), cnt + 1, h.dev(N2), h.dev(O2), cnt + 3, h.dev(I2),
                                             h.dev(M), cnt + 4, nullptr))
        return rc;
    if (int rc = h.fetch()) return rc;
    return counts[4];
}
