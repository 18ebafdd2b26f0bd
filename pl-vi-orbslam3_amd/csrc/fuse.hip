// fuse.hip — the duplicate searches of the back end as batched pure searches:
//   ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false)  (src/ORBmatcher.cc:1399-1610, mode 0)
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1612-1734, mode 1)
//   LineMatcher::Fuse(pKF, vpMapLines, th)                   (src/LineMatcher.cpp:373-485)
// with KeyFrame::GetFeaturesInArea / IsInImage / GetLinesInArea
// (src/KeyFrame.cc:1170-1249).  Inside one call the search for a point reads
// nothing an earlier iteration writes (the map mutation -- GetMapPoint,
// Replace, AddObservation, AddMapPoint -- starts after bestIdx / bestDist are
// known and touches none of the keyframe's keypoint, mvuRight, descriptor or
// grid tables), so every (keyframe, candidate) is independent: one lane per
// candidate, no greedy phase.  The pose products, PredictScale and every
// MapPoint / MapLine read stay with the caller.
//
// Points: the keyframe side is read through L2, not staged in LDS: a block
// serves kFuseChunk candidates of one pair and the grid is (chunks x pairs),
// so one keyframe against 8000 points runs on 125 CUs.  A window holds about
// ten keypoints; staging the whole keyframe (17 B per keypoint + 12 KB) per
// 64-candidate block would move more bytes than the walks read.  Without LDS
// neither capacity is bounded by it (DESIGN.md section 17 has the ISA figures).
// Lines: GetLinesInArea is a linear scan of every keyline by every candidate,
// so a block stages pt / angle / octave and the descriptors (48 B per keyline)
// in LDS once and every lane reads them at the same address (a broadcast).
#include <climits>

#include "grid_search.h"
#include "host_stage.h"
#include "plvi_math.h"

namespace plvi {

constexpr int kFuseChunk = PLVI_FUSE_CHUNK;  // candidates per block = one wave
static_assert(kFuseChunk == kWave, "one candidate per lane of one wave");

// Lane 0 adds the block's accepted rows to nfused[pair] (zeroed by the
// launcher on the same stream: integer adds, so the order is immaterial).
__device__ __forceinline__ void fuse_count(bool accepted, int* __restrict__ nfused) {
    const int c = __popcll(__ballot(accepted));
    if (threadIdx.x == 0 && c) atomicAdd(nfused, c);
}

__global__ __launch_bounds__(kFuseChunk) void fuse_points_kernel(
    plvi_fuse_params p, int nchunks, const plvi_keypoint* __restrict__ kps_all, const uint8_t* __restrict__ desc_all,
    const int* __restrict__ kp_n, int kp_cap, const float* __restrict__ uright_all,
    const int* __restrict__ cell_off_all, const int* __restrict__ cell_idx_all, const uint8_t* __restrict__ flags_all,
    const float* __restrict__ x3dc_all, const float* __restrict__ dist_all, const double* __restrict__ dot_all,
    const int* __restrict__ lvl_all, const uint8_t* __restrict__ mpdesc_all, const int* __restrict__ pt_n, int pt_cap,
    int* __restrict__ fuse_idx, int* __restrict__ fuse_dist, int* __restrict__ nfused) {
    const int pr = blockIdx.x / nchunks, chunk = blockIdx.x - pr * nchunks;
    const int np = max(min(pt_n[pr], pt_cap), 0), nk = max(min(kp_n[pr], kp_cap), 0);
    const int i = chunk * kFuseChunk + (int)threadIdx.x;
    const bool live = i < np;
    const size_t row = (size_t)pr * pt_cap + (live ? i : 0);
    int bestDist = p.mode ? INT_MAX : 256, bestIdx = -1;  // :1519 / :1694
    do {
        if (!live || nk == 0 || !(flags_all[row] & 1)) break;
        const float xc = x3dc_all[3 * row], yc = x3dc_all[3 * row + 1], zc = x3dc_all[3 * row + 2];
        if (zc < 0.0f) break;  // depth must be positive (:1459 / :1650)
        const float invz = 1 / zc;
        // Pinhole::project (Pinhole.cpp:36-42): no fused operation
        const float u = p.fx * xc / zc + p.cx, v = p.fy * yc / zc + p.cy;
        // KeyFrame::IsInImage: the upper bounds are strict
        if (!(u >= p.min_x && u < p.max_x && v >= p.min_y && v < p.max_y)) break;
        const float ur = rfmaf(-p.bf, invz, u);  // uv.x - bf*invz, one vfnmadd in the reference object (:1479)
        const float d3 = dist_all[3 * row], minDistance = dist_all[3 * row + 1], maxDistance = dist_all[3 * row + 2];
        if (d3 < minDistance || d3 > maxDistance) break;
        if (dot_all[row] < 0.5 * (double)d3) break;  // viewing angle, a double compare (:1496 / :1676)
        const int L = lvl_all[row];
        if (L < 0 || L >= p.nlevels) break;  // PredictScale clamps to [0, mnScaleLevels)
        const float radius = p.th * p.scale_factors[L];
        GridWindow w;
        if (!grid_window(p.min_x, p.min_y, p.inv_w, p.inv_h, u, v, radius, w)) break;
        const plvi_keypoint* K = kps_all + (size_t)pr * kp_cap;
        const uint8_t* D = desc_all + (size_t)pr * kp_cap * 32;
        const float* UR = uright_all ? uright_all + (size_t)pr * kp_cap : nullptr;
        const int* CO = cell_off_all + (size_t)pr * (kGridCells + 1);
        const int* CI = cell_idx_all + (size_t)pr * kp_cap;
        const uint4* dm = reinterpret_cast<const uint4*>(mpdesc_all + 32 * row);
        const uint4 m0 = dm[0], m1 = dm[1];
        // KeyFrame::GetFeaturesInArea order: grid column by column, one CSR range each
        for (int ix = w.nMinCellX; ix <= w.nMaxCellX; ++ix) {
            const int k0 = max(CO[ix * kGridRows + w.nMinCellY], 0);
            const int k1 = min(CO[ix * kGridRows + w.nMaxCellY + 1], kp_cap);
            for (int k = k0; k < k1; ++k) {
                const int i2 = CI[k];
                if ((unsigned)i2 >= (unsigned)nk) continue;  // not a keypoint of this keyframe
                const float kx = K[i2].x, ky = K[i2].y;
                if (!(fabsf(kx - u) < radius && fabsf(ky - v) < radius)) continue;
                const int kpLevel = K[i2].octave;
                if (kpLevel < L - 1 || kpLevel > L) continue;  // :1530 / :1701
                if (p.mode == 0) {
                    // the chi-square gate (:1533-1557); kpLevel is in [-1, nlevels) here, and a
                    // negative octave would index mvInvLevelSigma2[-1] in the reference: skipped
                    if (kpLevel < 0) continue;
                    const float ex = u - kx, ey = v - ky;
                    float e2 = rfmaf(ex, ex, ey * ey);  // ex*ex + ey*ey, the left product fused
                    const float kpr = UR ? UR[i2] : -1.0f;
                    if (kpr >= 0) {
                        const float er = ur - kpr;
                        e2 = rfmaf(er, er, e2);  // ... + er*er, fused
                        if ((double)(e2 * p.inv_level_sigma2[kpLevel]) > 7.8) continue;
                    } else {
                        if ((double)(e2 * p.inv_level_sigma2[kpLevel]) > 5.99) continue;
                    }
                }
                const int d = hamming256(m0, m1, D + (size_t)32 * i2);
                if (d < bestDist) {
                    bestDist = d;
                    bestIdx = i2;
                }
            }
        }
    } while (false);
    const bool accepted = bestIdx >= 0 && bestDist <= 50;  // TH_LOW (:1573 / :1716)
    if (live) {
        fuse_idx[row] = accepted ? bestIdx : -1;
        fuse_dist[row] = accepted ? bestDist : -1;
    }
    fuse_count(accepted, nfused + pr);
}

// LineMatcher::DescriptorDistance (src/LineMatcher.cpp:487-499): the >> 25
// quirk halves and floors every word's count.
__device__ __forceinline__ int line_distance(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return (__popc(a0.x ^ b0.x) >> 1) + (__popc(a0.y ^ b0.y) >> 1) + (__popc(a0.z ^ b0.z) >> 1) +
           (__popc(a0.w ^ b0.w) >> 1) + (__popc(a1.x ^ b1.x) >> 1) + (__popc(a1.y ^ b1.y) >> 1) +
           (__popc(a1.z ^ b1.z) >> 1) + (__popc(a1.w ^ b1.w) >> 1);
}

// Dynamic LDS per keyline: descriptor (32), pt.x, pt.y, angle, octave (4 each).
constexpr int kFuseLineBytes = 48;

__global__ __launch_bounds__(kFuseChunk) void fuse_lines_kernel(
    plvi_fuse_line_params p, int nchunks, const plvi_keyline* __restrict__ kl_all,
    const uint8_t* __restrict__ kldesc_all, const int* __restrict__ kl_n, int kl_cap,
    const uint8_t* __restrict__ flags_all, const float* __restrict__ spc_all, const float* __restrict__ epc_all,
    const float* __restrict__ dist_all, const double* __restrict__ dot_all, const int* __restrict__ lvl_all,
    const uint8_t* __restrict__ mldesc_all, const int* __restrict__ ml_n, int ml_cap, int* __restrict__ fuse_idx,
    int* __restrict__ fuse_dist, int* __restrict__ nfused) {
    extern __shared__ __align__(16) unsigned char lds[];
    const int pr = blockIdx.x / nchunks, chunk = blockIdx.x - pr * nchunks, tid = threadIdx.x;
    const int nl = max(min(ml_n[pr], ml_cap), 0), nk = max(min(kl_n[pr], kl_cap), 0);
    uint4* sdesc = reinterpret_cast<uint4*>(lds);                                  // [kl_cap][2]
    float* sx = reinterpret_cast<float*>(lds + (size_t)32 * kl_cap);               // [kl_cap]
    float* sy = sx + kl_cap;
    float* sang = sy + kl_cap;
    int* soct = reinterpret_cast<int*>(sang + kl_cap);
    {
        const plvi_keyline* KL = kl_all + (size_t)pr * kl_cap;
        const uint4* KD = reinterpret_cast<const uint4*>(kldesc_all + (size_t)pr * kl_cap * 32);
        for (int k = tid; k < nk; k += kFuseChunk) {
            sx[k] = KL[k].pt_x;
            sy[k] = KL[k].pt_y;
            sang[k] = KL[k].angle;
            soct[k] = KL[k].octave;
        }
        for (int k = tid; k < 2 * nk; k += kFuseChunk) sdesc[k] = KD[k];
    }
    __syncthreads();
    const int i = chunk * kFuseChunk + tid;
    const bool live = i < nl;
    const size_t row = (size_t)pr * ml_cap + (live ? i : 0);
    int bestDist = INT_MAX, bestIdx = -1;  // :450
    do {
        if (!live || !(flags_all[row] & 1)) break;
        const float X1 = spc_all[3 * row], Y1 = spc_all[3 * row + 1], Z1 = spc_all[3 * row + 2];
        const float X2 = epc_all[3 * row], Y2 = epc_all[3 * row + 1], Z2 = epc_all[3 * row + 2];
        if (Z1 < 0.0f || Z2 < 0.0f) break;  // :408
        // u = fx*X*invz + cx: the reference object fuses (fx*X) * invz + cx (:412-413, :421-422)
        const float invz1 = 1.0f / Z1;
        const float u1 = rfmaf(p.fx * X1, invz1, p.cx), v1 = rfmaf(p.fy * Y1, invz1, p.cy);
        if (u1 < p.min_x || u1 > p.max_x) break;  // both ends inclusive, unlike IsInImage
        if (v1 < p.min_y || v1 > p.max_y) break;
        const float invz2 = 1.0f / Z2;
        const float u2 = rfmaf(p.fx * X2, invz2, p.cx), v2 = rfmaf(p.fy * Y2, invz2, p.cy);
        if (u2 < p.min_x || u2 > p.max_x) break;
        if (v2 < p.min_y || v2 > p.max_y) break;
        const float d3 = dist_all[3 * row], minDistance = dist_all[3 * row + 1], maxDistance = dist_all[3 * row + 2];
        if (d3 < minDistance || d3 > maxDistance) break;
        if (dot_all[row] < 0.5 * (double)d3) break;
        const int L = lvl_all[row];
        if (L < 0 || L >= p.nlevels) break;
        const float r = p.th * p.scale_factors[L];
        // KeyFrame::GetLinesInArea(u1, v1, u2, v2, r) with the header's default levels (-1, -1: no
        // level filter), a scan of every keyline in index order (KeyFrame.cc:1170-1198)
        const double mx = (double)(u1 + u2), my = (double)(v1 + v2);  // float sums, widened
        const float r2 = r * r;
        const float slope0 = (v1 - v2) / (u1 - u2);  // +-inf or NaN where u1 == u2: the reference's behaviour
        const double slope_max = (double)r * 0.01;
        const uint4* dm = reinterpret_cast<const uint4*>(mldesc_all + 32 * row);
        const uint4 m0 = dm[0], m1 = dm[1];
        for (int k = 0; k < nk; ++k) {
            const double dx = rfma(0.5, mx, -(double)sx[k]), dy = rfma(0.5, my, -(double)sy[k]);
            const float distance = (float)rfma(dx, dx, dy * dy);
            if (distance > r2) continue;
            const float slope = slope0 - sang[k];
            if ((double)slope > slope_max) continue;  // no absolute value in the reference
            const int klLevel = soct[k];
            if (klLevel < L - 1 || klLevel > L) continue;  // :455
            const int d = line_distance(m0, m1, sdesc[2 * k], sdesc[2 * k + 1]);
            if (d < bestDist) {
                bestDist = d;
                bestIdx = k;
            }
        }
    } while (false);
    const bool accepted = bestIdx >= 0 && bestDist <= 50;  // :467
    if (live) {
        fuse_idx[row] = accepted ? bestIdx : -1;
        fuse_dist[row] = accepted ? bestDist : -1;
    }
    fuse_count(accepted, nfused + pr);
}

static bool fuse_params_ok(const plvi_fuse_params* p) {
    return p && p->nlevels >= 1 && p->nlevels <= 16 && (p->mode == 0 || p->mode == 1);
}

static bool fuse_line_params_ok(const plvi_fuse_line_params* p) { return p && p->nlevels >= 1 && p->nlevels <= 16; }

// Blocks of a (chunks x pairs) launch, 0 where they exceed a grid dimension.
static int fuse_blocks(int n_pairs, int cap, int& nchunks) {
    nchunks = (int)(((long long)cap + kFuseChunk - 1) / kFuseChunk);
    const long long blocks = (long long)nchunks * n_pairs;
    return blocks <= INT_MAX ? (int)blocks : 0;
}

}  // namespace plvi

using namespace plvi;

extern "C" int plvi_fuse_points_batch(int n_pairs, const plvi_fuse_params* p, const plvi_keypoint* d_kps,
                                      const uint8_t* d_desc, const int* d_kp_n, int kp_cap, const float* d_uright,
                                      const int* d_cell_off, const int* d_cell_idx, const uint8_t* d_flags,
                                      const float* d_x3dc, const float* d_dist, const double* d_dot, const int* d_level,
                                      const uint8_t* d_mp_desc, const int* d_pt_n, int pt_cap, int* d_fuse_idx,
                                      int* d_fuse_dist, int* d_nfused, void* stream) {
    if (!fuse_params_ok(p) || n_pairs < 0 || kp_cap < 1 || pt_cap < 1 || kp_cap > 65535) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    if (!d_kps || !d_desc || !d_kp_n || !d_cell_off || !d_cell_idx || !d_flags || !d_x3dc || !d_dist || !d_dot ||
        !d_level || !d_mp_desc || !d_pt_n || !d_fuse_idx || !d_fuse_dist || !d_nfused)
        return PLVI_E_BADARG;
    int nchunks;
    const int blocks = fuse_blocks(n_pairs, pt_cap, nchunks);
    if (!blocks) return PLVI_E_CAPACITY;
    PLVI_CHECK(hipMemsetAsync(d_nfused, 0, 4 * (size_t)n_pairs, (hipStream_t)stream));
    hipLaunchKernelGGL(fuse_points_kernel, dim3(blocks), dim3(kFuseChunk), 0, (hipStream_t)stream, *p, nchunks, d_kps,
                       d_desc, d_kp_n, kp_cap, d_uright, d_cell_off, d_cell_idx, d_flags, d_x3dc, d_dist, d_dot,
                       d_level, d_mp_desc, d_pt_n, pt_cap, d_fuse_idx, d_fuse_dist, d_nfused);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_fuse_lines_batch(int n_pairs, const plvi_fuse_line_params* p, const plvi_keyline* d_kl,
                                     const uint8_t* d_kl_desc, const int* d_kl_n, int kl_cap, const uint8_t* d_flags,
                                     const float* d_spc, const float* d_epc, const float* d_dist, const double* d_dot,
                                     const int* d_level, const uint8_t* d_ml_desc, const int* d_ml_n, int ml_cap,
                                     int* d_fuse_idx, int* d_fuse_dist, int* d_nfused, void* stream) {
    if (!fuse_line_params_ok(p) || n_pairs < 0 || kl_cap < 1 || ml_cap < 1) return PLVI_E_BADARG;
    if (n_pairs == 0) return PLVI_OK;
    if (!d_kl || !d_kl_desc || !d_kl_n || !d_flags || !d_spc || !d_epc || !d_dist || !d_dot || !d_level ||
        !d_ml_desc || !d_ml_n || !d_fuse_idx || !d_fuse_dist || !d_nfused)
        return PLVI_E_BADARG;
    int nchunks;
    const int blocks = fuse_blocks(n_pairs, ml_cap, nchunks);
    const size_t smem = (size_t)kFuseLineBytes * kl_cap;
    // (the LDS bound here too: a refusal comes before anything is enqueued)
    if (!blocks || !lds_fits<fuse_lines_kernel>(smem)) return PLVI_E_CAPACITY;
    PLVI_CHECK(hipMemsetAsync(d_nfused, 0, 4 * (size_t)n_pairs, (hipStream_t)stream));
    return launch_lds<fuse_lines_kernel>(dim3(blocks), dim3(kFuseChunk), smem, (hipStream_t)stream, *p, nchunks, d_kl,
                                         d_kl_desc, d_kl_n, kl_cap, d_flags, d_spc, d_epc, d_dist, d_dot, d_level,
                                         d_ml_desc, d_ml_n, ml_cap, d_fuse_idx, d_fuse_dist, d_nfused);
}

// One pair from host memory, synchronous (grid built on the device).
extern "C" int plvi_fuse_points(const plvi_fuse_params* p, const plvi_keypoint* kps, const uint8_t* desc, int n_kp,
                                const float* uright, const uint8_t* flags, const float* x3dc, const float* dist,
                                const double* dot, const int* level, const uint8_t* mp_desc, int n_pt, int* fuse_idx,
                                int* fuse_dist) {
    if (!fuse_params_ok(p) || n_kp < 0 || n_pt < 0 || (n_kp > 0 && (!kps || !desc))) return PLVI_E_BADARG;
    if (n_pt > 0 && (!flags || !x3dc || !dist || !dot || !level || !mp_desc || !fuse_idx || !fuse_dist))
        return PLVI_E_BADARG;
    if (n_kp > 8192) return PLVI_E_BADARG;  // plvi_assign_grid_batch
    if (n_pt == 0) return 0;
    if (n_kp == 0) {
        for (int i = 0; i < n_pt; ++i) fuse_idx[i] = fuse_dist[i] = -1;
        return 0;
    }
    const int kc = n_kp, pc = n_pt;
    int counts[3] = {n_kp, n_pt, 0};  // [2]: nfused
    HostStage st;
    const auto K = st.in(kps, kc);
    const auto D = st.in(desc, kc, 32), F = st.in(flags, pc), MD = st.in(mp_desc, pc, 32);
    const auto U = st.in(uright, kc), X = st.in(x3dc, pc, 3), S = st.in(dist, pc, 3);
    const auto T = st.in(dot, pc);
    const auto CO = st.scratch<int>(kGridCells + 1), CI = st.scratch<int>(kc), L = st.in(level, pc);
    const auto I = st.out(fuse_idx, pc), Di = st.out(fuse_dist, pc), N = st.inout(counts, 3);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    const plvi_grid_params gp{p->min_x, p->min_y, p->inv_w, p->inv_h};
    if (int rc = plvi_assign_grid_batch(st.dev(K), dN, kc, 1, &gp, st.dev(CO), st.dev(CI), nullptr)) return rc;
    if (int rc = plvi_fuse_points_batch(1, p, st.dev(K), st.dev(D), dN, kc, st.dev(U), st.dev(CO), st.dev(CI),
                                        st.dev(F), st.dev(X), st.dev(S), st.dev(T), st.dev(L), st.dev(MD), dN + 1, pc,
                                        st.dev(I), st.dev(Di), dN + 2, nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[2];
}

extern "C" int plvi_fuse_lines(const plvi_fuse_line_params* p, const plvi_keyline* kl, const uint8_t* kl_desc,
                               int n_kl, const uint8_t* flags, const float* spc, const float* epc, const float* dist,
                               const double* dot, const int* level, const uint8_t* ml_desc, int n_ml, int* fuse_idx,
                               int* fuse_dist) {
    if (!fuse_line_params_ok(p) || n_kl < 0 || n_ml < 0 || (n_kl > 0 && (!kl || !kl_desc))) return PLVI_E_BADARG;
    if (n_ml > 0 &&
        (!flags || !spc || !epc || !dist || !dot || !level || !ml_desc || !fuse_idx || !fuse_dist))
        return PLVI_E_BADARG;
    if (n_ml == 0) return 0;
    if (n_kl == 0) {
        for (int i = 0; i < n_ml; ++i) fuse_idx[i] = fuse_dist[i] = -1;
        return 0;
    }
    const int kc = n_kl, pc = n_ml;
    int counts[3] = {n_kl, n_ml, 0};  // [2]: nfused
    HostStage st;
    const auto K = st.in(kl, kc);
    const auto D = st.in(kl_desc, kc, 32), F = st.in(flags, pc), MD = st.in(ml_desc, pc, 32);
    const auto A = st.in(spc, pc, 3), B = st.in(epc, pc, 3), S = st.in(dist, pc, 3);
    const auto T = st.in(dot, pc);
    const auto L = st.in(level, pc), I = st.out(fuse_idx, pc), Di = st.out(fuse_dist, pc), N = st.inout(counts, 3);
    if (int rc = st.commit()) return rc;
    int* dN = st.dev(N);
    if (int rc = plvi_fuse_lines_batch(1, p, st.dev(K), st.dev(D), dN, kc, st.dev(F), st.dev(A), st.dev(B), st.dev(S),
                                       st.dev(T), st.dev(L), st.dev(MD), dN + 1, pc, st.dev(I), st.dev(Di), dN + 2,
                                       nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    return counts[2];
}
