// feature_refresh.hip — the map-feature refresh on the device:
//   MapPoint::UpdateNormalAndDepth          src/MapPoint.cc:427-494 (NLeft == -1)
//   MapLine::UpdateNormalAndDepth           src/MapLine.cc:339-382
//   ComputeDistinctiveDescriptors           through plvi_distinctive_descriptors_batch (distinctive.hip)
// for a list of pool ids, writing the pool columns normal / dist / desc in
// place (include/plvi_frontend.h, "Feature refresh").
//
// Arithmetic as the reference objects do it (MapPoint.cc.o, MapLine.cc.o,
// pinned by tests/test_ref_objects_feature_refresh.py): the double midpoint of
// a line, cv::norm narrowed to float for dist, n converted to double ahead of
// operator/(Mat, double), one float multiply and one float divide for the two
// distances.  Parity unpinned inside OpenCV: cv::norm (exact float squares
// summed in double) and the subtract as frustum.hip takes them; normal +
// normali / s as scaleAdd(normali, (float)(1 / s), normal), whose scalar tail
// PLVI_COMPAT_SCALEADD_FMA contracts.
//
// Work: the observers of a feature are independent gathers (obs_kf -> ow, 12
// bytes) in front of a sum that must run in list order.  A group of G lanes (8,
// 16 or 32 by max_obs) takes one id: a lane per observer for the gather, the
// reciprocal norm and, unfused, the product; then every lane of the group adds
// the G terms in order out of its neighbours' registers.  A longer list is
// walked G entries at a time by its own group, so it holds up nobody else's
// wave.  The same pass finds ref_kf's entry and, for DESC, writes the rows of
// the CSR that the distinctive kernels read.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "block_prims.h"
#include "host_stage.h"
#include "plvi_common.h"
#include "plvi_math.h"

namespace plvi {

namespace {

constexpr int kCsrThreads = 1024;  // one workgroup scans the list lengths
constexpr int kCsrPer = 4;         // ids per thread and tile
constexpr int kCsrTile = kCsrThreads * kCsrPer;
constexpr int kWalkThreads = 256;
constexpr int kScatterThreads = 256;

struct RefreshArgs {
    int kf_cap, cap;
    const uint8_t* kf_bad;
    const float* ow;
    const int* cnt;
    const uint8_t* info;
    int n;
    const uint8_t* bad;
    const int* obs_off;
    const int* obs_kf;
    const int* obs_idx;
    const float* pos;
    const double* sep;
    const int* ref_kf;
    int lines, what, fma_form, n_levels, max_obs, row_cap;
    const int* ids;
    int n_ids;
    float* normal;
    float* dist;
    uint8_t* state;
    int* csr_off;
    int* csr_row;
    int* n_rows;
    int* err;
    float scale[PLVI_REFRESH_MAX_LEVELS];
};

// cv::norm(v) (NORM_L2, 3x1 float): exact float squares summed in double (frustum.hip).
__device__ __forceinline__ double cv_norm3(float a, float b, float c) {
    double s = 0.0;
    s += (double)a * a;
    s += (double)b * b;
    s += (double)c * c;
    return __builtin_sqrt(s);
}

// the list both functions walk: empty for an id outside the pool and for a bad feature
__device__ __forceinline__ int list_len(const RefreshArgs& a, int id) {
    if (!in_range(id, a.n) || a.bad[id]) return 0;
    return clampi(a.obs_off[id + 1] - a.obs_off[id], 0, a.max_obs);
}

// csr_off [n_ids + 1] = the exclusive scan of the list lengths, *n_rows its full sum.  A sum above
// row_cap leaves every list empty: nothing downstream reads or writes a row then.
__global__ __launch_bounds__(kCsrThreads) void refresh_csr_kernel(const RefreshArgs a) {
    __shared__ int s_wave[kCsrThreads / kWave];
    const int tid = threadIdx.x;
    int base = 0;
    for (int t0 = 0; t0 < a.n_ids; t0 += kCsrTile) {
        int len[kCsrPer], sum = 0;
#pragma unroll
        for (int k = 0; k < kCsrPer; ++k) {
            const int i = t0 + tid * kCsrPer + k;
            len[k] = i < a.n_ids ? list_len(a, a.ids[i]) : 0;
            sum += len[k];
        }
        int tot;
        int run = base + block_scan<kCsrThreads / kWave>(sum, s_wave, tid, &tot);
#pragma unroll
        for (int k = 0; k < kCsrPer; ++k) {
            const int i = t0 + tid * kCsrPer + k;
            if (i < a.n_ids) a.csr_off[i] = run;
            run += len[k];
        }
        base += tot;
    }
    const bool over = base > a.row_cap;
    if (over) {
        __syncthreads();
        for (int i = tid; i < a.n_ids; i += kCsrThreads) a.csr_off[i] = 0;
    }
    if (tid == 0) {
        a.csr_off[a.n_ids] = over ? 0 : base;
        *a.n_rows = base;
        if (over) atomicOr(a.err, PLVI_REFRESH_ERR_ROWS);
    }
}

template <int G>
__global__ __launch_bounds__(kWalkThreads) void refresh_walk_kernel(const RefreshArgs a) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), sub = lane & (G - 1), gbase = lane & ~(G - 1);
    const unsigned long long gmask = G == 64 ? ~0ull : (1ull << G) - 1;
    const int i = (int)(((long long)blockIdx.x * kWalkThreads + tid) / G);
    const bool live = i < a.n_ids;
    const bool do_normal = a.what & PLVI_REFRESH_NORMAL, do_desc = a.what & PLVI_REFRESH_DESC;
    const int id = live ? a.ids[i] : -1;
    const int len = live ? list_len(a, id) : 0;
    const int o0 = len ? a.obs_off[id] : 0;
    int r0 = 0, rlen = 0;
    if (do_desc && live) {
        r0 = a.csr_off[i];
        rlen = a.csr_off[i + 1] - r0;  // len, or 0 after ERR_ROWS
    }
    float P[3] = {0.f, 0.f, 0.f};
    int ref = -1;
    if (do_normal && len) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            P[c] = a.lines ? (float)((a.sep[6 * (size_t)id + c] + a.sep[6 * (size_t)id + 3 + c]) * 0.5)
                           : a.pos[3 * (size_t)id + c];
        ref = a.ref_kf[id];
    }
    float acc[3] = {0.f, 0.f, 0.f};
    int n = 0, ref_idx = 0;  // observations[pRefKF] of an absent key: the default tuple, index 0
    bool found = false;
    for (int base = 0; __any(base < len); base += G) {
        const int j = base + sub;
        int kf = -1, idx = -1;
        if (j < len) {
            kf = a.obs_kf[o0 + j];
            idx = a.obs_idx ? a.obs_idx[o0 + j] : -1;
        }
        const bool valid = in_range(kf, a.kf_cap);
        if (do_desc && j < rlen) {
            const bool ok = valid && !a.kf_bad[kf] && in_range(idx, clampi(a.cnt[kf], 0, a.cap));
            a.csr_row[r0 + j] = ok ? kf * a.cap + idx : -1;
        }
        if (!do_normal) continue;
        float v[3] = {0.f, 0.f, 0.f}, alpha = 0.f;
        if (valid && len) {
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = P[c] - a.ow[3 * (size_t)kf + c];
            alpha = (float)(1.0 / cv_norm3(d[0], d[1], d[2]));
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = a.fma_form ? d[c] : d[c] * alpha;
        }
        const unsigned long long vm = (__ballot(valid) >> gbase) & gmask;
        const unsigned long long rm = (__ballot(valid && kf == ref) >> gbase) & gmask;
        const int first = __shfl(idx, rm ? __builtin_ctzll(rm) : 0, G);
        if (!found && rm) {
            found = true;
            ref_idx = first;
        }
        // the ordered sum: every lane of the group adds the same terms
        const int clen = min(G, len - base);
        for (int t = 0; __any(t < clen); ++t) {
            const float x0 = __shfl(v[0], t, G), x1 = __shfl(v[1], t, G), x2 = __shfl(v[2], t, G);
            const float xa = __shfl(alpha, t, G);
            if (t < clen && ((vm >> t) & 1)) {
                if (a.fma_form) {
                    acc[0] = rfmaf(x0, xa, acc[0]);
                    acc[1] = rfmaf(x1, xa, acc[1]);
                    acc[2] = rfmaf(x2, xa, acc[2]);
                } else {
                    acc[0] = x0 + acc[0];
                    acc[1] = x1 + acc[1];
                    acc[2] = x2 + acc[2];
                }
                ++n;
            }
        }
    }
    if (sub != 0 || !live) return;
    uint8_t st = 0;
    if (do_normal && n > 0) {
        int e = 0, level = 0;
        if (!in_range(ref, a.kf_cap)) {
            e = PLVI_REFRESH_ERR_REF;
        } else if (!a.lines) {
            if (!in_range(ref_idx, clampi(a.cnt[ref], 0, a.cap))) e = PLVI_REFRESH_ERR_KEYPOINT;
            else level = a.info[ref * a.cap + ref_idx] & 63;
        }
        if (!e && level >= a.n_levels) e = PLVI_REFRESH_ERR_LEVEL;
        if (e) {
            atomicOr(a.err, e);
        } else {
            const float rn = (float)(1.0 / (double)n);
            const float d = (float)cv_norm3(P[0] - a.ow[3 * (size_t)ref], P[1] - a.ow[3 * (size_t)ref + 1],
                                            P[2] - a.ow[3 * (size_t)ref + 2]);
            const float dmax = d * a.scale[level];
            const float dmin = dmax / a.scale[a.n_levels - 1];
#pragma unroll
            for (int c = 0; c < 3; ++c) a.normal[3 * (size_t)id + c] = acc[c] * rn;
            a.dist[2 * (size_t)id] = dmin;
            a.dist[2 * (size_t)id + 1] = dmax;
            st = PLVI_REFRESH_NORMAL;
        }
    }
    a.state[i] = st;
}

// desc[id] = chosen[i] where a descriptor was chosen; a dword per thread
__global__ __launch_bounds__(kScatterThreads) void refresh_scatter_kernel(const int* __restrict__ ids, int n_ids, int n,
                                                                          const int* __restrict__ best_pos,
                                                                          const uint32_t* __restrict__ chosen,
                                                                          uint32_t* desc, uint8_t* state) {
    const long long t = (long long)blockIdx.x * kScatterThreads + threadIdx.x;
    const int i = (int)(t >> 3), w = (int)(t & 7);
    if (i >= n_ids || best_pos[i] < 0) return;
    const int id = ids[i];
    if (!in_range(id, n)) return;
    desc[8 * (size_t)id + w] = chosen[8 * (size_t)i + w];
    if (w == 0) state[i] |= PLVI_REFRESH_DESC;
}

template <int G>
void launch_walk(const RefreshArgs& a, hipStream_t st) {
    const long long threads = (long long)a.n_ids * G;
    hipLaunchKernelGGL(refresh_walk_kernel<G>, dim3((unsigned)((threads + kWalkThreads - 1) / kWalkThreads)),
                       dim3(kWalkThreads), 0, st, a);
}

struct ScratchLayout {
    size_t off, row, pos, median, chosen, total;
};

ScratchLayout scratch_layout(int n_ids, int row_cap) {
    ScratchLayout s;
    s.off = 0;
    s.row = s.off + up256(4 * ((size_t)n_ids + 1));
    s.pos = s.row + up256(4 * (size_t)row_cap);
    s.median = s.pos + up256(4 * (size_t)n_ids);
    s.chosen = s.median + up256(4 * (size_t)n_ids);
    s.total = s.chosen + up256(32 * (size_t)n_ids);
    return s;
}

int refresh_validate(const plvi_refresh_keyframes* kf, const plvi_local_map_pool* pool, const plvi_ba_features* feat,
                     const plvi_eg_features* ref, const plvi_refresh_params* p, const int* ids, int n_ids,
                     const plvi_refresh_outputs* out) {
    if (!kf || !pool || !p || !out || n_ids < 0 || kf->kf_cap < 0 || kf->cap < 0 || pool->n < 0) return PLVI_E_BADARG;
    if (p->kind != PLVI_REFRESH_POINTS && p->kind != PLVI_REFRESH_LINES) return PLVI_E_BADARG;
    const int all = PLVI_REFRESH_NORMAL | PLVI_REFRESH_DESC;
    if (!p->what || (p->what & ~all)) return PLVI_E_BADARG;
    const bool normal = p->what & PLVI_REFRESH_NORMAL, desc = p->what & PLVI_REFRESH_DESC;
    const bool points = p->kind == PLVI_REFRESH_POINTS;
    if (p->n_levels < 1 || p->n_levels > PLVI_REFRESH_MAX_LEVELS || p->max_obs < 0) return PLVI_E_BADARG;
    if (desc && p->row_cap < 0) return PLVI_E_BADARG;
    if (!out->state || !out->n_rows || !out->err || (n_ids > 0 && !ids)) return PLVI_E_BADARG;
    if (!pool->bad || !pool->obs_off || !pool->obs_kf) return PLVI_E_BADARG;
    const bool need_idx = desc || (normal && points);
    if (need_idx && (!feat || !feat->obs_idx || !kf->cnt)) return PLVI_E_BADARG;
    if (normal) {
        if (!kf->ow || !ref || !ref->ref_kf || !out->normal || !out->dist) return PLVI_E_BADARG;
        if (points ? !pool->pos || !kf->info : !pool->sep) return PLVI_E_BADARG;
    }
    if (desc && (!kf->bad || !kf->desc || !out->desc)) return PLVI_E_BADARG;
    if (p->max_obs > PLVI_DISTINCTIVE_MAX_OBS) return PLVI_E_CAPACITY;
    if ((long long)kf->kf_cap * kf->cap > INT_MAX || (long long)n_ids * p->max_obs > INT_MAX) return PLVI_E_CAPACITY;
    return PLVI_OK;
}

}  // namespace

}  // namespace plvi

using namespace plvi;

extern "C" size_t plvi_feature_refresh_scratch_bytes(int n_ids, int row_cap) {
    if (n_ids < 0 || row_cap < 0) return 0;
    return scratch_layout(n_ids, row_cap).total;
}

extern "C" int plvi_feature_refresh_batch(const plvi_refresh_keyframes* kf, const plvi_local_map_pool* pool,
                                          const plvi_ba_features* feat, const plvi_eg_features* ref,
                                          const plvi_refresh_params* params, const int* d_ids, int n_ids,
                                          const plvi_refresh_outputs* out, void* d_scratch, size_t scratch_bytes,
                                          void* stream) {
    if (int rc = refresh_validate(kf, pool, feat, ref, params, d_ids, n_ids, out)) return rc;
    const bool desc = params->what & PLVI_REFRESH_DESC;
    const ScratchLayout lay = scratch_layout(n_ids, desc ? params->row_cap : 0);
    if (desc && n_ids > 0 && (!d_scratch || scratch_bytes < lay.total)) return PLVI_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    PLVI_CHECK(hipMemsetAsync(out->n_rows, 0, sizeof(int), st));
    PLVI_CHECK(hipMemsetAsync(out->err, 0, sizeof(int), st));
    if (n_ids == 0) return PLVI_OK;

    RefreshArgs a;
    memset(&a, 0, sizeof a);
    a.kf_cap = kf->kf_cap, a.cap = kf->cap, a.kf_bad = kf->bad, a.ow = kf->ow, a.cnt = kf->cnt, a.info = kf->info;
    a.n = pool->n, a.bad = pool->bad, a.obs_off = pool->obs_off, a.obs_kf = pool->obs_kf;
    a.obs_idx = feat ? feat->obs_idx : nullptr;
    a.pos = pool->pos, a.sep = pool->sep, a.ref_kf = ref ? ref->ref_kf : nullptr;
    a.lines = params->kind == PLVI_REFRESH_LINES, a.what = params->what;
    a.fma_form = (params->compat & PLVI_COMPAT_SCALEADD_FMA) != 0;
    a.n_levels = params->n_levels, a.max_obs = params->max_obs, a.row_cap = params->row_cap;
    a.ids = d_ids, a.n_ids = n_ids;
    a.normal = out->normal, a.dist = out->dist, a.state = out->state, a.n_rows = out->n_rows, a.err = out->err;
    memcpy(a.scale, params->scale, sizeof(float) * (size_t)params->n_levels);
    uint8_t* scr = static_cast<uint8_t*>(d_scratch);
    int *best_pos = nullptr, *best_median = nullptr;
    if (desc) {
        a.csr_off = reinterpret_cast<int*>(scr + lay.off);
        a.csr_row = reinterpret_cast<int*>(scr + lay.row);
        best_pos = out->best_pos ? out->best_pos : reinterpret_cast<int*>(scr + lay.pos);
        best_median = out->best_median ? out->best_median : reinterpret_cast<int*>(scr + lay.median);
        hipLaunchKernelGGL(refresh_csr_kernel, dim3(1), dim3(kCsrThreads), 0, st, a);
        PLVI_CHECK(hipGetLastError());
    }
    if (params->max_obs <= 8) launch_walk<8>(a, st);
    else if (params->max_obs <= 16) launch_walk<16>(a, st);
    else launch_walk<32>(a, st);
    PLVI_CHECK(hipGetLastError());
    if (desc) {
        // the public batch call on the CSR: no distinctive kernel is new
        if (int rc = plvi_distinctive_descriptors_batch(n_ids, kf->desc, kf->kf_cap * kf->cap, a.csr_off, a.csr_row,
                                                        params->max_obs, best_pos, best_median, scr + lay.chosen, st))
            return rc;
        const long long threads = 8ll * n_ids;
        hipLaunchKernelGGL(refresh_scatter_kernel, dim3((unsigned)((threads + kScatterThreads - 1) / kScatterThreads)),
                           dim3(kScatterThreads), 0, st, d_ids, n_ids, pool->n, best_pos,
                           reinterpret_cast<const uint32_t*>(scr + lay.chosen),
                           reinterpret_cast<uint32_t*>(out->desc), out->state);
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

extern "C" int plvi_feature_refresh(const plvi_refresh_keyframes* kf, const plvi_local_map_pool* pool,
                                    const plvi_ba_features* feat, const plvi_eg_features* ref,
                                    const plvi_refresh_params* params, const int* ids, int n_ids,
                                    const plvi_refresh_outputs* out) {
    if (int rc = refresh_validate(kf, pool, feat, ref, params, ids, n_ids, out)) return rc;
    const size_t n = (size_t)pool->n, rows = (size_t)kf->kf_cap * kf->cap;
    if (pool->obs_off[n] < 0) return PLVI_E_BADARG;
    const size_t n_obs = (size_t)pool->obs_off[n];
    const bool desc = params->what & PLVI_REFRESH_DESC;
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut;
    HostStage hs;
    plvi_refresh_keyframes dk = *kf;
    hs.field(dk.bad, In, (size_t)kf->kf_cap);
    hs.field(dk.ow, In, (size_t)kf->kf_cap, 3);
    hs.field(dk.cnt, In, (size_t)kf->kf_cap);
    hs.field(dk.info, In, rows);
    hs.field(dk.desc, In, rows, 32);
    plvi_local_map_pool dp;
    memset(&dp, 0, sizeof dp);
    dp.n = pool->n, dp.bad = pool->bad, dp.obs_off = pool->obs_off, dp.obs_kf = pool->obs_kf;
    dp.pos = pool->pos, dp.sep = pool->sep;
    hs.field(dp.bad, In, n);
    hs.field(dp.obs_off, In, n + 1);
    hs.field(dp.obs_kf, In, n_obs);
    hs.field(dp.pos, In, n, 3);
    hs.field(dp.sep, In, n, 6);
    plvi_ba_features df;
    memset(&df, 0, sizeof df);
    df.obs_idx = feat ? feat->obs_idx : nullptr;
    hs.field(df.obs_idx, In, n_obs);
    plvi_eg_features dr;
    memset(&dr, 0, sizeof dr);
    dr.ref_kf = ref ? ref->ref_kf : nullptr;
    hs.field(dr.ref_kf, In, n);
    const auto I = hs.in(ids, (size_t)n_ids);
    // in/out: the rows of ids not refreshed keep the caller's values
    plvi_refresh_outputs dout = *out;
    hs.field(dout.normal, InOut, n, 3);
    hs.field(dout.dist, InOut, n, 2);
    hs.field(dout.desc, InOut, n, 32);
    hs.field(dout.state, InOut, (size_t)n_ids);
    hs.field(dout.best_pos, InOut, (size_t)n_ids);
    hs.field(dout.best_median, InOut, (size_t)n_ids);
    hs.field(dout.n_rows, HostStage::Out, 1);
    hs.field(dout.err, HostStage::Out, 1);
    const size_t sb = plvi_feature_refresh_scratch_bytes(n_ids, desc ? params->row_cap : 0);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_feature_refresh_batch(&dk, &dp, &df, &dr, params, hs.dev(I), n_ids, &dout, hs.dev(scr), sb,
                                            nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    if (*out->err) return PLVI_E_CAPACITY;
    int count = 0;
    for (int i = 0; i < n_ids; ++i) count += out->state[i] & PLVI_REFRESH_NORMAL;
    return count;
}
