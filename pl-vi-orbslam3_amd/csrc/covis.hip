// covis.hip — the covisibility graph on the device: KeyFrame::UpdateConnections[WithLines]
// (src/KeyFrame.cc:499-622 / :624-769) for a batch of keyframes, AddConnection (:201-214),
// UpdateBestCovisibles (:216-238), EraseConnection (:1154-1168) and the two getters, over a
// resident graph of weight maps and ordered lists by keyframe slot.  Integers only.
//
// The reference applied to the queries one after another equals a gather: a query's counter
// depends on observations, bad flags and map ids only, never on connection state, so
//   covis_count_kernel   one workgroup per query.  The vote of lm_keyframes_kernel (map_pool.h) as a
//                        histogram over the slots, in LDS up to PLVI_COVIS_LDS_KF and in scratch
//                        above; an ordered block-scan compaction of `order` gives the counter (the
//                        query's new weight map, written in place: no other workgroup reads it),
//                        pKFmax (a 64-bit LDS atomicMax of count : reversed position) and the
//                        >= 15 subset, which is sorted in LDS and becomes the query's list; the
//                        parent rule and the query's covis row.
//   covis_upsert_kernel  one thread per (query, listed neighbour): AddConnection on the neighbour
//                        as its map stood after the first kernel (the row counts are snapshot by
//                        covis_init_kernel, a query's own by its count workgroup; appended keys
//                        are distinct, one atomicAdd each).  A neighbour
//                        that is itself a LATER query with a counter is skipped: its own update
//                        overwrites what the earlier query added.
//   covis_resort_kernel  one workgroup per slot marked dirty: UpdateBestCovisibles.
// The sort is rank-by-count on 64-bit keys (weight : rank): the keys are distinct, so
// every entry's position is the number of larger keys -- no padding to a power of two and no
// barrier per stage as a bitonic network would need; lists are tens to a few hundred long.
#include <climits>
#include <cstring>
#include <vector>

#include "block_prims.h"
#include "map_pool.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kCovLdsKf = PLVI_COVIS_LDS_KF;
constexpr int kCovMaxConn = PLVI_COVIS_MAX_CONN;
constexpr int kCovTh = PLVI_COVIS_TH;
constexpr int kCovThreads = 512, kCovWaves = kCovThreads / kWave;
constexpr int kSortThreads = 256, kSortWaves = kSortThreads / kWave;
constexpr int kCovNb = PLVI_KFDB_NEIGHBOURS;
constexpr int kRankNone = 0x7f7f7f7f;  // the byte fill of the rank table
constexpr int kSetChunk = 512;         // slots handed to covis_set_kernel by value

typedef unsigned long long u64;

struct CovState {  // the graph's device tables
    int K, C;
    int *map_kf, *map_w, *map_n, *map_n0;  // [K][C], [K], the snapshot of the counts
    int *ord_kf, *ord_w, *ord_n;
    int *err, *rank, *qpos, *dirty, *q;    // [K]
};

struct CovArgs {
    CovState g;
    int B, n_order, kp_cap, kl_cap, with_lines, mp_n, ml_n;
    const uint8_t *kf_bad, *init_kf, *mp_bad, *ml_bad;
    const int *order, *kf_mp, *kf_nmp, *kf_ml, *kf_nml, *map_id;
    const int *mp_obs_off, *mp_obs_kf, *ml_obs_off, *ml_obs_kf;
    uint8_t* first_conn;
    int *parent, *covis;
    int* hist_g;  // scratch [B][K], K > kCovLdsKf only
    int *n_counted, *n_conn, *kf_max, *w_max, *new_parent, *o_err;
};

struct CovSet {
    int n, base, mode;  // mode 0: q[base + i] = slot, qpos[slot] = base + i; 1: dirty[slot] = 1
    int slot[kSetChunk];
};

// a larger key sorts earlier: sort() ascending on pair<int, KeyFrame*> and push_front (:569-576)
// leave the list descending by (weight, address), the address being the position in `order`
__device__ __forceinline__ u64 sort_key(int w, int rank, int slot, int n_order) {
    const unsigned r = rank == kRankNone ? (unsigned)n_order + (unsigned)slot : (unsigned)rank;
    return (u64)(unsigned)w << 32 | r;
}

// s_key[0, n) / s_slot[0, n) -> the row's ordered list, descending; every thread calls it
template <int NT>
__device__ void sort_to_row(const u64* s_key, const int* s_slot, int n, int* ord_kf, int* ord_w, int tid) {
    for (int e = tid; e < n; e += NT) {
        const u64 k = s_key[e];
        int p = 0;
        for (int j = 0; j < n; ++j) p += s_key[j] > k;
        ord_kf[p] = s_slot[e];
        ord_w[p] = (int)(k >> 32);
    }
}

// GetBestCovisibilityKeyFrames(10) of a rewritten list: the whole row, -1 past the list
__device__ __forceinline__ void write_covis_row(int* covis, int slot, const int* ord_kf, int n, int tid) {
    if (covis && tid < kCovNb) covis[(size_t)slot * kCovNb + tid] = tid < n ? ord_kf[tid] : -1;
}

// the work tables of a call in one launch (three fills and a copy would be four stream operations,
// and the call is bound by their number: DESIGN.md section 22): no rank, no query, nothing dirty,
// and the row counts as they stand -- the upserts look a key up below these
__global__ void covis_init_kernel(CovState g) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.K) return;
    g.rank[i] = kRankNone;
    g.qpos[i] = -1;
    g.dirty[i] = 0;
    g.map_n0[i] = g.map_n[i];
}

__global__ void covis_rank_kernel(CovState g, const int* order, int n_order) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_order) return;
    const int s = order[i];
    if ((unsigned)s < (unsigned)g.K) atomicMin(g.rank + s, i);
}

__global__ void covis_set_kernel(CovState g, CovSet a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int s = a.slot[i];  // checked on the host
    if (a.mode == 0) {
        g.q[a.base + i] = s;
        g.qpos[s] = a.base + i;
    } else {
        g.dirty[s] = 1;
    }
}

__global__ __launch_bounds__(kCovThreads) void covis_count_kernel(CovArgs a) {
    __shared__ int s_hist[kCovLdsKf];
    __shared__ u64 s_key[kCovMaxConn];
    __shared__ int s_slot[kCovMaxConn];
    __shared__ int s_wave[kCovWaves];
    __shared__ u64 s_best;
    const CovState& g = a.g;
    const int tid = threadIdx.x, q = blockIdx.x;
    const int K = g.K, C = g.C, qs = g.q[q];
    const bool in_lds = K <= kCovLdsKf;
    int* hist = in_lds ? s_hist : a.hist_g + (size_t)q * K;  // the global table was cleared before the launch
    if (in_lds)
        for (int i = tid; i < K; i += kCovThreads) s_hist[i] = 0;
    if (tid == 0) s_best = 0;
    __syncthreads();

    // Count (:512-531; the line loop of :656-676 into the same counter)
    for (int k = 0; k < 1 + a.with_lines; ++k) {
        const int cap = k ? a.kl_cap : a.kp_cap, pool_n = k ? a.ml_n : a.mp_n;
        if (cap <= 0 || pool_n <= 0) continue;
        const int* tab = (k ? a.kf_ml : a.kf_mp) + (size_t)qs * cap;
        const uint8_t* bad = k ? a.ml_bad : a.mp_bad;
        const int n = clampi((k ? a.kf_nml : a.kf_nmp)[qs], 0, cap);
        for (int i = tid; i < n; i += kCovThreads) {
            const int id = tab[i];
            if ((unsigned)id >= (unsigned)pool_n || bad[id]) continue;
            vote_observations(hist, K, k ? a.ml_obs_off : a.mp_obs_off, k ? a.ml_obs_kf : a.mp_obs_kf, id);
        }
    }
    __syncthreads();

    // Walk (:547-561) as an ordered compaction of `order`: the counter goes to the query's weight
    // map, the >= th subset to the sort buffer.  Nothing is written for an empty counter (:534).
    int* map_kf = g.map_kf + (size_t)qs * C;
    int* map_w = g.map_w + (size_t)qs * C;
    const int my_map = a.map_id ? a.map_id[qs] : 0;
    int n_all = 0, n_th = 0;
    for (int i0 = 0; i0 < a.n_order; i0 += kCovThreads) {
        const int i = i0 + tid;
        const int slot = i < a.n_order ? a.order[i] : -1;
        int c = 0;
        const bool counted = (unsigned)slot < (unsigned)K && g.rank[slot] == i && slot != qs && (c = hist[slot]) > 0 &&
                             !a.kf_bad[slot] && (!a.map_id || a.map_id[slot] == my_map);
        const bool listed = counted && c >= kCovTh;
        int tot_all, tot_th;
        const int p_all = n_all + block_scan<kCovWaves>(counted, s_wave, tid, &tot_all);
        const int p_th = n_th + block_scan<kCovWaves>(listed, s_wave, tid, &tot_th);
        if (counted) {
            if (p_all < C) {
                map_kf[p_all] = slot;
                map_w[p_all] = c;
            }
            // `second > nmax` keeps the first of the largest: the largest (count, reversed position)
            atomicMax(&s_best, (u64)(unsigned)c << 32 | (0xffffffffu - (unsigned)i));
        }
        if (listed && p_th < C) {
            s_key[p_th] = sort_key(c, i, slot, a.n_order);
            s_slot[p_th] = slot;
        }
        n_all += tot_all;
        n_th += tot_th;
    }
    __syncthreads();
    if (n_all == 0) {
        if (tid == 0) {
            a.n_counted[q] = 0;
            a.n_conn[q] = 0;
            a.kf_max[q] = -1;
            a.w_max[q] = 0;
            a.new_parent[q] = -1;
            a.o_err[q] = 0;
        }
        return;
    }
    const u64 best = s_best;
    const int i_max = (int)(0xffffffffu - (unsigned)best), w_max = (int)(best >> 32), s_max = a.order[i_max];
    if (n_th == 0) {  // :563-567
        if (tid == 0) {
            s_key[0] = sort_key(w_max, i_max, s_max, a.n_order);
            s_slot[0] = s_max;
        }
        n_th = 1;
        __syncthreads();
    }
    const int n_list = min(n_th, C);
    int* ord_kf = g.ord_kf + (size_t)qs * C;
    sort_to_row<kCovThreads>(s_key, s_slot, n_list, ord_kf, g.ord_w + (size_t)qs * C, tid);
    __syncthreads();
    write_covis_row(a.covis, qs, ord_kf, n_list, tid);
    if (tid == 0) {
        const int err = n_all > C || n_th > C;
        g.map_n[qs] = min(n_all, C);
        g.map_n0[qs] = min(n_all, C);  // the map as it stands after this kernel
        g.ord_n[qs] = n_list;
        g.err[qs] = err;
        a.n_counted[q] = n_all;
        a.n_conn[q] = n_th;
        a.kf_max[q] = s_max;
        a.w_max[q] = w_max;
        a.o_err[q] = err;
        int np = -1;
        if (a.first_conn && a.first_conn[qs] && !(a.init_kf && a.init_kf[qs])) {  // :593-619
            np = ord_kf[0];
            a.parent[qs] = np;
            a.first_conn[qs] = 0;
        }
        a.new_parent[q] = np;
    }
}

// AddConnection(query, w) on every listed neighbour of every query (:559, :566)
__global__ __launch_bounds__(kSortThreads) void covis_upsert_kernel(CovArgs a) {
    const CovState& g = a.g;
    const int q = blockIdx.y, e = blockIdx.x * kSortThreads + threadIdx.x;
    if (a.n_counted[q] == 0) return;  // :534 returned before any AddConnection
    const int qs = g.q[q], C = g.C;
    if (e >= min(g.ord_n[qs], C)) return;
    const int t = g.ord_kf[(size_t)qs * C + e], w = g.ord_w[(size_t)qs * C + e];
    if ((unsigned)t >= (unsigned)g.K) return;
    const int tq = g.qpos[t];
    if (tq > q && a.n_counted[tq] > 0) return;  // t's own update comes later and overwrites this
    int* t_kf = g.map_kf + (size_t)t * C;
    int* t_w = g.map_w + (size_t)t * C;
    const int n0 = min(g.map_n0[t], C);
    for (int j = 0; j < n0; ++j)
        if (t_kf[j] == qs) {
            if (t_w[j] != w) {
                t_w[j] = w;
                g.dirty[t] = 1;
            }
            return;  // an equal weight returns before UpdateBestCovisibles (:209)
        }
    const int p = atomicAdd(g.map_n + t, 1);  // resort clamps the count back to C
    if (p < C) {
        t_kf[p] = qs;
        t_w[p] = w;
    } else {
        g.err[t] = 1;
    }
    g.dirty[t] = 1;
}

// UpdateBestCovisibles (:216-238) of every dirty slot; entries erased (-1) leave the map first
__global__ __launch_bounds__(kSortThreads) void covis_resort_kernel(CovState g, const uint8_t* kf_bad, int n_order,
                                                                    int* covis) {
    __shared__ int s_mkf[kCovMaxConn], s_mw[kCovMaxConn], s_slot[kCovMaxConn];
    __shared__ u64 s_key[kCovMaxConn];
    __shared__ int s_wave[kSortWaves];
    const int s = blockIdx.x, tid = threadIdx.x, C = g.C;
    if (!g.dirty[s]) return;
    int* map_kf = g.map_kf + (size_t)s * C;
    int* map_w = g.map_w + (size_t)s * C;
    const int n = clampi(g.map_n[s], 0, C);
    for (int e = tid; e < n; e += kSortThreads) {
        s_mkf[e] = map_kf[e];
        s_mw[e] = map_w[e];
    }
    __syncthreads();
    int n_map = 0, n_list = 0;
    for (int e0 = 0; e0 < n; e0 += kSortThreads) {
        const int e = e0 + tid;
        const int kf = e < n ? s_mkf[e] : -1;
        const bool live = (unsigned)kf < (unsigned)g.K;
        const bool good = live && !kf_bad[kf];
        int tot_map, tot_list;
        const int p_map = n_map + block_scan<kSortWaves>(live, s_wave, tid, &tot_map);
        const int p_list = n_list + block_scan<kSortWaves>(good, s_wave, tid, &tot_list);
        if (live) {
            map_kf[p_map] = kf;
            map_w[p_map] = s_mw[e];
        }
        if (good) {
            s_key[p_list] = sort_key(s_mw[e], g.rank[kf], kf, n_order);
            s_slot[p_list] = kf;
        }
        n_map += tot_map;
        n_list += tot_list;
    }
    __syncthreads();
    int* ord_kf = g.ord_kf + (size_t)s * C;
    sort_to_row<kSortThreads>(s_key, s_slot, n_list, ord_kf, g.ord_w + (size_t)s * C, tid);
    __syncthreads();
    write_covis_row(covis, s, ord_kf, n_list, tid);
    if (tid == 0) {
        g.map_n[s] = n_map;
        g.ord_n[s] = n_list;
    }
}

// EraseConnection(slot) on every key of an erased slot's map (:894-897)
__global__ __launch_bounds__(kSortThreads) void covis_erase_kernel(CovState g) {
    const int s = g.q[blockIdx.y], e = blockIdx.x * kSortThreads + threadIdx.x, C = g.C;
    if (e >= min(g.map_n[s], C)) return;
    const int t = g.map_kf[(size_t)s * C + e];
    if ((unsigned)t >= (unsigned)g.K || g.qpos[t] >= 0) return;  // an erased neighbour ends empty anyway
    int* t_kf = g.map_kf + (size_t)t * C;
    const int n = min(g.map_n[t], C);
    for (int j = 0; j < n; ++j)
        if (t_kf[j] == s) {
            t_kf[j] = -1;  // dropped by the re-sort; keys are distinct, so no other thread writes this cell
            g.dirty[t] = 1;
            return;
        }
}

// the erased slots' own map and list cleared (:915-916)
__global__ void covis_clear_kernel(CovState g, int n, int* covis) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = g.q[i];
    g.map_n[s] = 0;
    g.ord_n[s] = 0;
    g.err[s] = 0;
    if (covis)
        for (int c = 0; c < kCovNb; ++c) covis[(size_t)s * kCovNb + c] = -1;
}

__global__ void covis_by_weight_kernel(CovState g, int n, const int* slot, const int* w, int* count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = slot[i];
    int lo = 0;
    if ((unsigned)s < (unsigned)g.K) {
        // upper_bound with weightComp (:274) on a descending list: the first weight below w
        const int* ow = g.ord_w + (size_t)s * g.C;
        int hi = clampi(g.ord_n[s], 0, g.C);
        const int wi = w[i];
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ow[mid] >= wi)
                lo = mid + 1;
            else
                hi = mid;
        }
    }
    count[i] = lo;
}

__global__ void covis_weight_kernel(CovState g, int n, const int* a, const int* b, int* weight) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = a[i], t = b[i];
    int w = 0;
    if ((unsigned)s < (unsigned)g.K) {
        const int m = clampi(g.map_n[s], 0, g.C);
        for (int j = 0; j < m; ++j)
            if (g.map_kf[(size_t)s * g.C + j] == t) w = g.map_w[(size_t)s * g.C + j];
    }
    weight[i] = w;
}

}  // namespace plvi

using namespace plvi;

struct plvi_covis_graph {
    CovState g;
    int device = 0;
    DevBuf map_kf, map_w, ord_kf, ord_w, small;  // small: the eight [K] tables
    std::vector<int> stamp;                      // host: the call that last named a slot
    int call = 0;
};

extern "C" int plvi_covis_create(int kf_cap, int conn_cap, int device, plvi_covis_graph** out) {
    if (!out) return PLVI_E_BADARG;
    *out = nullptr;
    if (kf_cap < 1 || conn_cap < 1) return PLVI_E_BADARG;
    if (kf_cap > (1 << 24) || conn_cap > kCovMaxConn) return PLVI_E_CAPACITY;
    PLVI_CHECK(hipSetDevice(device));
    plvi_covis_graph* h = new plvi_covis_graph;
    h->device = device;
    h->stamp.assign(kf_cap, 0);
    const size_t K = (size_t)kf_cap, cells = 4 * K * conn_cap, row = up256(4 * K);
    if (h->map_kf.alloc(cells) || h->map_w.alloc(cells) || h->ord_kf.alloc(cells) || h->ord_w.alloc(cells) ||
        h->small.alloc(8 * row) || hipMemset(h->small.p, 0, 8 * row) != hipSuccess) {
        delete h;
        return PLVI_E_HIP;
    }
    CovState& g = h->g;
    g.K = kf_cap;
    g.C = conn_cap;
    g.map_kf = h->map_kf.as<int>();
    g.map_w = h->map_w.as<int>();
    g.ord_kf = h->ord_kf.as<int>();
    g.ord_w = h->ord_w.as<int>();
    int** small[8] = {&g.map_n, &g.map_n0, &g.ord_n, &g.err, &g.rank, &g.qpos, &g.dirty, &g.q};
    for (int i = 0; i < 8; ++i) *small[i] = reinterpret_cast<int*>(h->small.as<uint8_t>() + i * row);
    *out = h;
    return PLVI_OK;
}

extern "C" int plvi_covis_destroy(plvi_covis_graph* h) {
    if (!h) return PLVI_E_BADARG;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return PLVI_OK;
}

extern "C" size_t plvi_covis_scratch_bytes(int n_queries, int kf_cap) {
    if (n_queries < 0 || kf_cap < 0) return 0;
    return 256 + (kf_cap > kCovLdsKf ? up256(4 * (size_t)n_queries * kf_cap) : 0);
}

// every slot in range and named once
static bool slots_ok(plvi_covis_graph* h, int n, const int* slots) {
    if (h->call == INT_MAX) {
        h->stamp.assign(h->stamp.size(), 0);
        h->call = 0;
    }
    const int c = ++h->call;
    for (int i = 0; i < n; ++i) {
        const int s = slots[i];
        if (s < 0 || s >= h->g.K || h->stamp[s] == c) return false;
        h->stamp[s] = c;
    }
    return true;
}

// the work tables of a call: rank from `order`, qpos / dirty cleared, the named slots set
static int cov_begin(plvi_covis_graph* h, int n, const int* slots, int mode, const int* d_order, int n_order,
                     hipStream_t st) {
    const CovState& g = h->g;
    hipLaunchKernelGGL(covis_init_kernel, dim3((g.K + 255) / 256), dim3(256), 0, st, g);
    PLVI_CHECK(hipGetLastError());
    if (n_order > 0) {
        hipLaunchKernelGGL(covis_rank_kernel, dim3((n_order + 255) / 256), dim3(256), 0, st, g, d_order, n_order);
        PLVI_CHECK(hipGetLastError());
    }
    for (int i0 = 0; i0 < n; i0 += kSetChunk) {
        CovSet a;
        a.n = n - i0 < kSetChunk ? n - i0 : kSetChunk;
        a.base = i0;
        a.mode = mode;
        memcpy(a.slot, slots + i0, 4 * (size_t)a.n);
        hipLaunchKernelGGL(covis_set_kernel, dim3((a.n + 255) / 256), dim3(256), 0, st, g, a);
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

static int cov_resort(plvi_covis_graph* h, const uint8_t* d_bad, int n_order, int* d_covis, hipStream_t st) {
    hipLaunchKernelGGL(covis_resort_kernel, dim3(h->g.K), dim3(kSortThreads), 0, st, h->g, d_bad, n_order, d_covis);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

static int cov_validate(plvi_covis_graph* h, int n_queries, const plvi_covis_keyframes* kf,
                        const plvi_local_map_pool* mp, const plvi_local_map_pool* ml, const plvi_covis_outputs* out) {
    if (!h || n_queries < 0 || !kf || !mp || !out) return PLVI_E_BADARG;
    if (kf->kf_cap != h->g.K || kf->n_order < 0 || kf->kp_cap < 0 || kf->kl_cap < 0 || !pool_ok(mp) ||
        (ml && !pool_ok(ml)))
        return PLVI_E_BADARG;
    if (n_queries == 0) return PLVI_OK;
    const bool with_lines = kf->ml && ml;
    if (!kf->bad || (kf->n_order > 0 && !kf->order) || (kf->kp_cap > 0 && (!kf->mp || !kf->nmp)) ||
        (with_lines && !kf->nml) || (kf->first_conn == nullptr) != (kf->parent == nullptr))
        return PLVI_E_BADARG;
    if (!out->n_counted || !out->n_conn || !out->kf_max || !out->w_max || !out->new_parent || !out->err)
        return PLVI_E_BADARG;
    if (n_queries > PLVI_COVIS_MAX_QUERIES) return PLVI_E_CAPACITY;
    return PLVI_OK;
}

extern "C" int plvi_covis_update_batch(plvi_covis_graph* h, int n_queries, const int* q_slot,
                                       const plvi_covis_keyframes* kf, const plvi_local_map_pool* mp,
                                       const plvi_local_map_pool* ml, const plvi_covis_outputs* out, void* d_scratch,
                                       size_t scratch_bytes, void* stream) {
    if (int rc = cov_validate(h, n_queries, kf, mp, ml, out)) return rc;
    if (n_queries == 0) return PLVI_OK;
    const size_t sb = plvi_covis_scratch_bytes(n_queries, h->g.K);
    if (!q_slot || !d_scratch || scratch_bytes < sb) return PLVI_E_BADARG;
    if (!slots_ok(h, n_queries, q_slot)) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const CovState& g = h->g;
    const bool with_lines = kf->ml && ml;
    if (int rc = cov_begin(h, n_queries, q_slot, 0, kf->order, kf->n_order, st)) return rc;
    CovArgs a;
    memset(&a, 0, sizeof a);
    a.g = g;
    a.B = n_queries;
    a.n_order = kf->n_order;
    a.kp_cap = kf->kp_cap;
    a.kl_cap = with_lines ? kf->kl_cap : 0;
    a.with_lines = with_lines;
    a.mp_n = mp->n;
    a.ml_n = with_lines ? ml->n : 0;
    a.kf_bad = kf->bad;
    a.init_kf = kf->init_kf;
    a.mp_bad = mp->bad;
    a.mp_obs_off = mp->obs_off;
    a.mp_obs_kf = mp->obs_kf;
    if (with_lines) {
        a.ml_bad = ml->bad;
        a.ml_obs_off = ml->obs_off;
        a.ml_obs_kf = ml->obs_kf;
        a.kf_ml = kf->ml;
        a.kf_nml = kf->nml;
    }
    a.order = kf->order;
    a.kf_mp = kf->mp;
    a.kf_nmp = kf->nmp;
    a.map_id = kf->map_id;
    a.first_conn = kf->first_conn;
    a.parent = kf->parent;
    a.covis = kf->covis;
    a.hist_g = reinterpret_cast<int*>(static_cast<uint8_t*>(d_scratch) + 256);
    if (g.K > kCovLdsKf) PLVI_CHECK(hipMemsetAsync(a.hist_g, 0, 4 * (size_t)n_queries * g.K, st));
    a.n_counted = out->n_counted;
    a.n_conn = out->n_conn;
    a.kf_max = out->kf_max;
    a.w_max = out->w_max;
    a.new_parent = out->new_parent;
    a.o_err = out->err;
    hipLaunchKernelGGL(covis_count_kernel, dim3(n_queries), dim3(kCovThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    hipLaunchKernelGGL(covis_upsert_kernel, dim3((g.C + kSortThreads - 1) / kSortThreads, n_queries),
                       dim3(kSortThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return cov_resort(h, kf->bad, kf->n_order, kf->covis, st);
}

static int cov_slots_call(plvi_covis_graph* h, int n, const int* slots, const uint8_t* d_bad, const int* d_order,
                          int n_order, int* d_covis, void* stream, bool erase) {
    if (!h || n < 0 || n_order < 0) return PLVI_E_BADARG;
    if (n == 0) return PLVI_OK;
    if (!slots || !d_bad || (n_order > 0 && !d_order) || !slots_ok(h, n, slots)) return PLVI_E_BADARG;
    if (n > PLVI_COVIS_MAX_QUERIES) return PLVI_E_CAPACITY;
    PLVI_CHECK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = cov_begin(h, n, slots, erase ? 0 : 1, d_order, n_order, st)) return rc;
    if (erase) {
        hipLaunchKernelGGL(covis_erase_kernel, dim3((h->g.C + kSortThreads - 1) / kSortThreads, n), dim3(kSortThreads),
                           0, st, h->g);
        PLVI_CHECK(hipGetLastError());
    }
    if (int rc = cov_resort(h, d_bad, n_order, d_covis, st)) return rc;
    if (erase) {
        hipLaunchKernelGGL(covis_clear_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h->g, n, d_covis);
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

extern "C" int plvi_covis_erase_batch(plvi_covis_graph* h, int n, const int* slots, const uint8_t* d_bad,
                                      const int* d_order, int n_order, int* d_covis, void* stream) {
    return cov_slots_call(h, n, slots, d_bad, d_order, n_order, d_covis, stream, true);
}

extern "C" int plvi_covis_resort_batch(plvi_covis_graph* h, int n, const int* slots, const uint8_t* d_bad,
                                       const int* d_order, int n_order, int* d_covis, void* stream) {
    return cov_slots_call(h, n, slots, d_bad, d_order, n_order, d_covis, stream, false);
}

extern "C" int plvi_covis_by_weight_batch(plvi_covis_graph* h, int n, const int* d_slot, const int* d_w, int* d_count,
                                          void* stream) {
    if (!h || n < 0) return PLVI_E_BADARG;
    if (n == 0) return PLVI_OK;
    if (!d_slot || !d_w || !d_count) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(covis_by_weight_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->g, n, d_slot,
                       d_w, d_count);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_covis_weight_batch(plvi_covis_graph* h, int n, const int* d_a, const int* d_b, int* d_weight,
                                       void* stream) {
    if (!h || n < 0) return PLVI_E_BADARG;
    if (n == 0) return PLVI_OK;
    if (!d_a || !d_b || !d_weight) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(covis_weight_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->g, n, d_a, d_b,
                       d_weight);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_covis_rows(plvi_covis_graph* h, const int** d_ord_kf, const int** d_ord_w, const int** d_ord_n,
                               int* conn_cap) {
    if (!h) return PLVI_E_BADARG;
    if (d_ord_kf) *d_ord_kf = h->g.ord_kf;
    if (d_ord_w) *d_ord_w = h->g.ord_w;
    if (d_ord_n) *d_ord_n = h->g.ord_n;
    if (conn_cap) *conn_cap = h->g.C;
    return PLVI_OK;
}

extern "C" int plvi_covis_map_rows(plvi_covis_graph* h, const int** d_map_kf, const int** d_map_w, const int** d_map_n,
                                   int* conn_cap) {
    if (!h) return PLVI_E_BADARG;
    if (d_map_kf) *d_map_kf = h->g.map_kf;
    if (d_map_w) *d_map_w = h->g.map_w;
    if (d_map_n) *d_map_n = h->g.map_n;
    if (conn_cap) *conn_cap = h->g.C;
    return PLVI_OK;
}

extern "C" int plvi_covis_download(plvi_covis_graph* h, int slot, int* map_kf, int* map_w, int* n_map, int* ord_kf,
                                   int* ord_w, int* n_ord, int* err) {
    if (!h || slot < 0 || slot >= h->g.K) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    PLVI_CHECK(hipDeviceSynchronize());
    const CovState& g = h->g;
    const size_t C = (size_t)g.C, row = (size_t)slot * C;
    int nm = 0, no = 0;
    PLVI_CHECK(hipMemcpy(&nm, g.map_n + slot, 4, hipMemcpyDeviceToHost));
    PLVI_CHECK(hipMemcpy(&no, g.ord_n + slot, 4, hipMemcpyDeviceToHost));
    nm = nm < 0 ? 0 : nm > g.C ? g.C : nm;
    no = no < 0 ? 0 : no > g.C ? g.C : no;
    if (n_map) *n_map = nm;
    if (n_ord) *n_ord = no;
    if (err) PLVI_CHECK(hipMemcpy(err, g.err + slot, 4, hipMemcpyDeviceToHost));
    if ((map_kf || map_w) && nm) {
        std::vector<int> k(nm), w(nm), idx(nm);
        PLVI_CHECK(hipMemcpy(k.data(), g.map_kf + row, 4 * (size_t)nm, hipMemcpyDeviceToHost));
        PLVI_CHECK(hipMemcpy(w.data(), g.map_w + row, 4 * (size_t)nm, hipMemcpyDeviceToHost));
        // ascending slot: insertion sort by key (the rows are short)
        for (int i = 0; i < nm; ++i) idx[i] = i;
        for (int i = 1; i < nm; ++i) {
            const int v = idx[i];
            int j = i;
            for (; j > 0 && k[idx[j - 1]] > k[v]; --j) idx[j] = idx[j - 1];
            idx[j] = v;
        }
        for (int i = 0; i < nm; ++i) {
            if (map_kf) map_kf[i] = k[idx[i]];
            if (map_w) map_w[i] = w[idx[i]];
        }
    }
    if (ord_kf && no) PLVI_CHECK(hipMemcpy(ord_kf, g.ord_kf + row, 4 * (size_t)no, hipMemcpyDeviceToHost));
    if (ord_w && no) PLVI_CHECK(hipMemcpy(ord_w, g.ord_w + row, 4 * (size_t)no, hipMemcpyDeviceToHost));
    return PLVI_OK;
}

// One keyframe from host memory.  Every pointer of the structs is a host pointer here.
extern "C" int plvi_covis_update(plvi_covis_graph* h, int slot, const plvi_covis_keyframes* kf,
                                 const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                 const plvi_covis_outputs* out) {
    if (int rc = cov_validate(h, 1, kf, mp, ml, out)) return rc;
    if (slot < 0 || slot >= h->g.K) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    const bool with_lines = kf->ml && ml;
    const size_t K = (size_t)kf->kf_cap;
    // copies of the caller's structs: commit() turns their host pointers into device pointers
    plvi_covis_keyframes dk = *kf;
    plvi_local_map_pool dmp = *mp, dml = with_lines ? *ml : plvi_local_map_pool{};
    plvi_covis_outputs dout = *out;
    if (!with_lines) dk.ml = dk.nml = nullptr;
    HostStage hs;
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut, Out = HostStage::Out;
    hs.field(dk.bad, In, K);
    hs.field(dk.order, In, kf->n_order);
    hs.field(dk.mp, In, K, kf->kp_cap);
    hs.field(dk.nmp, In, K);
    hs.field(dk.ml, In, K, kf->kl_cap);
    hs.field(dk.nml, In, K);
    hs.field(dk.map_id, In, K);
    hs.field(dk.init_kf, In, K);
    hs.field(dk.first_conn, InOut, K);
    hs.field(dk.parent, InOut, K);
    hs.field(dk.covis, InOut, K, kCovNb);
    stage_pool(hs, dmp, kPoolObs);
    if (with_lines) stage_pool(hs, dml, kPoolObs);
    for (int** o : {&dout.n_counted, &dout.n_conn, &dout.kf_max, &dout.w_max, &dout.new_parent, &dout.err})
        hs.field(*o, Out, 1);
    const size_t sb = plvi_covis_scratch_bytes(1, kf->kf_cap);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_covis_update_batch(h, 1, &slot, &dk, &dmp, with_lines ? &dml : nullptr, &dout, hs.dev(scr), sb,
                                         nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err ? PLVI_E_CAPACITY : PLVI_OK;
}
