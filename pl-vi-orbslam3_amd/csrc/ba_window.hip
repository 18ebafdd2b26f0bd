// ba_window.hip — the set-up of local bundle adjustment for a batch of current keyframes:
// Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, num_fixedKF) (src/Optimizer.cc:4851-4960,
// edges :5048-5168), LocalBundleAdjustmentOnlyLines and its two Angle variants (:6181-6233, edges
// :6291-6337) and LocalInertialBA (:9185-9307, edges :9521-9640).  Integers only.
//
// The reference's mnBALocalForKF / mnBAFixedForKF stamps make "first come" decisions along a
// fixed traversal; here every such decision is "the smallest traversal position wins" (first_walk.h):
//   local keyframes  cam[slot] = atomicMin of the row position (q is 0, row entry p is 1 + p); a
//                    row entry that is stamped but not listed leaves kBaLocal.  dl[] is the list
//                    without its repeats, which is all the feature walk needs.
//   local features   the first-occurrence walk over the rows of dl[], first[n] cleared per query.
//   fixed cameras    keys[slot] = atomicMin of (feature position << 32 | observation offset) over
//                    the observers that are not stamped local; the keys of the slots that pass the
//                    bad / map test are sorted, and a key names its slot through obs_kf.
//   two-lowest rule  thread 0, over the row as written.
//   inertial walk    the break makes feature j's choice depend on the features before it.  Wave 0
//                    takes 64 features at a time against the current stamps; most choose nothing.
//                    The lanes that chose are then taken in lane order, and a lane whose keyframe
//                    an earlier lane took walks its observers again.  (A bad unstamped observer is
//                    stamped by the reference and passed; the stamp of a bad keyframe is read by
//                    nothing that reaches an output, so it is not kept.)
//   edges            count per feature, block scan per tile, write; edge_cam from cam[], which by
//                    then holds every listed keyframe's first position in local || fixed.
// One workgroup per query and one launch; keys[] and cam[] are LDS up to PLVI_BA_LDS_KF slots.
#include <cstring>

#include "first_walk.h"
#include "map_pool.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kBaThreads = 1024;
constexpr int kBaWaves = kBaThreads / kWave;
constexpr int kBaMaxFix = PLVI_BA_MAX_FIXED_INERTIAL;
constexpr unsigned kBaLocal = kNoPos - 1, kBaFixed = kNoPos - 2;  // cam[] stamps above every position

typedef unsigned long long u64;
constexpr u64 kBaNoKey = ~0ull;

struct BaArgs {
    int K, cand_stride, mode, max_opt;
    int n, cap;  // the pool of the mode and the row length of its keyframe table
    int P;       // pow2_at_least(K): entries of keys[]
    const uint8_t *kf_bad, *init_kf;
    const int *cand, *n_cand;
    const unsigned* kf_id;
    const int *prev_kf, *kf_map;
    const int *tab, *ntab;  // [K][cap], [K]
    const uint8_t* info;    // [K][cap], points only
    const uint8_t* f_bad;
    const int *obs_off, *obs_kf, *obs_idx, *f_map;
    plvi_ba_queries q;
    plvi_ba_outputs o;
    uint8_t* scratch;
    size_t per_query;
};

// the scratch block of one query: keys[P] cam[K] (used above PLVI_BA_LDS_KF) dl[K] first[n] lf[n]
__host__ __device__ inline size_t ba_up256(size_t v) { return (v + 255) & ~size_t(255); }
__host__ __device__ inline size_t ba_off_cam(int P) { return ba_up256(sizeof(u64) * (size_t)P); }
__host__ __device__ inline size_t ba_off_dl(int P, int K) { return ba_off_cam(P) + ba_up256(4 * (size_t)K); }
__host__ __device__ inline size_t ba_off_first(int P, int K) { return ba_off_dl(P, K) + ba_up256(4 * (size_t)K); }
__host__ __device__ inline size_t ba_off_lf(int P, int K, int n) { return ba_off_first(P, K) + ba_up256(4 * (size_t)n); }
__host__ __device__ inline size_t ba_per_query(int P, int K, int n) { return ba_off_lf(P, K, n) + ba_up256(4 * (size_t)n); }

__device__ __forceinline__ unsigned ba_load(const unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void ba_store(unsigned* p, unsigned v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// :4866 / :6195 for a slot in range
__device__ __forceinline__ bool ba_listed(const BaArgs& a, int s, int M) {
    return !a.kf_bad[s] && (a.mode == PLVI_BA_LINES || !a.kf_map || a.kf_map[s] == M);
}

// :4886 / :6208 / :9229 for a feature that is in range and not bad
__device__ __forceinline__ bool ba_in_map(const BaArgs& a, int id, int M) {
    return a.mode == PLVI_BA_INERTIAL || !a.f_map || a.f_map[id] == M;
}

// :9289-9301 for one feature against the current stamps: its first observer in range that is
// unstamped and not bad, or -1
__device__ int ba_choice(const BaArgs& a, const unsigned* cam, int id) {
    const int o1 = a.obs_off[id + 1];
    for (int o = a.obs_off[id]; o < o1; ++o) {
        const int kf = a.obs_kf[o];
        if ((unsigned)kf < (unsigned)a.K && ba_load(cam + kf) == kNoPos && !a.kf_bad[kf]) return kf;
    }
    return -1;
}

// the edge test of :5066 / :6308 / :9538-9541 for observation o
__device__ __forceinline__ bool ba_edge(const BaArgs& a, const unsigned* cam, int o, int M) {
    const int kf = a.obs_kf[o];
    if ((unsigned)kf >= (unsigned)a.K || a.kf_bad[kf] || (a.kf_map && a.kf_map[kf] != M)) return false;
    if (a.mode == PLVI_BA_INERTIAL && cam[kf] == kNoPos) return false;
    return (unsigned)a.obs_idx[o] < (unsigned)a.cap;
}

template <bool kLds>
__global__ __launch_bounds__(kBaThreads) void ba_window_kernel(BaArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int s_wave[kBaWaves];
    __shared__ int s_chain[PLVI_BA_MAX_OPT + 1], s_fix[kBaMaxFix];
    __shared__ int s_n_dl, s_init, s_n_opt, s_n_fixed, s_moved[2], s_n_moved, s_err, s_num_fixed, s_kind[2];
    __shared__ int s_n_fixed_all;  // with the keyframes moved by the two-lowest rule
    const int tid = threadIdx.x, q = blockIdx.x;
    const int cur = a.q.q_slot[q];
    const bool inertial = a.mode == PLVI_BA_INERTIAL;
    const plvi_ba_outputs& o = a.o;

    if ((unsigned)cur >= (unsigned)a.K) {
        if (tid == 0) {
            o.n_local_kf[q] = o.n_fixed_kf[q] = o.num_fixed[q] = o.init_in_local[q] = o.n_local_feat[q] = 0;
            o.n_mono[q] = o.n_stereo[q] = o.n_line[q] = 0;
            o.non_fixed[q] = 1;
            o.err[q] = PLVI_BA_ERR_QUERY;
        }
        return;
    }
    uint8_t* blk = a.scratch + (size_t)q * a.per_query;
    u64* keys = kLds ? reinterpret_cast<u64*>(lds) : reinterpret_cast<u64*>(blk);
    unsigned* cam = kLds ? reinterpret_cast<unsigned*>(lds + sizeof(u64) * a.P)
                         : reinterpret_cast<unsigned*>(blk + ba_off_cam(a.P));
    int* dl = reinterpret_cast<int*>(blk + ba_off_dl(a.P, a.K));
    unsigned* first = reinterpret_cast<unsigned*>(blk + ba_off_first(a.P, a.K));
    int* lf = reinterpret_cast<int*>(blk + ba_off_lf(a.P, a.K, a.n));

    const int M = a.kf_map ? a.kf_map[cur] : 0;
    const int n_row = inertial ? 0 : clampi(a.n_cand[cur], 0, a.cand_stride);
    const int* row = a.cand + (size_t)cur * a.cand_stride;

    for (int s = tid; s < a.K; s += kBaThreads) cam[s] = kNoPos;
    for (int s = tid; s < a.P; s += kBaThreads) keys[s] = kBaNoKey;
    for (int i = tid; i < a.n; i += kBaThreads) first[i] = kNoPos;
    if (tid == 0) {
        s_init = s_n_moved = s_err = s_n_fixed = s_kind[0] = s_kind[1] = 0;
        s_moved[0] = s_moved[1] = -1;
    }
    __syncthreads();

    // ---- 1 / 5: the local keyframes and dl[], the list without its repeats
    if (!inertial) {
        if (tid == 0) atomicMin(cam + cur, 0u);
        for (int p = tid; p < n_row; p += kBaThreads) {
            const int s = row[p];
            if ((unsigned)s < (unsigned)a.K) atomicMin(cam + s, ba_listed(a, s, M) ? 1u + p : kBaLocal);
        }
        __syncthreads();
        int run = 0;
        for (int t0 = 0; t0 <= n_row; t0 += kBaThreads) {
            const int t = t0 + tid;
            const int s = t == 0 ? cur : t <= n_row ? row[t - 1] : -1;
            const int flag = (unsigned)s < (unsigned)a.K && cam[s] == (unsigned)t;
            int tot;
            const int at = run + block_scan<kBaWaves>(flag, s_wave, tid, &tot);
            if (flag) {
                dl[at] = s;
                if (a.init_kf && a.init_kf[s]) s_init = 1;
            }
            run += tot;
        }
        if (tid == 0) s_n_dl = run;
    } else if (tid == 0) {
        const long long nd = min((long long)a.q.n_kf_in_map[q] - 2, (long long)a.max_opt);
        int n = 1, n_dl = 0;
        s_chain[0] = cur;
        for (long long i = 1; i < nd; ++i) {  // :9207-9216
            const int p = a.prev_kf[s_chain[n - 1]];
            if ((unsigned)p >= (unsigned)a.K) break;
            s_chain[n++] = p;
        }
        for (int i = 0; i < n; ++i) {
            const int s = s_chain[i];
            if (cam[s] == kNoPos) {
                cam[s] = kBaLocal;
                dl[n_dl++] = s;
                if (a.init_kf && a.init_kf[s]) s_init = 1;
            }
        }
        const int back = s_chain[n - 1], p = a.prev_kf[back];  // :9240-9251
        if ((unsigned)p < (unsigned)a.K) {
            s_fix[0] = p;
            if (cam[p] == kNoPos) cam[p] = kBaFixed;
        } else {
            cam[back] = kBaFixed;
            s_fix[0] = back;
            --n;
        }
        s_n_dl = n_dl;
        s_n_opt = n;
        s_n_fixed = 1;
    }
    __syncthreads();
    const int n_dl = s_n_dl;

    // ---- 2: the local features: the walk over the rows of dl[] (at most kf_cap * cap positions, which
    // fits: PLVI_LOCAL_MAP_MAX_ENTRIES)
    const KfTable v{a.tab, a.ntab, a.cap, a.n, a.f_bad};
    const auto in_map = [&](int id) { return ba_in_map(a, id, M); };
    first_mark<kBaThreads>((unsigned)n_dl * (unsigned)a.cap, first, row_walk(dl, v, in_map), false);
    const int n_feat =
        first_compact<kBaThreads, 8>(dl, n_dl, v, first, in_map, s_wave, [&](int at, int id, unsigned) {
            lf[at] = id;
            if (at < o.feat_cap) o.local_feat[(size_t)q * o.feat_cap + at] = id;
        });
    __syncthreads();

    // ---- 3 / 5: the fixed cameras
    int n_local = 0;
    if (!inertial) {
        for (int j = tid; j < n_feat; j += kBaThreads) {
            const int id = lf[j], o1 = a.obs_off[id + 1];
            for (int ob = a.obs_off[id]; ob < o1; ++ob) {
                const int kf = a.obs_kf[ob];
                if ((unsigned)kf < (unsigned)a.K && cam[kf] == kNoPos) atomicMin(keys + kf, (u64)j << 32 | (unsigned)ob);
            }
        }
        __syncthreads();
        int mine = 0;
        for (int s = tid; s < a.K; s += kBaThreads) {
            if (keys[s] == kBaNoKey) continue;
            if (a.kf_bad[s] || (a.kf_map && a.kf_map[s] != M))
                keys[s] = kBaNoKey;  // stamped, never listed
            else
                ++mine;
        }
        block_add(mine, &s_n_fixed, tid);
        __syncthreads();
        bitonic_sort<kBaThreads>(keys, a.P, tid);
        // ---- 4: the two-lowest rule
        if (tid == 0) {
            int num_fixed = s_n_fixed + (a.mode == PLVI_BA_POINTS ? s_init : 0);
            if (a.mode == PLVI_BA_POINTS && num_fixed < 2) {
                int lower = (int)a.kf_id[cur], second = lower, p_lower = -1, p_second = -1, nm = 0;
                for (int p = 0; p < n_row; ++p) {
                    const int s = row[p];
                    if ((unsigned)s >= (unsigned)a.K || !ba_listed(a, s, M)) continue;
                    if (s == cur || (a.init_kf && a.init_kf[s])) continue;
                    const u64 id = a.kf_id[s];  // the int is sign-extended, the compare unsigned
                    if (id < (u64)(long long)lower) {
                        lower = (int)id;
                        p_lower = s;
                    } else if (id < (u64)(long long)second) {
                        second = (int)id;
                        p_second = s;
                    }
                }
                if (p_lower >= 0)
                    s_moved[nm++] = p_lower;
                else
                    s_err |= PLVI_BA_ERR_UNDEFINED;
                ++num_fixed;
                if (num_fixed < 2) {
                    if (p_second >= 0)
                        s_moved[nm++] = p_second;
                    else
                        s_err |= PLVI_BA_ERR_UNDEFINED;
                    ++num_fixed;
                }
                s_n_moved = nm;
            }
            s_num_fixed = num_fixed;
        }
        // cam[] turns from stamps into positions in local || fixed
        for (int s = tid; s < a.K; s += kBaThreads) cam[s] = kNoPos;
        __syncthreads();
        const int m0 = s_n_moved > 0 ? s_moved[0] : -1, m1 = s_n_moved > 1 ? s_moved[1] : -1;
        for (int t0 = 0; t0 <= n_row; t0 += kBaThreads) {
            const int t = t0 + tid;
            const int s = t == 0 ? cur : t <= n_row ? row[t - 1] : -1;
            const int flag = (unsigned)s < (unsigned)a.K && (t == 0 || ba_listed(a, s, M)) && s != m0 && s != m1;
            int tot;
            const int at = n_local + block_scan<kBaWaves>(flag, s_wave, tid, &tot);
            if (flag) {
                if (at < o.lkf_cap) o.local_kf[(size_t)q * o.lkf_cap + at] = s;
                atomicMin(cam + s, (unsigned)at);
            }
            n_local += tot;
        }
        __syncthreads();
        const int n_sorted = s_n_fixed;
        for (int i = tid; i < n_sorted; i += kBaThreads) {
            const int s = a.obs_kf[(unsigned)keys[i]];
            if (i < o.fkf_cap) o.fixed_kf[(size_t)q * o.fkf_cap + i] = s;
            cam[s] = n_local + i;
        }
        if (tid == 0) {
            for (int k = 0; k < s_n_moved; ++k) {
                const int at = n_sorted + k;
                if (at < o.fkf_cap) o.fixed_kf[(size_t)q * o.fkf_cap + at] = s_moved[k];
                atomicMin(cam + s_moved[k], (unsigned)(n_local + at));
            }
            s_n_fixed_all = n_sorted + s_n_moved;
        }
    } else {
        if (tid < kWave) {  // :9286-9305
            int nf = 1;
            bool full = nf >= kBaMaxFix;
            for (int j0 = 0; j0 < n_feat && !full; j0 += kWave) {
                const int j = j0 + tid;
                int c = j < n_feat ? ba_choice(a, cam, lf[j]) : -1;
                u64 mask = __ballot(c >= 0);
                while (mask) {
                    const int l = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    int add = 0;
                    if (tid == l) {
                        if (ba_load(cam + c) != kNoPos) c = ba_choice(a, cam, lf[j]);  // an earlier lane took it
                        if (c >= 0) {
                            ba_store(cam + c, kBaFixed);
                            s_fix[nf] = c;
                            add = 1;
                        }
                    }
                    __threadfence_block();
                    nf += __shfl(add, l, kWave);
                    if (nf >= kBaMaxFix) {
                        full = true;
                        break;
                    }
                }
            }
            if (tid == 0) s_n_fixed = nf;
        }
        __syncthreads();
        n_local = s_n_opt;
        const int nf = s_n_fixed;
        for (int s = tid; s < a.K; s += kBaThreads) cam[s] = kNoPos;
        __syncthreads();
        for (int i = tid; i < n_local + nf; i += kBaThreads) {
            const bool opt = i < n_local;
            const int s = opt ? s_chain[i] : s_fix[i - n_local];
            const int cap = opt ? o.lkf_cap : o.fkf_cap, at = opt ? i : i - n_local;
            if (at < cap) (opt ? o.local_kf : o.fixed_kf)[(size_t)q * cap + at] = s;
            atomicMin(cam + s, (unsigned)i);
        }
        if (tid == 0) s_num_fixed = s_n_fixed_all = nf;
    }
    __syncthreads();
    const int n_fixed = s_n_fixed_all;

    // ---- 6: the edges
    int n_edges = 0, n_mono = 0, n_stereo = 0;
    for (int j0 = 0; j0 < n_feat; j0 += kBaThreads) {
        const int j = j0 + tid;
        int id = -1, o0 = 0, o1 = 0, cnt = 0;
        if (j < n_feat) {
            id = lf[j];
            o0 = a.obs_off[id];
            o1 = a.obs_off[id + 1];
            for (int ob = o0; ob < o1; ++ob) cnt += ba_edge(a, cam, ob, M);
        }
        int tot;
        int at = n_edges + block_scan<kBaWaves>(cnt, s_wave, tid, &tot);
        for (int ob = o0; ob < o1 && cnt; ++ob) {
            if (!ba_edge(a, cam, ob, M)) continue;
            const int kf = a.obs_kf[ob], idx = a.obs_idx[ob];
            int kind = PLVI_BA_EDGE_LINE;
            if (a.mode != PLVI_BA_LINES) {
                kind = a.info && (a.info[(size_t)kf * a.cap + idx] & 0x80) ? PLVI_BA_EDGE_STEREO : PLVI_BA_EDGE_MONO;
                n_mono += kind == PLVI_BA_EDGE_MONO;
                n_stereo += kind == PLVI_BA_EDGE_STEREO;
            }
            if (at < o.edge_cap) {
                const size_t e = (size_t)q * o.edge_cap + at;
                o.edge_feat[e] = j;
                o.edge_kf[e] = kf;
                o.edge_idx[e] = idx;
                o.edge_cam[e] = (int)cam[kf];  // kNoPos is -1
                o.edge_kind[e] = (uint8_t)kind;
            }
            ++at;
        }
        n_edges += tot;
    }
    block_add(n_mono, &s_kind[0], tid);
    block_add(n_stereo, &s_kind[1], tid);
    __syncthreads();
    if (tid == 0) {
        const bool lines = a.mode == PLVI_BA_LINES;
        o.n_local_kf[q] = n_local;
        o.n_fixed_kf[q] = n_fixed;
        o.num_fixed[q] = s_num_fixed;
        o.init_in_local[q] = s_init;
        o.non_fixed[q] = n_fixed == 0;
        o.n_local_feat[q] = n_feat;
        o.n_mono[q] = lines ? 0 : s_kind[0];
        o.n_stereo[q] = lines ? 0 : s_kind[1];
        o.n_line[q] = lines ? n_edges : 0;
        o.err[q] = s_err | (n_local > o.lkf_cap ? PLVI_BA_ERR_LOCAL_KF : 0) |
                   (n_fixed > o.fkf_cap ? PLVI_BA_ERR_FIXED_KF : 0) | (n_feat > o.feat_cap ? PLVI_BA_ERR_FEAT : 0) |
                   (n_edges > o.edge_cap ? PLVI_BA_ERR_EDGE : 0);
    }
}

}  // namespace plvi

using namespace plvi;

static int ba_validate(int n_queries, const plvi_cull_keyframes* kf, const int* kf_map_id,
                       const plvi_local_map_pool* mp, const plvi_ba_features* fmp, const plvi_local_map_pool* ml,
                       const plvi_ba_features* fml, const plvi_ba_params* params, const plvi_ba_queries* qs,
                       const plvi_ba_outputs* out, BaArgs* a) {
    if (n_queries < 0 || !kf || !params || !qs || !out) return PLVI_E_BADARG;
    if (params->mode != PLVI_BA_POINTS && params->mode != PLVI_BA_LINES && params->mode != PLVI_BA_INERTIAL)
        return PLVI_E_BADARG;
    const bool lines = params->mode == PLVI_BA_LINES, inertial = params->mode == PLVI_BA_INERTIAL;
    const plvi_local_map_pool* pool = lines ? ml : mp;
    const plvi_ba_features* f = lines ? fml : fmp;
    if (kf->kf_cap < 1 || kf->kp_cap < 0 || kf->kl_cap < 0 || kf->cand_stride < 0 || out->lkf_cap < 0 ||
        out->fkf_cap < 0 || out->feat_cap < 0 || out->edge_cap < 0)
        return PLVI_E_BADARG;
    if (!pool || !pool_ok(pool)) return PLVI_E_BADARG;
    if (inertial && (params->max_opt < 0 || params->max_opt > PLVI_BA_MAX_OPT)) return PLVI_E_BADARG;
    memset(a, 0, sizeof *a);
    if (n_queries == 0) return PLVI_OK;
    const int cap = lines ? kf->kl_cap : kf->kp_cap;
    const int* tab = lines ? kf->ml : kf->mp;
    const int* ntab = lines ? kf->nml : kf->nmp;
    if (!kf->bad || !qs->q_slot) return PLVI_E_BADARG;
    if (cap > 0 && (!tab || !ntab)) return PLVI_E_BADARG;
    if (pool->n > 0 && (!f || !f->obs_idx)) return PLVI_E_BADARG;
    if (!inertial && ((kf->cand_stride > 0 && !kf->cand) || !kf->n_cand)) return PLVI_E_BADARG;
    if (params->mode == PLVI_BA_POINTS && !kf->kf_id) return PLVI_E_BADARG;
    if (inertial && (!kf->prev_kf || !qs->n_kf_in_map)) return PLVI_E_BADARG;
    if (!out->n_local_kf || !out->n_fixed_kf || !out->num_fixed || !out->init_in_local || !out->non_fixed ||
        !out->n_local_feat || !out->n_mono || !out->n_stereo || !out->n_line || !out->err)
        return PLVI_E_BADARG;
    if ((out->lkf_cap > 0 && !out->local_kf) || (out->fkf_cap > 0 && !out->fixed_kf) ||
        (out->feat_cap > 0 && !out->local_feat))
        return PLVI_E_BADARG;
    if (out->edge_cap > 0 &&
        (!out->edge_feat || !out->edge_kf || !out->edge_idx || !out->edge_cam || !out->edge_kind))
        return PLVI_E_BADARG;
    if (n_queries > 65535) return PLVI_E_CAPACITY;
    if ((long long)kf->kf_cap * (kf->kp_cap > kf->kl_cap ? kf->kp_cap : kf->kl_cap) > PLVI_LOCAL_MAP_MAX_ENTRIES)
        return PLVI_E_CAPACITY;
    a->K = kf->kf_cap;
    a->cand_stride = kf->cand_stride;
    a->mode = params->mode;
    a->max_opt = params->max_opt;
    a->n = pool->n;
    a->cap = cap;
    a->P = pow2_at_least(kf->kf_cap, 2);
    a->kf_bad = kf->bad;
    a->init_kf = kf->init_kf;
    a->cand = kf->cand;
    a->n_cand = kf->n_cand;
    a->kf_id = kf->kf_id;
    a->prev_kf = kf->prev_kf;
    a->kf_map = kf_map_id;
    a->tab = tab;
    a->ntab = ntab;
    a->info = lines ? nullptr : kf->kp_info;
    a->f_bad = pool->bad;
    a->obs_off = pool->obs_off;
    a->obs_kf = pool->obs_kf;
    a->obs_idx = f ? f->obs_idx : nullptr;
    a->f_map = f ? f->map_id : nullptr;
    a->q = *qs;
    a->o = *out;
    a->per_query = ba_per_query(a->P, a->K, a->n);
    return PLVI_OK;
}

extern "C" size_t plvi_ba_window_scratch_bytes(int n_queries, int kf_cap, int mp_n, int ml_n) {
    if (n_queries < 0 || kf_cap < 1 || mp_n < 0 || ml_n < 0) return 0;
    return 256 + (size_t)n_queries * ba_per_query(pow2_at_least(kf_cap, 2), kf_cap, mp_n > ml_n ? mp_n : ml_n);
}

extern "C" int plvi_ba_window_batch(int n_queries, const plvi_cull_keyframes* kf, const int* kf_map_id,
                                    const plvi_local_map_pool* mp, const plvi_ba_features* fmp,
                                    const plvi_local_map_pool* ml, const plvi_ba_features* fml,
                                    const plvi_ba_params* params, const plvi_ba_queries* queries,
                                    const plvi_ba_outputs* out, void* d_scratch, size_t scratch_bytes, void* stream) {
    BaArgs a;
    if (int rc = ba_validate(n_queries, kf, kf_map_id, mp, fmp, ml, fml, params, queries, out, &a)) return rc;
    if (n_queries == 0) return PLVI_OK;
    if (!d_scratch || scratch_bytes < 256 + (size_t)n_queries * a.per_query) return PLVI_E_BADARG;
    a.scratch = static_cast<uint8_t*>(d_scratch) + 256;
    hipStream_t st = (hipStream_t)stream;
    if (a.K <= PLVI_BA_LDS_KF)
        return launch_lds<ba_window_kernel<true>>(dim3(n_queries), dim3(kBaThreads),
                                                  (sizeof(u64) + sizeof(unsigned)) * (size_t)a.P, st, a);
    hipLaunchKernelGGL(ba_window_kernel<false>, dim3(n_queries), dim3(kBaThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

static void stage_ba_pool(HostStage& hs, plvi_local_map_pool& p, plvi_ba_features& f) {
    const size_t n = (size_t)p.n;
    const size_t n_obs = p.obs_off && n && p.obs_off[n] > 0 ? (size_t)p.obs_off[n] : 0;
    stage_pool(hs, p, kPoolObs);
    hs.field(f.obs_idx, HostStage::In, n_obs);
    hs.field(f.map_id, HostStage::In, n);
}

// One query from host memory.  Every pointer of the structs is a host pointer here.
extern "C" int plvi_ba_window(const plvi_cull_keyframes* kf, const int* kf_map_id, const plvi_local_map_pool* mp,
                              const plvi_ba_features* fmp, const plvi_local_map_pool* ml,
                              const plvi_ba_features* fml, const plvi_ba_params* params,
                              const plvi_ba_queries* queries, const plvi_ba_outputs* out) {
    BaArgs chk;
    if (int rc = ba_validate(1, kf, kf_map_id, mp, fmp, ml, fml, params, queries, out, &chk)) return rc;
    const bool lines = params->mode == PLVI_BA_LINES, inertial = params->mode == PLVI_BA_INERTIAL;
    const size_t K = (size_t)kf->kf_cap;
    // copies of the caller's structs: commit() turns their host pointers into device pointers
    plvi_cull_keyframes dk = *kf;
    plvi_local_map_pool dp = lines ? *ml : *mp;
    const plvi_ba_features* f = lines ? fml : fmp;
    plvi_ba_features df = f ? *f : plvi_ba_features{};
    plvi_ba_queries dq = *queries;
    plvi_ba_outputs dout = *out;
    const int* dmap = kf_map_id;
    // only what the mode reads travels
    dk.not_erase = nullptr;
    dk.timestamp = nullptr;
    dk.next_kf = nullptr;
    dk.kl_info = nullptr;
    if (lines) dk.mp = dk.nmp = nullptr, dk.kp_info = nullptr;
    if (!lines) dk.ml = dk.nml = nullptr;
    if (params->mode != PLVI_BA_POINTS) dk.kf_id = nullptr;
    if (inertial) dk.cand = dk.n_cand = nullptr;
    if (!inertial) dk.prev_kf = nullptr, dq.n_kf_in_map = nullptr;
    HostStage hs;
    const HostStage::Dir In = HostStage::In, Out = HostStage::Out, InOut = HostStage::InOut;
    hs.field(dk.bad, In, K);
    hs.field(dk.init_kf, In, K);
    hs.field(dk.mp, In, K, kf->kp_cap);
    hs.field(dk.nmp, In, K);
    hs.field(dk.kp_info, In, K, kf->kp_cap);
    hs.field(dk.ml, In, K, kf->kl_cap);
    hs.field(dk.nml, In, K);
    hs.field(dk.cand, In, K, kf->cand_stride);
    hs.field(dk.n_cand, In, K);
    hs.field(dk.kf_id, In, K);
    hs.field(dk.prev_kf, In, K);
    hs.field(dmap, In, K);
    stage_ba_pool(hs, dp, df);
    hs.field(dq.q_slot, In, 1);
    hs.field(dq.n_kf_in_map, In, 1);
    for (int** p : {&dout.n_local_kf, &dout.n_fixed_kf, &dout.num_fixed, &dout.init_in_local, &dout.non_fixed,
                    &dout.n_local_feat, &dout.n_mono, &dout.n_stereo, &dout.n_line, &dout.err})
        hs.field(*p, Out, 1);
    // in/out: cells past a list's end keep the caller's fill
    hs.field(dout.local_kf, InOut, out->lkf_cap);
    hs.field(dout.fixed_kf, InOut, out->fkf_cap);
    hs.field(dout.local_feat, InOut, out->feat_cap);
    hs.field(dout.edge_feat, InOut, out->edge_cap);
    hs.field(dout.edge_kf, InOut, out->edge_cap);
    hs.field(dout.edge_idx, InOut, out->edge_cap);
    hs.field(dout.edge_cam, InOut, out->edge_cap);
    hs.field(dout.edge_kind, InOut, out->edge_cap);
    const size_t sb = plvi_ba_window_scratch_bytes(1, kf->kf_cap, dp.n, 0);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_ba_window_batch(1, &dk, dmap, lines ? nullptr : &dp, lines ? nullptr : &df,
                                      lines ? &dp : nullptr, lines ? &df : nullptr, params, &dq, &dout,
                                      hs.dev(scr), sb, nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err & ~PLVI_BA_ERR_UNDEFINED ? PLVI_E_CAPACITY : PLVI_OK;
}
