// cull.hip — LocalMapping::KeyFrameCulling() / KeyFrameCullingWithLines() (src/LocalMapping.cc:
// 1566-1718 / :1720-1964) for a batch of current keyframes: the redundancy walk over the covisibles,
// with the observation erasures of KeyFrame::SetBadFlag[WithLines] (src/KeyFrame.cc:900-907,
// :1035-1050), MapPoint / MapLine::EraseObservation (src/MapPoint.cc:168-202, src/MapLine.cc:
// 131-157) and the mPrevKF / mNextKF relinks kept in an overlay.  Integers, one float
// multiply-compare and one double subtraction.
//
// The loop is sequential, but its state is small: nObs only decreases, so a feature's live
// Observations() and whether it died are functions of the SET of keyframes erased so far --
//   live nObs = nobs - sum over its observations by an erased keyframe of (info bit 7 ? 2 : 1)
//   dead      = it has such an observation and live nObs <= 2
// and a walk erases at most 101 keyframes (a cull does not `continue`, so the break test follows
// it).  That set is a list in LDS, found through a 2048-bit filter, whatever kf_cap is.
//   cull_count_kernel one workgroup per (candidate, query), speculative: the counts of the first
//                     PLVI_CULL_SPEC candidates from `start` against the overlay known at launch
//                     (the pre list of a resumed query, nothing for a fresh one).  A thread per
//                     table entry walks the entry's observation list once (erased observers
//                     subtract, the others are compared by octave); the sums are added up in LDS.
//   cull_walk_kernel  one workgroup per query.  It takes a candidate's speculative counts as long
//                     as this call has erased nothing, and from the first erasure on counts each
//                     candidate itself with the whole workgroup under the current overlay; thread
//                     0 does the test, the gates, the relinks and the outcome, and appends to the
//                     overlay.  A resumed query rebuilds its overlay from the pre list with the
//                     same apply() first.
// PLVI_CULL_SPECULATE=0 builds the walk kernel alone, everything counted in order (the A/B of
// DESIGN.md section 24).
#include <cstring>

#include "block_prims.h"
#include "map_pool.h"
#include "plvi_common.h"

#ifndef PLVI_CULL_SPECULATE
#define PLVI_CULL_SPECULATE 1
#endif

namespace plvi {

constexpr bool kCullSpeculate = PLVI_CULL_SPECULATE;
constexpr int kCullSpec = PLVI_CULL_SPEC;
constexpr int kCullThreads = 256;
constexpr int kCullMax = PLVI_CULL_MAX_CHANGED;
constexpr int kCullChain = 3 * kCullMax;  // a relink rewrites three keyframes' links
constexpr int kCullFilt = 2048;           // bits
constexpr int kCullNd = 21;               // Nd of :1572

typedef unsigned long long u64;

struct CullPool {
    int n, cap;  // features; row length of the keyframe table
    const uint8_t* bad;
    const int *obs_off, *obs_kf, *obs_idx, *nobs;
    const int *tab, *ntab;  // [K][cap], [K]
    const uint8_t* info;    // [K][cap]
};

struct CullArgs {
    int K, cand_stride, with_lines, monocular, inertial, slam_mode;
    float th;
    const uint8_t *kf_bad, *init_kf, *not_erase;
    CullPool p[2];
    const int *cand, *n_cand;
    const unsigned* kf_id;
    const double* ts;
    const int *prev_kf, *next_kf;
    plvi_cull_queries q;
    plvi_cull_outputs o;
    int4* spec;  // [queries][kCullSpec] nMPs, their redundant ones, nMLs, theirs; by position - start
};

struct CullOverlay {  // LDS
    int n;                               // entries of slot / kind (the changed list)
    int n_erased;                        // of them, with PLVI_CULL_KIND_POINTS
    int slot[kCullMax], kind[kCullMax];
    unsigned filt[kCullFilt / 32];       // slots with PLVI_CULL_KIND_POINTS, by slot % kCullFilt
    int n_chain;
    int c_slot[kCullChain], c_prev[kCullChain], c_next[kCullChain];
    int n_kf, err;
};

// was slot `kf` erased with a kind that has `mask`?  (every thread)
__device__ __forceinline__ bool cull_erased(const CullOverlay& ov, int kf, int mask) {
    if (!(ov.filt[(kf & (kCullFilt - 1)) >> 5] >> (kf & 31) & 1)) return false;
    for (int j = 0; j < ov.n; ++j)
        if (ov.slot[j] == kf && (ov.kind[j] & mask)) return true;
    return false;
}

// thread 0: the links of a slot under the overlay
__device__ void cull_links(const CullOverlay& ov, const CullArgs& a, int s, int* prev, int* next) {
    for (int j = ov.n_chain - 1; j >= 0; --j)
        if (ov.c_slot[j] == s) {
            *prev = ov.c_prev[j];
            *next = ov.c_next[j];
            return;
        }
    const int p = a.prev_kf[s], n = a.next_kf[s];
    *prev = (unsigned)p < (unsigned)a.K ? p : -1;
    *next = (unsigned)n < (unsigned)a.K ? n : -1;
}

__device__ void cull_set_links(CullOverlay& ov, int s, int prev, int next) {
    for (int j = 0; j < ov.n_chain; ++j)
        if (ov.c_slot[j] == s) {
            ov.c_prev[j] = prev;
            ov.c_next[j] = next;
            return;
        }
    if (ov.n_chain < kCullChain) {
        ov.c_slot[ov.n_chain] = s;
        ov.c_prev[ov.n_chain] = prev;
        ov.c_next[ov.n_chain] = next;
        ++ov.n_chain;
    }
}

// thread 0: an entry joins the list (ov.n < kCullMax) and, erased, the filter
__device__ void cull_mark(CullOverlay& ov, int s, int kind) {
    ov.slot[ov.n] = s;
    ov.kind[ov.n] = kind;
    if (kind & PLVI_CULL_KIND_POINTS) {
        ov.filt[(s & (kCullFilt - 1)) >> 5] |= 1u << (s & 31);
        ++ov.n_erased;
        --ov.n_kf;  // Map::EraseKeyFrame at the end of SetBadFlag
    }
    ++ov.n;
}

// thread 0: one entry of the changed list takes effect -- a cull inside the loop, or an entry of
// the pre list of a resumed query
__device__ void cull_apply(CullOverlay& ov, const CullArgs& a, int q, int s, int kind) {
    if (ov.n >= kCullMax) {
        ov.err |= PLVI_CULL_ERR_CHANGED;
        return;
    }
    if (ov.n < a.o.changed_cap) {
        a.o.changed_slot[(size_t)q * a.o.changed_cap + ov.n] = s;
        a.o.changed_kind[(size_t)q * a.o.changed_cap + ov.n] = kind;
    } else {
        ov.err |= PLVI_CULL_ERR_CHANGED;
    }
    if (kind & PLVI_CULL_KIND_RELINKED) {  // :1691-1694, before SetBadFlag
        int p, n;
        cull_links(ov, a, s, &p, &n);
        if (p >= 0 && n >= 0) {
            int x, y;
            cull_links(ov, a, n, &x, &y);
            cull_set_links(ov, n, p, y);  // next->mPrevKF = prev
            cull_links(ov, a, p, &x, &y);
            cull_set_links(ov, p, x, n);  // prev->mNextKF = next
            cull_set_links(ov, s, -1, -1);
        }
    }
    cull_mark(ov, s, kind);
}

// Every thread: nMPs / nRedundant (or nMLs / ...) of keyframe K into cnt[0], cnt[1] (zeroed, and
// a barrier passed, before; a barrier is due after).  `need` other observers make an entry redundant.
__device__ void cull_count(const CullOverlay& ov, const CullPool& p, int K, int kf_cap, bool monocular, int erase_mask,
                           int need, int* cnt, int tid) {
    if (p.cap <= 0 || p.n <= 0) return;
    const int* tab = p.tab + (size_t)K * p.cap;
    const uint8_t* info = p.info + (size_t)K * p.cap;
    const int n = clampi(p.ntab[K], 0, p.cap);
    const bool any_erased = ov.n_erased > 0;
    int n_f = 0, n_red = 0;
    for (int i = tid; i < n; i += kCullThreads) {
        const int id = tab[i];
        if ((unsigned)id >= (unsigned)p.n || p.bad[id]) continue;
        const int own = info[i];
        if (!monocular && (own & 0x40)) continue;
        const int o0 = p.obs_off[id], o1 = p.obs_off[id + 1];
        int hits = 0, lost = 0;
        for (int o = o0; o < o1; ++o) {
            const int kf = p.obs_kf[o], idx = p.obs_idx[o];
            if ((unsigned)kf >= (unsigned)kf_cap || (unsigned)idx >= (unsigned)p.cap) continue;
            const int inf = p.info[(size_t)kf * p.cap + idx];
            if (any_erased && cull_erased(ov, kf, erase_mask))
                lost += inf & 0x80 ? 2 : 1;
            else if (kf != K && (inf & 63) <= (own & 63) + 1)
                ++hits;
        }
        const int live = (p.nobs ? p.nobs[id] : o1 - o0) - lost;
        if (lost && live <= 2) continue;  // died in an earlier SetBadFlag: bad
        ++n_f;
        n_red += live > 3 && hits >= need;
    }
    // not wave_sum: with the __shfl_xor butterfly the compiler schedules the whole count loop
    // differently and a count takes 1.8 % longer (profiles/r18/cull.txt); only lane 0 reads the sums
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        n_f += __shfl_down(n_f, m, kWave);
        n_red += __shfl_down(n_red, m, kWave);
    }
    if ((tid & (kWave - 1)) == 0) {
        if (n_f) atomicAdd(cnt, n_f);
        if (n_red) atomicAdd(cnt + 1, n_red);
    }
}

// Every thread: the overlay of query q as it stands before the walk -- empty, or rebuilt from the
// pre list.  The walk kernel (kWalk) writes the list forward to the changed list and relinks; the
// count kernel needs the erased set alone.  Ends with a barrier.
template <bool kWalk>
__device__ void cull_begin(CullOverlay& ov, const CullArgs& a, int q, bool query_ok, int tid) {
    for (int i = tid; i < kCullFilt / 32; i += kCullThreads) ov.filt[i] = 0;
    __syncthreads();
    if (tid == 0) {
        ov.n = ov.n_erased = ov.n_chain = 0;
        ov.n_kf = a.q.n_kf_in_map[q];
        ov.err = query_ok ? 0 : PLVI_CULL_ERR_QUERY;
        if (query_ok && a.q.pre_n) {
            int pre_n = a.q.pre_n[q];
            const int lim = min(a.q.pre_cap, kCullMax);
            if (pre_n < 0 || pre_n > lim) {
                ov.err |= PLVI_CULL_ERR_PRE;
                pre_n = clampi(pre_n, 0, lim);
            }
            for (int j = 0; j < pre_n; ++j) {
                const int s = a.q.pre_slot[(size_t)q * a.q.pre_cap + j], kind = a.q.pre_kind[(size_t)q * a.q.pre_cap + j];
                if ((unsigned)s >= (unsigned)a.K || (kind & ~15) || kind == 0)
                    ov.err |= PLVI_CULL_ERR_PRE;
                else if (kWalk)
                    cull_apply(ov, a, q, s, kind);
                else
                    cull_mark(ov, s, kind);
            }
        }
    }
    __syncthreads();
}

// :1608 for candidate K -- uniform, every thread evaluates it; 0 = the body runs
__device__ __forceinline__ int cull_skip(const CullOverlay& ov, const CullArgs& a, int K) {
    if ((unsigned)K >= (unsigned)a.K) return PLVI_CULL_SKIP_BAD;
    if (a.init_kf && a.init_kf[K]) return PLVI_CULL_SKIP_INIT;
    if (a.kf_bad[K] || (ov.n_erased && cull_erased(ov, K, PLVI_CULL_KIND_POINTS))) return PLVI_CULL_SKIP_BAD;
    return 0;
}

// Every thread: both tables of K counted into cnt[0..3] (two barriers)
__device__ void cull_count_both(const CullOverlay& ov, const CullArgs& a, int K, int* cnt, int tid) {
    if (tid < 4) cnt[tid] = 0;
    __syncthreads();  // and thread 0's changes to the overlay are seen
    cull_count(ov, a.p[0], K, a.K, a.monocular, PLVI_CULL_KIND_POINTS, 4, cnt, tid);
    if (a.with_lines) cull_count(ov, a.p[1], K, a.K, a.monocular, PLVI_CULL_KIND_LINES, 3, cnt + 2, tid);
    __syncthreads();
}

__global__ __launch_bounds__(kCullThreads) void cull_count_kernel(CullArgs a) {
    __shared__ CullOverlay ov;
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, j = blockIdx.x, q = blockIdx.y;
    const int cur = a.q.q_slot[q];
    const int start = a.q.start ? a.q.start[q] : 0;
    if ((unsigned)cur >= (unsigned)a.K || start < 0) return;
    if (j >= clampi(a.n_cand[cur], 0, a.cand_stride) - start) return;  // start + j without overflow
    const int K = a.cand[(size_t)cur * a.cand_stride + start + j];
    if ((unsigned)K >= (unsigned)a.K || (a.init_kf && a.init_kf[K]) || a.kf_bad[K]) return;  // the walk skips it
    cull_begin<false>(ov, a, q, true, tid);
    cull_count_both(ov, a, K, s_cnt, tid);
    if (tid == 0) a.spec[(size_t)q * kCullSpec + j] = make_int4(s_cnt[0], s_cnt[1], s_cnt[2], s_cnt[3]);
}

__global__ __launch_bounds__(kCullThreads) void cull_walk_kernel(CullArgs a) {
    __shared__ CullOverlay ov;
    __shared__ int s_cnt[4];
    __shared__ int s_flow;  // 0 = next candidate, 1 = the walk is over
    const int tid = threadIdx.x, q = blockIdx.x;
    const int cur = a.q.q_slot[q];
    const int start = a.q.start ? a.q.start[q] : 0;
    const bool query_ok = (unsigned)cur < (unsigned)a.K && start >= 0;

    unsigned last_id = 0;
    if (tid == 0 && query_ok && a.inertial) {  // :1588-1599, on the unmodified chain
        int aux = cur;
        for (int c = 0; c < kCullNd; ++c) {
            const int p = a.prev_kf[aux];
            if ((unsigned)p >= (unsigned)a.K) break;
            aux = p;
        }
        last_id = a.kf_id[aux];
    }
    cull_begin<true>(ov, a, q, query_ok, tid);
    const int n_erased0 = ov.n_erased;

    const int n_cand = query_ok ? clampi(a.n_cand[cur], 0, a.cand_stride) : 0;
    const int verdict = a.q.verdict ? a.q.verdict[q] : -1;
    const int* cand = a.cand + (size_t)(query_ok ? cur : 0) * a.cand_stride;
    int stop = PLVI_CULL_STOP_END;
    int p = query_ok ? start : 0;
    for (; p < n_cand; ++p) {
        const int K = cand[p];
        const bool in_tab = p < a.o.out_cap;
        const size_t cell = (size_t)q * a.o.out_cap + p;
        const int skip = cull_skip(ov, a, K);
        if (skip) {
            if (tid == 0) {
                if (in_tab) {
                    a.o.outcome[cell] = (uint8_t)skip;
                    a.o.n_mps[cell] = a.o.n_mls[cell] = a.o.n_redundant[cell] = 0;
                } else {
                    ov.err |= PLVI_CULL_ERR_OUT;
                }
            }
            continue;
        }
        // the counts taken at launch hold until this call erases something
        const bool spec = kCullSpeculate && ov.n_erased == n_erased0 && p - start < kCullSpec;
        if (spec)
            __syncthreads();  // every thread has read the overlay before thread 0 changes it
        else
            cull_count_both(ov, a, K, s_cnt, tid);
        if (tid == 0) {
            const int4 c = spec ? a.spec[(size_t)q * kCullSpec + (p - start)]
                                : make_int4(s_cnt[0], s_cnt[1], s_cnt[2], s_cnt[3]);
            const int n_mps = c.x, n_mls = c.z;
            int n_red, n;
            if (!a.with_lines) {
                n_red = c.y;
                n = n_mps;
            } else if (a.slam_mode == 0) {
                n_red = c.y + c.w;
                n = n_mps + n_mls;
            } else {
                n_red = c.w;
                n = n_mls;
            }
            int code = PLVI_CULL_KEEP, flow = 0;
            bool cont = false;  // a `continue` of the reference: no break test
            if ((float)n_red > __fmul_rn(a.th, (float)n)) {
                const bool keep_alive = a.not_erase && a.not_erase[K];
                if (!a.inertial) {
                    code = PLVI_CULL_CULLED;
                    cull_apply(ov, a, q, K,
                               keep_alive ? PLVI_CULL_KIND_DEFERRED
                                          : PLVI_CULL_KIND_POINTS | (a.with_lines ? PLVI_CULL_KIND_LINES : 0));
                    if (keep_alive) code |= PLVI_CULL_DEFERRED;
                } else if (ov.n_kf <= kCullNd) {
                    code = PLVI_CULL_KEEP_FEW_KF;
                    cont = true;
                } else if ((u64)a.kf_id[K] > (u64)a.kf_id[cur] - 2) {
                    code = PLVI_CULL_KEEP_RECENT;
                    cont = true;
                } else {
                    int pv, nx;
                    cull_links(ov, a, K, &pv, &nx);
                    if (pv < 0 || nx < 0) {
                        code = PLVI_CULL_KEEP_NO_CHAIN;
                    } else {
                        const float t = (float)(a.ts[nx] - a.ts[pv]);
                        bool cull = false;
                        if ((a.q.imu_init[q] && a.kf_id[K] < last_id && t < 3.f) || t < 0.5f) {
                            code = PLVI_CULL_CULLED_TIME;
                            cull = true;
                        } else if (a.q.inertial_ba2[q] || !(t < 3.f)) {
                            code = PLVI_CULL_KEEP_TIME;
                        } else if (p == start && verdict >= 0) {
                            code = verdict ? PLVI_CULL_CULLED_NORM : PLVI_CULL_KEEP_NORM;
                            cull = verdict != 0;
                        } else {
                            code = PLVI_CULL_NEEDS_NORM;
                            stop = PLVI_CULL_STOP_NEEDS_NORM;
                            flow = 1;
                        }
                        if (cull) {
                            cull_apply(ov, a, q, K,
                                       PLVI_CULL_KIND_RELINKED |
                                           (keep_alive ? PLVI_CULL_KIND_DEFERRED : PLVI_CULL_KIND_POINTS));
                            if (keep_alive) code |= PLVI_CULL_DEFERRED;
                        }
                    }
                }
            }
            if (in_tab) {
                a.o.outcome[cell] = (uint8_t)code;
                a.o.n_mps[cell] = n_mps;
                a.o.n_mls[cell] = n_mls;
                a.o.n_redundant[cell] = n_red;
            } else {
                ov.err |= PLVI_CULL_ERR_OUT;
            }
            if (!cont && !flow) {  // :1713
                const int count = p + 1;
                if (count > 20 && a.q.abort_ba[q]) {
                    stop = PLVI_CULL_STOP_BREAK_ABORT;
                    flow = 1;
                } else if (count > 100) {
                    stop = PLVI_CULL_STOP_BREAK_100;
                    flow = 1;
                }
            }
            s_flow = flow;
        }
        __syncthreads();
        if (s_flow) {
            ++p;
            break;
        }
    }
    if (tid == 0) {
        a.o.n_visited[q] = query_ok ? max(p, start) : 0;
        a.o.stop[q] = stop;
        a.o.n_kf_in_map[q] = ov.n_kf;
        a.o.err[q] = ov.err;
        a.o.n_changed[q] = ov.n;
    }
}

}  // namespace plvi

using namespace plvi;

static bool cull_pool(CullPool& c, const plvi_local_map_pool* p, const plvi_cull_features* f, int cap, const int* tab,
                      const int* ntab, const uint8_t* info) {
    c = CullPool{};
    if (!p || !pool_ok(p)) return false;
    c.cap = cap;
    if (p->n == 0 || cap == 0) return true;  // nothing to count
    if (!f || !f->obs_idx || !tab || !ntab || !info) return false;
    c.n = p->n;
    c.bad = p->bad;
    c.obs_off = p->obs_off;
    c.obs_kf = p->obs_kf;
    c.obs_idx = f->obs_idx;
    c.nobs = f->nobs;
    c.tab = tab;
    c.ntab = ntab;
    c.info = info;
    return true;
}

static int cull_validate(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                         const plvi_cull_features* fmp, const plvi_local_map_pool* ml, const plvi_cull_features* fml,
                         const plvi_cull_params* params, const plvi_cull_queries* qs, const plvi_cull_outputs* out,
                         CullArgs* a) {
    if (n_queries < 0 || !kf || !mp || !params || !qs || !out) return PLVI_E_BADARG;
    if (kf->kf_cap < 1 || kf->kp_cap < 0 || kf->kl_cap < 0 || kf->cand_stride < 0 || out->out_cap < 0 ||
        out->changed_cap < 0 || qs->pre_cap < 0)
        return PLVI_E_BADARG;
    const bool with_lines = kf->ml && ml;
    memset(a, 0, sizeof *a);
    if (!cull_pool(a->p[0], mp, fmp, kf->kp_cap, kf->mp, kf->nmp, kf->kp_info)) return PLVI_E_BADARG;
    if (with_lines && !cull_pool(a->p[1], ml, fml, kf->kl_cap, kf->ml, kf->nml, kf->kl_info)) return PLVI_E_BADARG;
    if (n_queries == 0) return PLVI_OK;
    if (!kf->bad || (kf->cand_stride > 0 && !kf->cand) || !kf->n_cand) return PLVI_E_BADARG;
    if (params->inertial && (!kf->kf_id || !kf->timestamp || !kf->prev_kf || !kf->next_kf)) return PLVI_E_BADARG;
    if (!qs->q_slot || !qs->abort_ba || !qs->n_kf_in_map || !qs->imu_init || !qs->inertial_ba2) return PLVI_E_BADARG;
    const int n_resume = !!qs->start + !!qs->verdict + !!qs->pre_n + !!qs->pre_slot + !!qs->pre_kind;
    if (n_resume != 0 && n_resume != 5) return PLVI_E_BADARG;
    if (!out->n_visited || !out->stop || !out->n_kf_in_map || !out->err || !out->n_changed) return PLVI_E_BADARG;
    if (out->out_cap > 0 && (!out->outcome || !out->n_mps || !out->n_mls || !out->n_redundant)) return PLVI_E_BADARG;
    if (out->changed_cap > 0 && (!out->changed_slot || !out->changed_kind)) return PLVI_E_BADARG;
    if (n_queries > 65535) return PLVI_E_CAPACITY;
    a->K = kf->kf_cap;
    a->cand_stride = kf->cand_stride;
    a->with_lines = with_lines;
    a->monocular = params->monocular != 0;
    a->inertial = params->inertial != 0;
    a->slam_mode = params->slam_mode;
    a->th = params->redundant_th;
    a->kf_bad = kf->bad;
    a->init_kf = kf->init_kf;
    a->not_erase = kf->not_erase;
    a->cand = kf->cand;
    a->n_cand = kf->n_cand;
    a->kf_id = kf->kf_id;
    a->ts = kf->timestamp;
    a->prev_kf = kf->prev_kf;
    a->next_kf = kf->next_kf;
    a->q = *qs;
    a->o = *out;
    return PLVI_OK;
}

extern "C" size_t plvi_keyframe_culling_scratch_bytes(int n_queries) {
    return n_queries < 0 ? 0 : 256 + sizeof(int4) * (size_t)n_queries * kCullSpec;
}

extern "C" int plvi_keyframe_culling_batch(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                                           const plvi_cull_features* fmp, const plvi_local_map_pool* ml,
                                           const plvi_cull_features* fml, const plvi_cull_params* params,
                                           const plvi_cull_queries* queries, const plvi_cull_outputs* out,
                                           void* d_scratch, size_t scratch_bytes, void* stream) {
    CullArgs a;
    if (int rc = cull_validate(n_queries, kf, mp, fmp, ml, fml, params, queries, out, &a)) return rc;
    if (n_queries == 0) return PLVI_OK;
    if (!d_scratch || scratch_bytes < plvi_keyframe_culling_scratch_bytes(n_queries)) return PLVI_E_BADARG;
    a.spec = reinterpret_cast<int4*>(static_cast<uint8_t*>(d_scratch) + 256);
    hipStream_t st = (hipStream_t)stream;
    const int n_spec = a.cand_stride < kCullSpec ? a.cand_stride : kCullSpec;
    if (kCullSpeculate && n_spec > 0) {
        hipLaunchKernelGGL(cull_count_kernel, dim3(n_spec, n_queries), dim3(kCullThreads), 0, st, a);
        PLVI_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(cull_walk_kernel, dim3(n_queries), dim3(kCullThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

static void stage_cull_pool(HostStage& hs, plvi_local_map_pool& p, plvi_cull_features& f) {
    const size_t n = (size_t)p.n;
    const size_t n_obs = p.obs_off && n && p.obs_off[n] > 0 ? (size_t)p.obs_off[n] : 0;
    stage_pool(hs, p, kPoolObs);
    hs.field(f.obs_idx, HostStage::In, n_obs);
    hs.field(f.nobs, HostStage::In, n);
}

// One query from host memory.  Every pointer of the structs is a host pointer here.
extern "C" int plvi_keyframe_culling(const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                                     const plvi_cull_features* fmp, const plvi_local_map_pool* ml,
                                     const plvi_cull_features* fml, const plvi_cull_params* params,
                                     const plvi_cull_queries* queries, const plvi_cull_outputs* out) {
    CullArgs chk;
    if (int rc = cull_validate(1, kf, mp, fmp, ml, fml, params, queries, out, &chk)) return rc;
    const bool with_lines = kf->ml && ml;
    const size_t K = (size_t)kf->kf_cap;
    // copies of the caller's structs: commit() turns their host pointers into device pointers
    plvi_cull_keyframes dk = *kf;
    plvi_local_map_pool dmp = *mp, dml = with_lines ? *ml : plvi_local_map_pool{};
    plvi_cull_features dfmp = fmp ? *fmp : plvi_cull_features{}, dfml = with_lines && fml ? *fml : plvi_cull_features{};
    plvi_cull_queries dq = *queries;
    plvi_cull_outputs dout = *out;
    if (!with_lines) dk.ml = dk.nml = nullptr, dk.kl_info = nullptr;
    if (!params->inertial) {
        dk.kf_id = nullptr;
        dk.timestamp = nullptr;
        dk.prev_kf = dk.next_kf = nullptr;
    }
    HostStage hs;
    const HostStage::Dir In = HostStage::In, Out = HostStage::Out;
    hs.field(dk.bad, In, K);
    hs.field(dk.init_kf, In, K);
    hs.field(dk.not_erase, In, K);
    hs.field(dk.mp, In, K, kf->kp_cap);
    hs.field(dk.nmp, In, K);
    hs.field(dk.kp_info, In, K, kf->kp_cap);
    hs.field(dk.ml, In, K, kf->kl_cap);
    hs.field(dk.nml, In, K);
    hs.field(dk.kl_info, In, K, kf->kl_cap);
    hs.field(dk.cand, In, K, kf->cand_stride);
    hs.field(dk.n_cand, In, K);
    hs.field(dk.kf_id, In, K);
    hs.field(dk.timestamp, In, K);
    hs.field(dk.prev_kf, In, K);
    hs.field(dk.next_kf, In, K);
    stage_cull_pool(hs, dmp, dfmp);
    if (with_lines) stage_cull_pool(hs, dml, dfml);
    for (const int** f : {&dq.q_slot, &dq.abort_ba, &dq.n_kf_in_map, &dq.imu_init, &dq.inertial_ba2, &dq.start,
                          &dq.verdict, &dq.pre_n})
        hs.field(*f, In, 1);
    hs.field(dq.pre_slot, In, queries->pre_cap);
    hs.field(dq.pre_kind, In, queries->pre_cap);
    for (int** o : {&dout.n_visited, &dout.stop, &dout.n_kf_in_map, &dout.err, &dout.n_changed}) hs.field(*o, Out, 1);
    // in/out: cells the walk does not write keep the caller's fill
    const HostStage::Dir InOut = HostStage::InOut;
    hs.field(dout.outcome, InOut, out->out_cap);
    hs.field(dout.n_mps, InOut, out->out_cap);
    hs.field(dout.n_mls, InOut, out->out_cap);
    hs.field(dout.n_redundant, InOut, out->out_cap);
    hs.field(dout.changed_slot, InOut, out->changed_cap);
    hs.field(dout.changed_kind, InOut, out->changed_cap);
    const size_t sb = plvi_keyframe_culling_scratch_bytes(1);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_keyframe_culling_batch(1, &dk, &dmp, &dfmp, with_lines ? &dml : nullptr,
                                             with_lines ? &dfml : nullptr, params, &dq, &dout, hs.dev(scr), sb,
                                             nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err ? PLVI_E_CAPACITY : PLVI_OK;
}
