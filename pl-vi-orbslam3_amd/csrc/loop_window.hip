// loop_window.hip — the integer work between the device calls of LoopClosing::NewDetectCommonRegions
// (src/LoopClosing.cc): the six-keyframe window around a BoW candidate and its abort by proximity
// (:797-804, :833-840), the first-come merge of the six SearchByBoW results (:818-858), the covisible
// window of DetectCommonRegionsFromBoW with its point cloud and owners (:893-915) and the window of
// FindMatchesByProjection (:1162-1199).  Integers only.
//
// The reference's std::set<MapPoint*> makes "first come" decisions along a fixed traversal; here they are
// the first-occurrence walk of first_walk.h, with its reset (the scratch block needs no fill):
//   window        thread 0: at most PLVI_LOOP_WIN_MAX slots, and dl[], the window without its repeats
//                 and without the entries that name no slot (neither contributes a table).
//   abort_at      the connected set is walked by the whole workgroup, each entry against the window:
//                 atomicMin of the window position in LDS.
//   point cloud   the walk over the rows of dl[].
//   gathers       a second launch over (256-point chunks, queries): the gather of map_pool.h.
//   merge         the mark pass over position j * n1 + k of at most 6 * cap1 matches; entry (j, k) wins
//                 iff it holds its point's minimum, cell k takes the winner of the largest j, num is the
//                 number of winners.
// One workgroup per query in both list kernels.
#include <climits>
#include <cstring>

#include "first_walk.h"
#include "map_pool.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kLwThreads = 1024;
constexpr int kLwWaves = kLwThreads / kWave;
constexpr int kLwCov = PLVI_LOOP_COVISIBLES, kLwBow = PLVI_LOOP_BOW_WIN, kLwWin = PLVI_LOOP_WIN_MAX;
constexpr int kLwGather = 256;  // points per workgroup of the gather

struct LwTables {
    int K, cand_stride;
    const uint8_t* kf_bad;
    KfTable v;  // the keypoint tables [K][kp_cap] over the MapPoint pool (:905 / :1190 / :846)
    const int *cand, *n_cand;
    unsigned* first;  // [n_queries][n], in the scratch block
};

struct LwArgs {
    LwTables t;
    plvi_loop_queries q;
    plvi_loop_outputs o;
};

struct LwMergeArgs {
    LwTables t;
    int cap1;
    const int *win, *n_win, *abort_at, *m12, *n1;
    int *matched_mp, *matched_kf, *num;
};

inline size_t lw_per_query(int n) { return 4 * (size_t)n; }  // first[n]

// GetBestCovisibilityKeyFrames(5) of slot s (in range) as stored; returns the length
__device__ int lw_cov(const LwTables& t, int s, int* out) {
    const int n = min(clampi(t.n_cand[s], 0, t.cand_stride), kLwCov);
    for (int i = 0; i < n; ++i) out[i] = t.cand[(size_t)s * t.cand_stride + i];
    return n;
}

__global__ __launch_bounds__(kLwThreads) void loop_window_kernel(LwArgs a) {
    __shared__ int s_wave[kLwWaves];
    __shared__ int s_win[kLwWin], s_dl[kLwWin];
    __shared__ int s_n_win, s_n_dl, s_err, s_abort;
    const int tid = threadIdx.x, q = blockIdx.x;
    const LwTables& t = a.t;
    const plvi_loop_outputs& o = a.o;
    const int kind = a.q.kind[q], m = a.q.kf_slot[q];
    const bool bow = kind == PLVI_LOOP_WIN_BOW;

    if (tid == 0) {
        int n = 0, err = 0;
        const bool known = bow || kind == PLVI_LOOP_WIN_PROJ || kind == PLVI_LOOP_WIN_LAST;
        if (!known || !in_range(m, t.K) || (bow && a.q.cur_slot && !in_range(a.q.cur_slot[q], t.K))) {
            err = PLVI_LOOP_ERR_QUERY;
        } else if (bow) {
            if (!t.kf_bad[m]) {  // :797
                int c[kLwCov];
                const int nc = lw_cov(t, m, c);
                s_win[n++] = m;  // push_back(front), [0] = pKFi: c0 goes last
                for (int i = 1; i < nc; ++i) s_win[n++] = c[i];
                if (nc)
                    s_win[n++] = c[0];
                else
                    err = PLVI_LOOP_ERR_UNDEFINED;
            }
        } else {
            const int nc = lw_cov(t, m, s_win);
            n = nc;
            s_win[n++] = m;
            if (kind == PLVI_LOOP_WIN_LAST)  // :1167-1182: every row is appended whole
                for (int i = 0; i < nc; ++i)
                    if (in_range(s_win[i], t.K)) n += lw_cov(t, s_win[i], s_win + n);
        }
        int n_dl = 0;
        for (int w = 0; w < n && !bow; ++w) {
            const int s = s_win[w];
            bool fresh = in_range(s, t.K);
            for (int r = 0; r < n_dl && fresh; ++r) fresh = s_dl[r] != s;
            if (fresh) s_dl[n_dl++] = s;
        }
        s_n_win = n;
        s_n_dl = n_dl;
        s_err = err;
        s_abort = INT_MAX;
    }
    __syncthreads();
    const int n_win = s_n_win, n_dl = s_n_dl;
    if (tid < n_win) o.win[(size_t)q * kLwWin + tid] = s_win[tid];

    if (bow) {  // :833-840; a bad member aborts like any other
        if (a.q.conn_off && n_win) {
            const int o1 = a.q.conn_off[q + 1];
            for (int c = max(a.q.conn_off[q], 0) + tid; c < o1; c += kLwThreads) {
                const int s = a.q.conn_slot[c];
                if (!in_range(s, t.K)) continue;
                for (int w = 0; w < n_win; ++w)
                    if (s_win[w] == s) {
                        atomicMin(&s_abort, w);
                        break;
                    }
            }
        }
        __syncthreads();
        if (tid == 0) {
            o.n_win[q] = n_win;
            o.abort_at[q] = s_abort == INT_MAX ? -1 : s_abort;
            o.n_pts[q] = 0;
            o.err[q] = s_err;
        }
        return;
    }

    // ---- the point cloud: the walk over the rows of dl[] (at most kLwWin * cap positions, which fits:
    // the host checks it)
    unsigned* first = t.first + (size_t)q * t.v.n;
    const auto every = [](int) { return true; };
    first_mark<kLwThreads>((unsigned)n_dl * (unsigned)t.v.cap, first, row_walk(s_dl, t.v, every), true);
    const bool owners = kind == PLVI_LOOP_WIN_PROJ && o.pts_kf;
    const auto write = [&](int at, int id, unsigned e) {
        if (at >= o.pt_cap) return;
        o.pts[(size_t)q * o.pt_cap + at] = id;
        if (owners) o.pts_kf[(size_t)q * o.pt_cap + at] = s_dl[e / (unsigned)t.v.cap];
    };
    const int n_pts = first_compact<kLwThreads, 8>(s_dl, n_dl, t.v, first, every, s_wave, write);
    if (tid == 0) {
        o.n_win[q] = n_win;
        o.abort_at[q] = -1;
        o.n_pts[q] = n_pts;
        o.err[q] = s_err | (n_pts > o.pt_cap ? PLVI_LOOP_ERR_PTS : 0);
    }
}

// the rows of pts[q][0, min(n_pts, pt_cap)) from the pool, in f21's layouts
__global__ __launch_bounds__(kLwGather) void loop_gather_kernel(plvi_loop_outputs o, const float* pos,
                                                                 const float* normal, const float* dist,
                                                                 const uint8_t* desc) {
    const int tid = threadIdx.x, q = blockIdx.y, base = blockIdx.x * kLwGather;
    const int n = min(o.n_pts[q], o.pt_cap) - base;  // points of this chunk
    if (n <= 0) return;
    const size_t row0 = (size_t)q * o.pt_cap + base;
    const PoolGather g{pos, nullptr, normal, dist, desc, o.pos, nullptr, o.normal, o.dist, o.desc};
    if (tid < n) g.rows(row0 + tid, (size_t)o.pts[row0 + tid]);
    g.descriptors<kLwGather>(min(n, kLwGather), tid, [&](int e, size_t* at) { return o.pts[*at = row0 + e]; });
}

__global__ __launch_bounds__(kLwThreads) void loop_bow_merge_kernel(LwMergeArgs a) {
    __shared__ int s_slot[kLwBow], s_nt[kLwBow];
    __shared__ int s_num;
    const int tid = threadIdx.x, q = blockIdx.x;
    const LwTables& t = a.t;
    const int n1 = clampi(a.n1[q], 0, a.cap1), n_win = clampi(a.n_win[q], 0, kLwBow), ab = a.abort_at[q];
    const int J = ab >= 0 ? min(ab, n_win) : n_win;  // the break of :835-840 stands before member ab's matches

    if (tid < kLwBow) {  // a bad member was not searched (:820): its vector is empty
        const int s = tid < J ? a.win[(size_t)q * kLwWin + tid] : -1;
        const bool ok = in_range(s, t.K) && !t.kf_bad[s];
        s_slot[tid] = ok ? s : -1;
        s_nt[tid] = ok ? t.v.len(s) : 0;
    }
    if (tid == 0) s_num = 0;
    __syncthreads();
    unsigned* first = t.first + (size_t)q * t.v.n;
    const int* m12 = a.m12 + (size_t)q * kLwBow * a.cap1;
    // the MapPoint of member j's match for k, -1 where :846 skips
    auto point = [&](int j, int k) {
        const int s = s_slot[j];
        return s < 0 ? -1 : t.v.at(s, m12[(size_t)j * a.cap1 + k], s_nt[j]);
    };
    const auto at_position = [&](unsigned e) {
        const int j = (int)(e / (unsigned)n1);
        return point(j, (int)(e - (unsigned)j * (unsigned)n1));
    };
    first_mark<kLwThreads>((unsigned)J * (unsigned)n1, first, at_position, true);
    int won = 0;
    for (int k = tid; k < n1; k += kLwThreads) {
        int cell = -1, owner = -1;
        for (int j = 0; j < J; ++j) {
            const int p = point(j, k);
            if (p >= 0 && first[p] == (unsigned)j * (unsigned)n1 + (unsigned)k) {
                ++won;
                cell = p;  // a later member overwrites the cell with its own new point
                owner = s_slot[j];
            }
        }
        a.matched_mp[(size_t)q * a.cap1 + k] = cell;
        a.matched_kf[(size_t)q * a.cap1 + k] = owner;
    }
    block_add(won, &s_num, tid);
    __syncthreads();
    if (tid == 0) a.num[q] = s_num;
}

}  // namespace plvi

using namespace plvi;

static int lw_tables(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp, LwTables* t) {
    if (n_queries < 0 || !kf || !mp) return PLVI_E_BADARG;
    if (kf->kf_cap < 1 || kf->kp_cap < 0 || kf->cand_stride < 0 || mp->n < 0) return PLVI_E_BADARG;
    memset(t, 0, sizeof *t);
    if (n_queries == 0) return PLVI_OK;
    if (!kf->bad || (kf->kp_cap > 0 && (!kf->mp || !kf->nmp)) || (mp->n > 0 && !mp->bad)) return PLVI_E_BADARG;
    if (n_queries > 65535) return PLVI_E_CAPACITY;
    const long long rows = kf->kf_cap > kLwWin ? kf->kf_cap : kLwWin;
    if (rows * kf->kp_cap > PLVI_LOCAL_MAP_MAX_ENTRIES) return PLVI_E_CAPACITY;
    t->K = kf->kf_cap;
    t->cand_stride = kf->cand_stride;
    t->kf_bad = kf->bad;
    t->v = KfTable{kf->mp, kf->nmp, kf->kp_cap, mp->n, mp->bad};
    t->cand = kf->cand;
    t->n_cand = kf->n_cand;
    return PLVI_OK;
}

static int lw_validate(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                       const plvi_loop_queries* qs, const plvi_loop_outputs* out, LwArgs* a) {
    if (!qs || !out) return PLVI_E_BADARG;
    if (int rc = lw_tables(n_queries, kf, mp, &a->t)) return rc;
    if (out->pt_cap < 0) return PLVI_E_BADARG;
    if (n_queries == 0) return PLVI_OK;
    if ((kf->cand_stride > 0 && !kf->cand) || !kf->n_cand) return PLVI_E_BADARG;
    if (!qs->kind || !qs->kf_slot || (qs->conn_off == nullptr) != (qs->conn_slot == nullptr)) return PLVI_E_BADARG;
    if (!out->win || !out->n_win || !out->abort_at || !out->n_pts || !out->err || (out->pt_cap > 0 && !out->pts))
        return PLVI_E_BADARG;
    // a gather needs its source row
    if ((out->pos && !mp->pos) || (out->normal && !mp->normal) || (out->dist && !mp->dist) ||
        (out->desc && !mp->desc))
        return PLVI_E_BADARG;
    a->q = *qs;
    a->o = *out;
    return PLVI_OK;
}

extern "C" size_t plvi_loop_window_scratch_bytes(int n_queries, int mp_n) {
    if (n_queries < 0 || mp_n < 0) return 0;
    return 256 + (size_t)n_queries * lw_per_query(mp_n);
}

extern "C" int plvi_loop_window_batch(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                                      const plvi_loop_queries* queries, const plvi_loop_outputs* out, void* d_scratch,
                                      size_t scratch_bytes, void* stream) {
    LwArgs a;
    if (int rc = lw_validate(n_queries, kf, mp, queries, out, &a)) return rc;
    if (n_queries == 0) return PLVI_OK;
    if (!d_scratch || scratch_bytes < plvi_loop_window_scratch_bytes(n_queries, mp->n)) return PLVI_E_BADARG;
    a.t.first = reinterpret_cast<unsigned*>(static_cast<uint8_t*>(d_scratch) + 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(loop_window_kernel, dim3(n_queries), dim3(kLwThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    if (out->pt_cap > 0 && (out->pos || out->normal || out->dist || out->desc)) {
        hipLaunchKernelGGL(loop_gather_kernel, dim3((out->pt_cap + kLwGather - 1) / kLwGather, n_queries),
                           dim3(kLwGather), 0, st, a.o, mp->pos, mp->normal, mp->dist, mp->desc);
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

static int lw_merge_validate(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                             const int* win, const int* n_win, const int* abort_at, const int* matches12,
                             const int* n1, int cap1, int* matched_mp, int* matched_kf, int* num, LwMergeArgs* a) {
    if (int rc = lw_tables(n_queries, kf, mp, &a->t)) return rc;
    if (cap1 < 0) return PLVI_E_BADARG;
    if (n_queries == 0) return PLVI_OK;
    if (!win || !n_win || !abort_at || !n1 || !num) return PLVI_E_BADARG;
    if (cap1 > 0 && (!matches12 || !matched_mp || !matched_kf)) return PLVI_E_BADARG;
    if ((long long)kLwBow * cap1 > PLVI_LOCAL_MAP_MAX_ENTRIES) return PLVI_E_CAPACITY;
    a->cap1 = cap1;
    a->win = win;
    a->n_win = n_win;
    a->abort_at = abort_at;
    a->m12 = matches12;
    a->n1 = n1;
    a->matched_mp = matched_mp;
    a->matched_kf = matched_kf;
    a->num = num;
    return PLVI_OK;
}

extern "C" int plvi_loop_bow_merge_batch(int n_queries, const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                                         const int* d_win, const int* d_n_win, const int* d_abort_at,
                                         const int* d_matches12, const int* d_n1, int cap1, int* d_matched_mp,
                                         int* d_matched_kf, int* d_num, void* d_scratch, size_t scratch_bytes,
                                         void* stream) {
    LwMergeArgs a;
    if (int rc = lw_merge_validate(n_queries, kf, mp, d_win, d_n_win, d_abort_at, d_matches12, d_n1, cap1,
                                   d_matched_mp, d_matched_kf, d_num, &a))
        return rc;
    if (n_queries == 0) return PLVI_OK;
    if (!d_scratch || scratch_bytes < plvi_loop_window_scratch_bytes(n_queries, mp->n)) return PLVI_E_BADARG;
    a.t.first = reinterpret_cast<unsigned*>(static_cast<uint8_t*>(d_scratch) + 256);
    hipLaunchKernelGGL(loop_bow_merge_kernel, dim3(n_queries), dim3(kLwThreads), 0, (hipStream_t)stream, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

// what both host forms read of the tables: bad, the keyframe tables, and with `rows` the graph's rows
static void lw_stage_tables(HostStage& hs, plvi_cull_keyframes& dk, plvi_local_map_pool& dp, bool rows) {
    const size_t K = (size_t)dk.kf_cap;
    const plvi_cull_keyframes src = dk;
    const plvi_local_map_pool psrc = dp;
    dk = plvi_cull_keyframes{};
    dk.kf_cap = src.kf_cap;
    dk.kp_cap = src.kp_cap;
    dk.cand_stride = src.cand_stride;
    dk.bad = src.bad;
    dk.mp = src.mp;
    dk.nmp = src.nmp;
    if (rows) dk.cand = src.cand, dk.n_cand = src.n_cand;
    dp = plvi_local_map_pool{};
    dp.n = psrc.n;
    dp.bad = psrc.bad;
    hs.field(dk.bad, HostStage::In, K);
    hs.field(dk.mp, HostStage::In, K, src.kp_cap);
    hs.field(dk.nmp, HostStage::In, K);
    hs.field(dk.cand, HostStage::In, K, src.cand_stride);
    hs.field(dk.n_cand, HostStage::In, K);
    hs.field(dp.bad, HostStage::In, (size_t)psrc.n);
}

// One query from host memory.  Every pointer of the structs is a host pointer here.
extern "C" int plvi_loop_window(const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp,
                                const plvi_loop_queries* queries, const plvi_loop_outputs* out) {
    LwArgs chk;
    if (int rc = lw_validate(1, kf, mp, queries, out, &chk)) return rc;
    // copies of the caller's structs: commit() turns their host pointers into device pointers
    plvi_cull_keyframes dk = *kf;
    plvi_local_map_pool dp = *mp;
    plvi_loop_queries dq = *queries;
    plvi_loop_outputs dout = *out;
    const size_t n = (size_t)mp->n, cap = (size_t)out->pt_cap;
    const size_t n_conn = queries->conn_off && queries->conn_off[1] > 0 ? (size_t)queries->conn_off[1] : 0;
    HostStage hs;
    const HostStage::Dir In = HostStage::In, Out = HostStage::Out, InOut = HostStage::InOut;
    lw_stage_tables(hs, dk, dp, true);
    // only the rows a gather reads travel
    if (out->pos) dp.pos = mp->pos;
    if (out->normal) dp.normal = mp->normal;
    if (out->dist) dp.dist = mp->dist;
    if (out->desc) dp.desc = mp->desc;
    hs.field(dp.pos, In, n, 3);
    hs.field(dp.normal, In, n, 3);
    hs.field(dp.dist, In, n, 2);
    hs.field(dp.desc, In, n, 32);
    hs.field(dq.kind, In, 1);
    hs.field(dq.kf_slot, In, 1);
    hs.field(dq.cur_slot, In, 1);
    hs.field(dq.conn_off, In, 2);
    hs.field(dq.conn_slot, In, n_conn);
    for (int** p : {&dout.n_win, &dout.abort_at, &dout.n_pts, &dout.err}) hs.field(*p, Out, 1);
    // in/out: cells past a list's end keep the caller's fill
    hs.field(dout.win, InOut, kLwWin);
    hs.field(dout.pts, InOut, cap);
    hs.field(dout.pts_kf, InOut, cap);
    hs.field(dout.pos, InOut, cap, 3);
    hs.field(dout.normal, InOut, cap, 3);
    hs.field(dout.dist, InOut, cap, 2);
    hs.field(dout.desc, InOut, cap, 32);
    const size_t sb = plvi_loop_window_scratch_bytes(1, mp->n);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_loop_window_batch(1, &dk, &dp, &dq, &dout, hs.dev(scr), sb, nullptr)) return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err & ~PLVI_LOOP_ERR_UNDEFINED ? PLVI_E_CAPACITY : PLVI_OK;
}

// One merge from host memory: per-query arrays of one entry, matches12 [PLVI_LOOP_BOW_WIN][cap1].
extern "C" int plvi_loop_bow_merge(const plvi_cull_keyframes* kf, const plvi_local_map_pool* mp, const int* win,
                                   const int* n_win, const int* abort_at, const int* matches12, const int* n1,
                                   int cap1, int* matched_mp, int* matched_kf, int* num) {
    LwMergeArgs chk;
    if (int rc = lw_merge_validate(1, kf, mp, win, n_win, abort_at, matches12, n1, cap1, matched_mp, matched_kf, num,
                                   &chk))
        return rc;
    plvi_cull_keyframes dk = *kf;
    plvi_local_map_pool dp = *mp;
    HostStage hs;
    lw_stage_tables(hs, dk, dp, false);
    const auto d_win = hs.in(win, kLwWin);
    const auto d_n_win = hs.in(n_win, 1);
    const auto d_abort = hs.in(abort_at, 1);
    const auto d_m12 = hs.in(matches12, kLwBow, (size_t)cap1);
    const auto d_n1 = hs.in(n1, 1);
    const auto d_mmp = hs.inout(matched_mp, (size_t)cap1);
    const auto d_mkf = hs.inout(matched_kf, (size_t)cap1);
    const auto d_num = hs.out(num, 1);
    const size_t sb = plvi_loop_window_scratch_bytes(1, mp->n);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_loop_bow_merge_batch(1, &dk, &dp, hs.dev(d_win), hs.dev(d_n_win), hs.dev(d_abort),
                                           hs.dev(d_m12), hs.dev(d_n1), cap1, hs.dev(d_mmp), hs.dev(d_mkf),
                                           hs.dev(d_num), hs.dev(scr), sb, nullptr))
        return rc;
    return hs.fetch();
}
