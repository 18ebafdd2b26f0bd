// essential_graph.hip — the integer work of LoopClosing::CorrectLoop[WithLines] (src/LoopClosing.cc:1212-1473,
// :1475-1712) and Optimizer::OptimizeEssentialGraph[4DoF] (src/Optimizer.cc:6952-7305, :14411-) around the Sim3
// arithmetic and the solver, over the resident keyframe tables, pools and covisibility rows.  Integers only.
//
// Every std::set<KeyFrame*> / std::map<KeyFrame*, ...> iteration is "ascending rank", the rank of a slot being
// its first position in `order` (n_order + slot for a slot that order does not name):
//   eg_fill / eg_rank      rank[] by slot: a fill of kf_cap cells and a grid-wide atomicMin.
//   eg_correct_kernel      one workgroup.  The window (cur's ordered row, then cur) is sorted by rank in LDS, its
//                          repeats dropped; the correction owners are the first-occurrence walk of first_walk.h
//                          over the sorted members with the stamp test as the predicate; emit stamps.
//   eg_loopconn_kernel     one workgroup.  The last window position of every slot (wpos, atomicMax), the
//                          loop-connection edges as an ordered compaction over (key, cell), and a pass flag per
//                          cell of lc_kf: "inserted?" is then a scan of the rows of whichever endpoint is a
//                          window member, so no global set is needed.
//   eg_edges_kernel        a wave per entry of order, run twice: <false> counts the entry's edges and its
//                          vertex, <true> writes them at the offsets eg_scan_kernel made of the counts (one
//                          workgroup, tile by tile with a carry).  Within a wave the loop row and the covisible
//                          prefix are taken 64 entries at a time, a ballot keeping their order.
//   eg_refs_kernel         a thread per feature.
//   eg_snapshot / eg_diff  LoopConnections (:1406-1424): per window position the slot's ordered row is copied to
//                          scratch, then plvi_covis_update_batch runs for that one query; after the last position
//                          a workgroup per position takes the keys of the slot's weight map, drops the snapshot
//                          and the window members, and places the rest by rank.
#include <climits>
#include <cstring>

#include "first_walk.h"
#include "host_stage.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kEgThreads = 1024, kEgWaves = kEgThreads / kWave;
constexpr int kEgWin = PLVI_EG_MAX_WIN;
constexpr int kEgMinFeat = PLVI_EG_MIN_FEAT;
constexpr int kEgRankNone = INT_MAX;
constexpr int kEgEdgeThreads = 256, kEgEdgeWaves = kEgEdgeThreads / kWave;  // entries of order per workgroup
constexpr unsigned kEgNoKey = 0xffffffffu;

struct EgGraph {  // what the kernels read of plvi_cull_keyframes and plvi_eg_keyframes
    int K, n_order, cand_stride, map_stride;
    const uint8_t *bad, *init_kf, *imu;
    const int *order, *map_id, *parent, *child_off, *child, *loop_off, *loop, *prev_kf, *next_kf;
    const unsigned* kf_id;
    const int *cand, *n_cand, *cand_w, *map_kf, *map_w, *map_n;
    int* rank;  // [K], scratch

    __device__ __forceinline__ unsigned rank_of(int s) const {  // s in range
        const int r = rank[s];
        return r == kEgRankNone ? (unsigned)n_order + (unsigned)s : (unsigned)r;
    }
    __device__ __forceinline__ int map_of(int s) const { return map_id ? map_id[s] : 0; }
    // a member of vpKFs that is not bad
    __device__ __forceinline__ bool vertex(int s, int M) const {
        return in_range(s, K) && rank[s] != kEgRankNone && !bad[s] && map_of(s) == M;
    }
    // GetWeight(j) of slot i (in range): the map entry or 0
    __device__ __forceinline__ int weight(int i, int j) const {
        const int n = clampi(map_n[i], 0, map_stride);
        for (int e = 0; e < n; ++e)
            if (map_kf[(size_t)i * map_stride + e] == j) return map_w[(size_t)i * map_stride + e];
        return 0;
    }
};

struct EgCorrectArgs {
    EgGraph g;
    int cur;
    KfTable vp, vl;  // vl.cap == 0 without lines
    unsigned *by_p, *by_l;
    int *ref_p, *ref_l;
    unsigned* first;  // [max(mp_n, ml_n)], scratch
    plvi_loop_correct_outputs o;
};

struct EgArgs {
    EgGraph g;
    int cur, loop, mode, win_cap, lc_cap;
    const int *win, *n_win, *lc_kf, *n_lc;
    int *wpos, *cnt_e, *cnt_v;  // [K], [n_order], [n_order], scratch
    uint8_t* pass;              // [win_cap][lc_cap], scratch
    plvi_eg_outputs o;
};

__global__ void eg_fill_kernel(int* rank, int* wpos, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    rank[i] = kEgRankNone;
    if (wpos) wpos[i] = -1;
}

__global__ void eg_rank_kernel(int* rank, int K, const int* order, int n_order) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_order) return;
    const int s = order[k];
    if (in_range(s, K)) atomicMin(rank + s, k);
}

// s_slot[0, n) -> s_sorted: the distinct slots in range, ascending rank; returns their number.  Every thread
// of the workgroup calls it; s_slot must be complete (a barrier of the caller's); ends with a barrier.
__device__ int eg_sort_window(const EgGraph& g, const int* s_slot, int n, unsigned* s_key, int* s_sorted, int* s_cnt) {
    const int tid = threadIdx.x;
    if (tid == 0) *s_cnt = 0;
    for (int i = tid; i < n; i += kEgThreads) {
        const int s = s_slot[i];
        bool first = in_range(s, g.K);
        for (int j = 0; j < i && first; ++j) first = s_slot[j] != s;
        s_key[i] = first ? g.rank_of(s) : kEgNoKey;
    }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += kEgThreads) {
        const unsigned k = s_key[i];
        if (k == kEgNoKey) continue;
        int p = 0;
        for (int j = 0; j < n; ++j) p += s_key[j] < k;  // the keys kept are distinct
        s_sorted[p] = s_slot[i];
        ++mine;
    }
    block_add(mine, s_cnt, tid);
    __syncthreads();
    return *s_cnt;
}

// the walk of one pool over the sorted members: lists and stamps; returns the full length
__device__ int eg_walk(const int* s_sorted, int n_sorted, const KfTable& v, unsigned* by, int* ref, unsigned stamp,
                       unsigned* first, int* out, int* out_kf, int cap, int* s_wave) {
    if (v.cap <= 0 || v.n <= 0) return 0;
    const auto fresh = [=](int id) { return !by || by[id] != stamp; };
    first_mark<kEgThreads>((unsigned)n_sorted * (unsigned)v.cap, first, row_walk(s_sorted, v, fresh), true);
    // A later position of a listed id may read its stamp while the owner writes it; that position does not
    // hold the id's minimum, so either value leaves it out.
    const auto emit = [&](int at, int id, unsigned e) {
        const int owner = s_sorted[e / (unsigned)v.cap];
        if (at < cap) {
            out[at] = id;
            out_kf[at] = owner;
        }
        if (by) {
            by[id] = stamp;
            ref[id] = owner;
        }
    };
    return first_compact<kEgThreads, 8>(s_sorted, n_sorted, v, first, fresh, s_wave, emit);
}

__global__ __launch_bounds__(kEgThreads) void eg_correct_kernel(EgCorrectArgs a) {
    __shared__ int s_win[kEgWin], s_sorted[kEgWin];
    __shared__ unsigned s_key[kEgWin];
    __shared__ int s_wave[kEgWaves];
    __shared__ int s_cnt;
    const EgGraph& g = a.g;
    const plvi_loop_correct_outputs& o = a.o;
    const int tid = threadIdx.x, cur = a.cur;
    const int n_row = clampi(g.n_cand[cur], 0, g.cand_stride), n_win = n_row + 1;
    for (int i = tid; i < n_win; i += kEgThreads) {
        const int s = i < n_row ? g.cand[(size_t)cur * g.cand_stride + i] : cur;
        s_win[i] = s;
        if (i < o.win_cap) o.win[i] = s;
    }
    __syncthreads();
    const int n_sorted = eg_sort_window(g, s_win, n_win, s_key, s_sorted, &s_cnt);
    for (int i = tid; i < min(n_sorted, o.win_cap); i += kEgThreads) o.win_sorted[i] = s_sorted[i];
    const unsigned stamp = g.kf_id[cur];
    const int n_pts = eg_walk(s_sorted, n_sorted, a.vp, a.by_p, a.ref_p, stamp, a.first, o.pts, o.pts_kf, o.pt_cap, s_wave);
    __syncthreads();  // first[] is reused
    const int n_lns = eg_walk(s_sorted, n_sorted, a.vl, a.by_l, a.ref_l, stamp, a.first, o.lns, o.lns_kf, o.ln_cap, s_wave);
    if (tid == 0) {
        *o.n_win = n_win;
        *o.n_sorted = n_sorted;
        *o.n_pts = n_pts;
        *o.n_lns = n_lns;
        *o.err = (n_win > o.win_cap ? PLVI_EG_ERR_WIN : 0) | (n_pts > o.pt_cap ? PLVI_EG_ERR_PTS : 0) |
                 (n_lns > o.ln_cap ? PLVI_EG_ERR_LNS : 0);
    }
}

// cur_slot / loop_slot outside the table: the counts and err of either call
__global__ void eg_query_error_kernel(int* c0, int* c1, int* c2, int* c3, int* five, int* err) {
    if (threadIdx.x) return;
    if (c0) *c0 = 0;
    if (c1) *c1 = 0;
    if (c2) *c2 = 0;
    if (c3) *c3 = 0;
    for (int k = 0; five && k < 5; ++k) five[k] = 0;
    *err = PLVI_EG_ERR_QUERY;
}

__global__ __launch_bounds__(kEgThreads) void eg_loopconn_kernel(EgArgs a) {
    __shared__ int s_win[kEgWin], s_sorted[kEgWin];
    __shared__ unsigned s_key[kEgWin];
    __shared__ int s_wave[kEgWaves];
    __shared__ int s_cnt;
    const EgGraph& g = a.g;
    const plvi_eg_outputs& o = a.o;
    const int tid = threadIdx.x;
    const int n_win = clampi(*a.n_win, 0, a.win_cap), M = g.map_of(a.cur);
    for (int p = tid; p < n_win; p += kEgThreads) {
        const int s = a.win[p];
        s_win[p] = s;
        if (in_range(s, g.K)) atomicMax(a.wpos + s, p);
    }
    if (tid == 0) {
        for (int k = 1; k < 5; ++k) o.n_edges[k] = 0;  // the count pass adds to these
        *o.err = 0;
    }
    __syncthreads();
    const int n_sorted = eg_sort_window(g, s_win, n_win, s_key, s_sorted, &s_cnt);
    const unsigned total = (unsigned)n_sorted * (unsigned)a.lc_cap;
    int n_kept = 0;
    bool orphan = false;
    for (unsigned base = 0; base < total; base += kEgThreads) {
        const unsigned pos = base + tid;
        int i = -1, j = -1;
        bool ok = false;
        if (pos < total) {
            const unsigned k = pos / (unsigned)a.lc_cap, e = pos - k * (unsigned)a.lc_cap;
            i = s_sorted[k];
            const int p = a.wpos[i];  // the row of the key's last position
            if ((int)e < clampi(a.n_lc[p], 0, a.lc_cap)) {
                const size_t cell = (size_t)p * a.lc_cap + e;
                j = a.lc_kf[cell];
                ok = in_range(j, g.K) && ((i == a.cur && j == a.loop) || g.weight(i, j) >= kEgMinFeat);
                a.pass[cell] = ok;
            }
        }
        int tot;
        const int at = n_kept + block_scan<kEgWaves>(ok, s_wave, tid, &tot);
        if (ok) {
            if (at < o.edge_cap) {
                o.edge_a[at] = i;
                o.edge_b[at] = j;
                o.edge_kind[at] = PLVI_EG_EDGE_LOOPCONN;
            }
            orphan |= !g.vertex(i, M) || !g.vertex(j, M);
        }
        n_kept += tot;
    }
    if (orphan) atomicOr(o.err, PLVI_EG_ERR_NO_VERTEX);
    if (tid == 0) o.n_edges[PLVI_EG_EDGE_LOOPCONN] = n_kept;
}

// is the unordered pair (i, n) a loop-connection edge?  Both in range.
__device__ bool eg_inserted(const EgArgs& a, int i, int n) {
    for (int t = 0; t < 2; ++t) {
        const int x = t ? n : i, y = t ? i : n, p = a.wpos[x];
        if (p < 0) continue;
        const int m = clampi(a.n_lc[p], 0, a.lc_cap);
        for (int e = 0; e < m; ++e)
            if (a.lc_kf[(size_t)p * a.lc_cap + e] == y && a.pass[(size_t)p * a.lc_cap + e]) return true;
    }
    return false;
}

__device__ __forceinline__ bool eg_in_row(const int* off, const int* row, int s, int v) {
    if (!off) return false;
    const int o1 = off[s + 1];
    for (int c = max(off[s], 0); c < o1; ++c)
        if (row[c] == v) return true;
    return false;
}

// The vertex and the normal edges of entry k of order, a wave each.  kWrite = false leaves the counts in cnt_v /
// cnt_e and adds to n_edges; kWrite = true writes at the scanned offsets.
template <bool kWrite>
__global__ __launch_bounds__(kEgEdgeThreads) void eg_edges_kernel(EgArgs a) {
    const EgGraph& g = a.g;
    const plvi_eg_outputs& o = a.o;
    const int lane = threadIdx.x & (kWave - 1);
    const int k = blockIdx.x * kEgEdgeWaves + threadIdx.x / kWave;
    if (k >= g.n_order) return;
    const int i = g.order[k], M = g.map_of(a.cur);
    if (!in_range(i, g.K) || g.rank[i] != k || g.map_of(i) != M) {  // not a member of vpKFs
        if (!kWrite && lane == 0) a.cnt_e[k] = a.cnt_v[k] = 0;
        return;
    }
    const bool is_vertex = !g.bad[i], four = a.mode == PLVI_EG_4DOF;
    if (kWrite && is_vertex && lane == 0) {
        const int at = a.cnt_v[k];
        if (at < o.vert_cap) {
            o.vert[at] = i;
            const bool fixed = four ? i == a.loop : g.init_kf && g.init_kf[i];
            o.vert_flags[at] = (int)fixed | (a.wpos[i] >= 0 ? 2 : 0);
        }
    }
    int at = kWrite ? o.n_edges[PLVI_EG_EDGE_LOOPCONN] + a.cnt_e[k] : 0;  // where this entry's next edge goes
    int n_kind[5] = {0, 0, 0, 0, 0};
    bool orphan = false;
    // ok per lane, in lane order
    const auto put = [&](bool ok, int b, int kind) {
        const unsigned long long m = __ballot(ok);
        if (kWrite && ok) {
            const int p = at + __popcll(m & ((1ull << lane) - 1));
            if (p < o.edge_cap) {
                o.edge_a[p] = i;
                o.edge_b[p] = b;
                o.edge_kind[p] = kind;
            }
            orphan |= !is_vertex || !g.vertex(b, M);
        }
        at += __popcll(m);
        n_kind[kind] += __popcll(m);
    };
    const unsigned id_i = g.kf_id[i];
    const int par = !four && g.parent ? g.parent[i] : -1;  // :14545: NULL in 4DOF
    const int prev = g.prev_kf[i], next = g.next_kf[i];
    const auto loops = [&] {
        if (!g.loop_off) return;
        const int o0 = max(g.loop_off[i], 0), o1 = g.loop_off[i + 1];
        for (int c0 = o0; c0 < o1; c0 += kWave) {
            const int c = c0 + lane, l = c < o1 ? g.loop[c] : -1;
            put(in_range(l, g.K) && g.kf_id[l] < id_i, l, PLVI_EG_EDGE_LOOP);
        }
    };
    const auto covis = [&] {
        // GetCovisiblesByWeight(minFeat): upper_bound on the descending weights
        const int* w = g.cand_w + (size_t)i * g.cand_stride;
        int lo = 0, hi = clampi(g.n_cand[i], 0, g.cand_stride);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (w[mid] >= kEgMinFeat)
                lo = mid + 1;
            else
                hi = mid;
        }
        for (int c0 = 0; c0 < lo; c0 += kWave) {
            const int c = c0 + lane, n = c < lo ? g.cand[(size_t)i * g.cand_stride + c] : -1;
            bool ok = in_range(n, g.K) && n != par && !(four && (n == prev || n == next));
            ok = ok && !eg_in_row(g.child_off, g.child, i, n) && !eg_in_row(g.loop_off, g.loop, i, n);
            ok = ok && !g.bad[n] && g.kf_id[n] < id_i && !eg_inserted(a, i, n);
            put(ok, n, PLVI_EG_EDGE_COVIS);
        }
    };
    if (four) {
        put(lane == 0 && in_range(prev, g.K), prev, PLVI_EG_EDGE_INERTIAL);
        loops();
        covis();
    } else {
        put(lane == 0 && in_range(par, g.K), par, PLVI_EG_EDGE_TREE);
        loops();
        covis();
        put(lane == 0 && g.imu && g.imu[i] && in_range(prev, g.K), prev, PLVI_EG_EDGE_INERTIAL);
    }
    if (kWrite) {
        if (orphan) atomicOr(o.err, PLVI_EG_ERR_NO_VERTEX);
    } else if (lane == 0) {
        int n = 0;
        for (int kind = 1; kind < 5; ++kind) {
            n += n_kind[kind];
            if (n_kind[kind]) atomicAdd(o.n_edges + kind, n_kind[kind]);
        }
        a.cnt_e[k] = n;
        a.cnt_v[k] = is_vertex;
    }
}

// cnt_e / cnt_v -> exclusive offsets, in place; the totals against the capacities
__global__ __launch_bounds__(kEgThreads) void eg_scan_kernel(EgArgs a) {
    __shared__ int s_wave[kEgWaves];
    const int tid = threadIdx.x, n = a.g.n_order;
    int sum_e = 0, sum_v = 0;
    for (int k0 = 0; k0 < n; k0 += kEgThreads) {
        const int k = k0 + tid;
        const int e = k < n ? a.cnt_e[k] : 0, v = k < n ? a.cnt_v[k] : 0;
        int tot_e, tot_v;
        const int off_e = sum_e + block_scan<kEgWaves>(e, s_wave, tid, &tot_e);
        const int off_v = sum_v + block_scan<kEgWaves>(v, s_wave, tid, &tot_v);
        if (k < n) {
            a.cnt_e[k] = off_e;
            a.cnt_v[k] = off_v;
        }
        sum_e += tot_e;
        sum_v += tot_v;
    }
    if (tid == 0) {
        *a.o.n_vert = sum_v;
        const int err = (sum_v > a.o.vert_cap ? PLVI_EG_ERR_VERT : 0) |
                        (a.o.n_edges[PLVI_EG_EDGE_LOOPCONN] + sum_e > a.o.edge_cap ? PLVI_EG_ERR_EDGE : 0);
        if (err) atomicOr(a.o.err, err);
    }
}

// :7235-7301: the keyframe a feature is re-mapped through; blockIdx.y = the pool
struct EgRefs {
    int n[2];
    const uint8_t* bad[2];
    const int *ref_kf[2], *map_id[2], *corr_ref[2];
    const unsigned* corr_by[2];
    int* out[2];
};

__global__ void eg_refs_kernel(EgGraph g, int cur, int mode, EgRefs r) {
    const int p = blockIdx.y, id = blockIdx.x * blockDim.x + threadIdx.x;
    if (!r.out[p] || id >= r.n[p]) return;
    int ref = -1;
    if (!r.bad[p][id] && (r.map_id[p] ? r.map_id[p][id] : 0) == g.map_of(cur))
        ref = mode == PLVI_EG_7DOF && r.corr_by[p] && r.corr_by[p][id] == g.kf_id[cur] ? r.corr_ref[p][id]
                                                                                        : r.ref_kf[p][id];
    r.out[p][id] = ref;
}

// ---- LoopConnections (:1406-1424)
constexpr int kEgChunk = 512;  // window entries handed to eg_set_kernel by value
constexpr int kEgDiffThreads = 256;

struct EgChunk {
    int n, base;
    int v[kEgChunk];
};

struct EgLcArgs {
    int K, C, n_order, n_win, lc_cap;
    const int *map_kf, *map_n;   // the graph's weight-map rows
    const int *win, *snap, *snap_n, *rank;
    int *lc_kf, *n_lc, *err;
};

__global__ void eg_set_kernel(int* dst, int* err, EgChunk c) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c.n) dst[c.base + i] = c.v[i];
    if (i == 0 && c.base == 0) *err = 0;
}

// vpPreviousNeighbors of one window position: the slot's ordered row as it stands
__global__ void eg_snapshot_kernel(const int* ord_kf, const int* ord_n, int C, int slot, int* row, int* n) {
    const int m = clampi(ord_n[slot], 0, C);
    for (int e = threadIdx.x; e < m; e += blockDim.x) row[e] = ord_kf[(size_t)slot * C + e];
    if (threadIdx.x == 0) *n = m;
}

// lc[p] = the keys of the slot's weight map minus snapshot p minus every window member, ascending rank
__global__ __launch_bounds__(kEgDiffThreads) void eg_diff_kernel(EgLcArgs a) {
    __shared__ unsigned s_key[PLVI_COVIS_MAX_CONN];
    __shared__ int s_slot[PLVI_COVIS_MAX_CONN];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, p = blockIdx.x, s = a.win[p];
    if (!in_range(s, a.K)) {
        if (tid == 0) a.n_lc[p] = 0;
        return;
    }
    const int n = clampi(a.map_n[s], 0, a.C), m = clampi(a.snap_n[p], 0, a.C);
    const int* snap = a.snap + (size_t)p * a.C;
    if (tid == 0) s_cnt = 0;
    for (int e = tid; e < n; e += kEgDiffThreads) {
        const int k = a.map_kf[(size_t)s * a.C + e];
        bool keep = in_range(k, a.K);
        for (int j = 0; j < m && keep; ++j) keep = snap[j] != k;
        for (int w = 0; w < a.n_win && keep; ++w) keep = a.win[w] != k;
        s_slot[e] = k;
        unsigned key = kEgNoKey;
        if (keep) key = a.rank[k] == kEgRankNone ? (unsigned)a.n_order + (unsigned)k : (unsigned)a.rank[k];
        s_key[e] = key;
    }
    __syncthreads();
    int mine = 0;
    for (int e = tid; e < n; e += kEgDiffThreads) {
        const unsigned key = s_key[e];
        if (key == kEgNoKey) continue;
        int pos = 0;
        for (int j = 0; j < n; ++j) pos += s_key[j] < key;  // map keys are distinct
        if (pos < a.lc_cap) a.lc_kf[(size_t)p * a.lc_cap + pos] = s_slot[e];
        ++mine;
    }
    block_add(mine, &s_cnt, tid);
    __syncthreads();
    if (tid == 0) {
        a.n_lc[p] = s_cnt;
        if (s_cnt > a.lc_cap) atomicOr(a.err, PLVI_EG_ERR_LC);
    }
}

}  // namespace plvi

using namespace plvi;

static bool eg_csr_ok(const int* off, const int* row) { return (off == nullptr) == (row == nullptr); }

// the checks and the table part of both calls; `graph` = everything plvi_essential_graph reads
static int eg_tables(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg, const plvi_local_map_pool* mp,
                     const plvi_local_map_pool* ml, bool graph, EgGraph* g) {
    if (!kf || !eg || !mp) return PLVI_E_BADARG;
    if (kf->kf_cap < 1 || kf->kp_cap < 0 || kf->kl_cap < 0 || kf->cand_stride < 0 || eg->n_order < 0 ||
        eg->map_stride < 0 || mp->n < 0 || (ml && ml->n < 0))
        return PLVI_E_BADARG;
    if (!kf->bad || !kf->n_cand || (kf->cand_stride > 0 && !kf->cand) || !kf->kf_id || (eg->n_order > 0 && !eg->order) ||
        (mp->n > 0 && !mp->bad) || (ml && ml->n > 0 && !ml->bad))
        return PLVI_E_BADARG;
    if (!graph) {  // the walk reads the keyframe tables
        if ((kf->kp_cap > 0 && (!kf->mp || !kf->nmp)) || (kf->ml && ml && kf->kl_cap > 0 && !kf->nml))
            return PLVI_E_BADARG;
    } else {
        if (!kf->prev_kf || !kf->next_kf || (kf->cand_stride > 0 && !eg->cand_w) || !eg->map_n ||
            (eg->map_stride > 0 && (!eg->map_kf || !eg->map_w)) || !eg_csr_ok(eg->child_off, eg->child) ||
            !eg_csr_ok(eg->loop_off, eg->loop))
            return PLVI_E_BADARG;
    }
    const long long longest = kf->kp_cap > kf->kl_cap ? kf->kp_cap : kf->kl_cap;
    if (kf->cand_stride > kEgWin - 1 || kf->kf_cap > (1 << 24) || eg->n_order > (1 << 30) ||
        kEgWin * longest > PLVI_LOCAL_MAP_MAX_ENTRIES)
        return PLVI_E_CAPACITY;
    memset(g, 0, sizeof *g);
    g->K = kf->kf_cap;
    g->n_order = eg->n_order;
    g->cand_stride = kf->cand_stride;
    g->map_stride = eg->map_stride;
    g->bad = kf->bad;
    g->init_kf = kf->init_kf;
    g->imu = eg->imu;
    g->order = eg->order;
    g->map_id = eg->map_id;
    g->parent = eg->parent;
    g->child_off = eg->child_off;
    g->child = eg->child;
    g->loop_off = eg->loop_off;
    g->loop = eg->loop;
    g->prev_kf = kf->prev_kf;
    g->next_kf = kf->next_kf;
    g->kf_id = kf->kf_id;
    g->cand = kf->cand;
    g->n_cand = kf->n_cand;
    g->cand_w = eg->cand_w;
    g->map_kf = eg->map_kf;
    g->map_w = eg->map_w;
    g->map_n = eg->map_n;
    return PLVI_OK;
}

static bool eg_features_ok(const plvi_eg_features* f) { return !f || !f->corr_by || f->corr_ref; }

// rank[] of a call: the fill (with wpos where given) and the atomicMin over order
static int eg_rank(const EgGraph& g, int* wpos, hipStream_t st) {
    hipLaunchKernelGGL(eg_fill_kernel, dim3((g.K + 255) / 256), dim3(256), 0, st, g.rank, wpos, g.K);
    PLVI_CHECK(hipGetLastError());
    if (g.n_order > 0) {
        hipLaunchKernelGGL(eg_rank_kernel, dim3((g.n_order + 255) / 256), dim3(256), 0, st, g.rank, g.K, g.order,
                           g.n_order);
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

static size_t eg_max(size_t a, size_t b) { return a > b ? a : b; }

extern "C" size_t plvi_loop_correct_scratch_bytes(int kf_cap, int mp_n, int ml_n) {
    if (kf_cap < 0 || mp_n < 0 || ml_n < 0) return 0;
    return up256(4 * (size_t)kf_cap) + up256(4 * eg_max(mp_n, ml_n));
}

extern "C" size_t plvi_essential_graph_scratch_bytes(int kf_cap, int n_order, int win_cap, int lc_cap) {
    if (kf_cap < 0 || n_order < 0 || win_cap < 0 || lc_cap < 0) return 0;
    return 2 * up256(4 * (size_t)kf_cap) + 2 * up256(4 * (size_t)n_order) + up256((size_t)win_cap * lc_cap);
}

static int eg_correct_validate(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                               const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                               const plvi_eg_features* fmp, const plvi_eg_features* fml,
                               const plvi_loop_correct_outputs* out, EgCorrectArgs* a) {
    if (!out) return PLVI_E_BADARG;
    memset(a, 0, sizeof *a);
    if (int rc = eg_tables(kf, eg, mp, ml, false, &a->g)) return rc;
    if (out->win_cap < 0 || out->pt_cap < 0 || out->ln_cap < 0 || !eg_features_ok(fmp) || !eg_features_ok(fml))
        return PLVI_E_BADARG;
    if (!out->n_win || !out->n_sorted || !out->n_pts || !out->n_lns || !out->err ||
        (out->win_cap > 0 && (!out->win || !out->win_sorted)) || (out->pt_cap > 0 && (!out->pts || !out->pts_kf)))
        return PLVI_E_BADARG;
    const bool lines = kf->ml && ml;
    if (lines && out->ln_cap > 0 && (!out->lns || !out->lns_kf)) return PLVI_E_BADARG;
    a->vp = KfTable{kf->mp, kf->nmp, kf->kp_cap, mp->n, mp->bad};
    if (lines) a->vl = KfTable{kf->ml, kf->nml, kf->kl_cap, ml->n, ml->bad};
    if (fmp) a->by_p = fmp->corr_by, a->ref_p = fmp->corr_ref;
    if (fml && lines) a->by_l = fml->corr_by, a->ref_l = fml->corr_ref;
    a->o = *out;
    return PLVI_OK;
}

extern "C" int plvi_loop_correct_device(int cur_slot, const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                                        const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                        const plvi_eg_features* fmp, const plvi_eg_features* fml,
                                        const plvi_loop_correct_outputs* out, void* d_scratch, size_t scratch_bytes,
                                        void* stream) {
    EgCorrectArgs a;
    if (int rc = eg_correct_validate(kf, eg, mp, ml, fmp, fml, out, &a)) return rc;
    if (!d_scratch || scratch_bytes < plvi_loop_correct_scratch_bytes(kf->kf_cap, mp->n, ml ? ml->n : 0))
        return PLVI_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cur_slot < 0 || cur_slot >= kf->kf_cap) {
        hipLaunchKernelGGL(eg_query_error_kernel, dim3(1), dim3(64), 0, st, out->n_win, out->n_sorted, out->n_pts,
                           out->n_lns, (int*)nullptr, out->err);
        PLVI_CHECK(hipGetLastError());
        return PLVI_OK;
    }
    a.cur = cur_slot;
    a.g.rank = static_cast<int*>(d_scratch);
    a.first = reinterpret_cast<unsigned*>(static_cast<uint8_t*>(d_scratch) + up256(4 * (size_t)kf->kf_cap));
    if (int rc = eg_rank(a.g, nullptr, st)) return rc;
    hipLaunchKernelGGL(eg_correct_kernel, dim3(1), dim3(kEgThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

static int eg_graph_validate(int mode, const int* win, const int* n_win, int win_cap, const int* lc_kf,
                             const int* n_lc, int lc_cap, const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                             const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                             const plvi_eg_features* fmp, const plvi_eg_features* fml, const plvi_eg_outputs* out,
                             EgArgs* a) {
    if (!out || (mode != PLVI_EG_7DOF && mode != PLVI_EG_4DOF)) return PLVI_E_BADARG;
    memset(a, 0, sizeof *a);
    if (int rc = eg_tables(kf, eg, mp, ml, true, &a->g)) return rc;
    if (win_cap < 0 || lc_cap < 0 || out->vert_cap < 0 || out->edge_cap < 0 || !eg_features_ok(fmp) ||
        !eg_features_ok(fml))
        return PLVI_E_BADARG;
    if (!n_win || (win_cap > 0 && (!win || !n_lc)) || (win_cap > 0 && lc_cap > 0 && !lc_kf)) return PLVI_E_BADARG;
    if (!out->n_vert || !out->n_edges || !out->err || (out->vert_cap > 0 && (!out->vert || !out->vert_flags)) ||
        (out->edge_cap > 0 && (!out->edge_a || !out->edge_b || !out->edge_kind)))
        return PLVI_E_BADARG;
    if ((out->pt_ref && (!fmp || !fmp->ref_kf)) || (out->ln_ref && (!ml || !fml || !fml->ref_kf))) return PLVI_E_BADARG;
    if (win_cap > kEgWin) return PLVI_E_CAPACITY;
    a->mode = mode;
    a->win = win;
    a->n_win = n_win;
    a->win_cap = win_cap;
    a->lc_kf = lc_kf;
    a->n_lc = n_lc;
    a->lc_cap = lc_cap;
    a->o = *out;
    return PLVI_OK;
}

extern "C" int plvi_essential_graph_device(int cur_slot, int loop_slot, int mode, const int* d_win, const int* d_n_win,
                                           int win_cap, const int* d_lc_kf, const int* d_n_lc, int lc_cap,
                                           const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                                           const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                           const plvi_eg_features* fmp, const plvi_eg_features* fml,
                                           const plvi_eg_outputs* out, void* d_scratch, size_t scratch_bytes,
                                           void* stream) {
    EgArgs a;
    if (int rc = eg_graph_validate(mode, d_win, d_n_win, win_cap, d_lc_kf, d_n_lc, lc_cap, kf, eg, mp, ml, fmp, fml,
                                   out, &a))
        return rc;
    const int K = kf->kf_cap, n_order = eg->n_order;
    if (!d_scratch || scratch_bytes < plvi_essential_graph_scratch_bytes(K, n_order, win_cap, lc_cap))
        return PLVI_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (cur_slot < 0 || cur_slot >= K || loop_slot < 0 || loop_slot >= K) {
        hipLaunchKernelGGL(eg_query_error_kernel, dim3(1), dim3(64), 0, st, out->n_vert, (int*)nullptr, (int*)nullptr,
                           (int*)nullptr, out->n_edges, out->err);
        PLVI_CHECK(hipGetLastError());
        return PLVI_OK;
    }
    uint8_t* s = static_cast<uint8_t*>(d_scratch);
    a.cur = cur_slot;
    a.loop = loop_slot;
    a.g.rank = reinterpret_cast<int*>(s);
    a.wpos = reinterpret_cast<int*>(s += up256(4 * (size_t)K));
    a.cnt_e = reinterpret_cast<int*>(s += up256(4 * (size_t)K));
    a.cnt_v = reinterpret_cast<int*>(s += up256(4 * (size_t)n_order));
    a.pass = s + up256(4 * (size_t)n_order);
    if (int rc = eg_rank(a.g, a.wpos, st)) return rc;
    hipLaunchKernelGGL(eg_loopconn_kernel, dim3(1), dim3(kEgThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    if (n_order > 0) {
        const dim3 grid((n_order + kEgEdgeWaves - 1) / kEgEdgeWaves);
        hipLaunchKernelGGL(eg_edges_kernel<false>, grid, dim3(kEgEdgeThreads), 0, st, a);
        PLVI_CHECK(hipGetLastError());
        hipLaunchKernelGGL(eg_scan_kernel, dim3(1), dim3(kEgThreads), 0, st, a);
        PLVI_CHECK(hipGetLastError());
        hipLaunchKernelGGL(eg_edges_kernel<true>, grid, dim3(kEgEdgeThreads), 0, st, a);
        PLVI_CHECK(hipGetLastError());
    } else {
        hipLaunchKernelGGL(eg_scan_kernel, dim3(1), dim3(kEgThreads), 0, st, a);
        PLVI_CHECK(hipGetLastError());
    }
    const bool lines = ml && out->ln_ref;
    const int n_feat = (int)eg_max(out->pt_ref ? mp->n : 0, lines ? ml->n : 0);
    if (n_feat > 0) {
        EgRefs r;
        memset(&r, 0, sizeof r);
        if (out->pt_ref) {
            r.n[0] = mp->n, r.bad[0] = mp->bad, r.ref_kf[0] = fmp->ref_kf, r.map_id[0] = fmp->map_id;
            r.corr_by[0] = fmp->corr_by, r.corr_ref[0] = fmp->corr_ref, r.out[0] = out->pt_ref;
        }
        if (lines) {
            r.n[1] = ml->n, r.bad[1] = ml->bad, r.ref_kf[1] = fml->ref_kf, r.map_id[1] = fml->map_id;
            r.corr_by[1] = fml->corr_by, r.corr_ref[1] = fml->corr_ref, r.out[1] = out->ln_ref;
        }
        hipLaunchKernelGGL(eg_refs_kernel, dim3((n_feat + 255) / 256, 2), dim3(256), 0, st, a.g, cur_slot, mode, r);
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

// ---- the host forms.  Every pointer of the structs is a host pointer here; the copies below are what
// commit() turns into device pointers.
struct EgStaged {
    plvi_cull_keyframes kf;
    plvi_eg_keyframes eg;
    plvi_local_map_pool mp, ml;
    plvi_eg_features fmp, fml;
    bool lines;
};

static int eg_csr_len(const int* off, int K) { return off && off[K] > 0 ? off[K] : 0; }

static void eg_stage(HostStage& hs, EgStaged& d, const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                     const plvi_local_map_pool* mp, const plvi_local_map_pool* ml, const plvi_eg_features* fmp,
                     const plvi_eg_features* fml, bool graph) {
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut;
    const size_t K = (size_t)kf->kf_cap;
    d.lines = kf->ml && ml;
    d.kf = plvi_cull_keyframes{};
    d.kf.kf_cap = kf->kf_cap, d.kf.kp_cap = kf->kp_cap, d.kf.kl_cap = kf->kl_cap, d.kf.cand_stride = kf->cand_stride;
    d.kf.bad = kf->bad, d.kf.cand = kf->cand, d.kf.n_cand = kf->n_cand, d.kf.kf_id = kf->kf_id;
    d.eg = plvi_eg_keyframes{};
    d.eg.n_order = eg->n_order, d.eg.map_stride = eg->map_stride, d.eg.order = eg->order;
    d.mp = plvi_local_map_pool{};
    d.mp.n = mp->n, d.mp.bad = mp->bad;
    d.ml = plvi_local_map_pool{};
    if (ml) d.ml.n = ml->n, d.ml.bad = ml->bad;
    d.fmp = fmp ? *fmp : plvi_eg_features{};
    d.fml = fml && ml ? *fml : plvi_eg_features{};
    if (graph) {
        d.kf.init_kf = kf->init_kf, d.kf.prev_kf = kf->prev_kf, d.kf.next_kf = kf->next_kf;
        const int n_order = d.eg.n_order, map_stride = d.eg.map_stride;
        d.eg = *eg;
        d.eg.n_order = n_order, d.eg.map_stride = map_stride;
    } else {  // the walk reads the tables; the graph does not
        d.kf.mp = kf->mp, d.kf.nmp = kf->nmp;
        if (d.lines) d.kf.ml = kf->ml, d.kf.nml = kf->nml;
        d.fmp.ref_kf = d.fmp.map_id = d.fml.ref_kf = d.fml.map_id = nullptr;
    }
    hs.field(d.kf.bad, In, K);
    hs.field(d.kf.init_kf, In, K);
    hs.field(d.kf.mp, In, K, kf->kp_cap);
    hs.field(d.kf.nmp, In, K);
    hs.field(d.kf.ml, In, K, kf->kl_cap);
    hs.field(d.kf.nml, In, K);
    hs.field(d.kf.cand, In, K, kf->cand_stride);
    hs.field(d.kf.n_cand, In, K);
    hs.field(d.kf.kf_id, In, K);
    hs.field(d.kf.prev_kf, In, K);
    hs.field(d.kf.next_kf, In, K);
    hs.field(d.eg.order, In, (size_t)eg->n_order);
    hs.field(d.eg.map_id, In, K);
    hs.field(d.eg.parent, In, K);
    const size_t n_child = eg_csr_len(d.eg.child_off, kf->kf_cap), n_loop = eg_csr_len(d.eg.loop_off, kf->kf_cap);
    hs.field(d.eg.child_off, In, K + 1);
    hs.field(d.eg.child, In, n_child);
    hs.field(d.eg.loop_off, In, K + 1);
    hs.field(d.eg.loop, In, n_loop);
    hs.field(d.eg.imu, In, K);
    hs.field(d.eg.cand_w, In, K, kf->cand_stride);
    hs.field(d.eg.map_kf, In, K, eg->map_stride);
    hs.field(d.eg.map_w, In, K, eg->map_stride);
    hs.field(d.eg.map_n, In, K);
    hs.field(d.mp.bad, In, (size_t)mp->n);
    hs.field(d.ml.bad, In, (size_t)d.ml.n);
    const HostStage::Dir stamps = graph ? In : InOut;
    for (int p = 0; p < 2; ++p) {
        plvi_eg_features& f = p ? d.fml : d.fmp;
        const size_t n = (size_t)(p ? d.ml.n : d.mp.n);
        hs.field(f.ref_kf, In, n);
        hs.field(f.corr_by, stamps, n);
        hs.field(f.corr_ref, stamps, n);
        hs.field(f.map_id, In, n);
    }
}

extern "C" int plvi_loop_correct(int cur_slot, const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                                 const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                 const plvi_eg_features* fmp, const plvi_eg_features* fml,
                                 const plvi_loop_correct_outputs* out) {
    EgCorrectArgs chk;
    if (int rc = eg_correct_validate(kf, eg, mp, ml, fmp, fml, out, &chk)) return rc;
    HostStage hs;
    EgStaged d;
    eg_stage(hs, d, kf, eg, mp, ml, fmp, fml, false);
    plvi_loop_correct_outputs dout = *out;
    if (!d.lines) dout.lns = dout.lns_kf = nullptr;
    for (int** p : {&dout.n_win, &dout.n_sorted, &dout.n_pts, &dout.n_lns, &dout.err}) hs.field(*p, HostStage::Out, 1);
    // in/out: cells past a list's end keep the caller's fill
    hs.field(dout.win, HostStage::InOut, (size_t)out->win_cap);
    hs.field(dout.win_sorted, HostStage::InOut, (size_t)out->win_cap);
    hs.field(dout.pts, HostStage::InOut, (size_t)out->pt_cap);
    hs.field(dout.pts_kf, HostStage::InOut, (size_t)out->pt_cap);
    hs.field(dout.lns, HostStage::InOut, (size_t)out->ln_cap);
    hs.field(dout.lns_kf, HostStage::InOut, (size_t)out->ln_cap);
    const size_t sb = plvi_loop_correct_scratch_bytes(kf->kf_cap, mp->n, ml ? ml->n : 0);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_loop_correct_device(cur_slot, &d.kf, &d.eg, &d.mp, ml ? &d.ml : nullptr, fmp ? &d.fmp : nullptr,
                                          fml && ml ? &d.fml : nullptr, &dout, hs.dev(scr), sb, nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err ? PLVI_E_CAPACITY : PLVI_OK;
}

extern "C" int plvi_essential_graph(int cur_slot, int loop_slot, int mode, const int* win, const int* n_win,
                                    int win_cap, const int* lc_kf, const int* n_lc, int lc_cap,
                                    const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg,
                                    const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                    const plvi_eg_features* fmp, const plvi_eg_features* fml,
                                    const plvi_eg_outputs* out) {
    EgArgs chk;
    if (int rc = eg_graph_validate(mode, win, n_win, win_cap, lc_kf, n_lc, lc_cap, kf, eg, mp, ml, fmp, fml, out, &chk))
        return rc;
    HostStage hs;
    EgStaged d;
    eg_stage(hs, d, kf, eg, mp, ml, fmp, fml, true);
    const auto d_win = hs.in(win, (size_t)win_cap);
    const auto d_n_win = hs.in(n_win, 1);
    const auto d_lc = hs.in(lc_kf, (size_t)win_cap, (size_t)lc_cap);
    const auto d_n_lc = hs.in(n_lc, (size_t)win_cap);
    plvi_eg_outputs dout = *out;
    if (!ml) dout.ln_ref = nullptr;
    hs.field(dout.n_vert, HostStage::Out, 1);
    hs.field(dout.n_edges, HostStage::Out, 5);
    hs.field(dout.err, HostStage::Out, 1);
    hs.field(dout.vert, HostStage::InOut, (size_t)out->vert_cap);
    hs.field(dout.vert_flags, HostStage::InOut, (size_t)out->vert_cap);
    hs.field(dout.edge_a, HostStage::InOut, (size_t)out->edge_cap);
    hs.field(dout.edge_b, HostStage::InOut, (size_t)out->edge_cap);
    hs.field(dout.edge_kind, HostStage::InOut, (size_t)out->edge_cap);
    hs.field(dout.pt_ref, HostStage::InOut, (size_t)mp->n);
    hs.field(dout.ln_ref, HostStage::InOut, (size_t)(ml ? ml->n : 0));
    const size_t sb = plvi_essential_graph_scratch_bytes(kf->kf_cap, eg->n_order, win_cap, lc_cap);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_essential_graph_device(cur_slot, loop_slot, mode, hs.dev(d_win), hs.dev(d_n_win), win_cap,
                                             hs.dev(d_lc), hs.dev(d_n_lc), lc_cap, &d.kf, &d.eg, &d.mp,
                                             ml ? &d.ml : nullptr, fmp ? &d.fmp : nullptr,
                                             fml && ml ? &d.fml : nullptr, &dout, hs.dev(scr), sb, nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err & ~PLVI_EG_ERR_NO_VERTEX ? PLVI_E_CAPACITY : PLVI_OK;
}

// ---- LoopConnections
static size_t eg_lc_fixed(int n_win, int kf_cap) {  // rank, the window, the snapshot counts
    return up256(4 * (size_t)kf_cap) + 2 * up256(4 * (size_t)n_win);
}

extern "C" size_t plvi_loop_connections_scratch_bytes(int n_win, int kf_cap, int conn_cap) {
    if (n_win < 0 || kf_cap < 0 || conn_cap < 0) return 0;
    return plvi_covis_scratch_bytes(1, kf_cap) + eg_lc_fixed(n_win, kf_cap) + up256(4 * (size_t)n_win * conn_cap);
}

static int eg_lc_validate(plvi_covis_graph* h, int n_win, const int* win, const plvi_covis_keyframes* kf,
                          const plvi_local_map_pool* mp, const plvi_covis_outputs* out, int lc_cap, const int* lc_kf,
                          const int* n_lc, const int* err) {
    if (!h || !kf || !mp || !out || n_win < 0 || lc_cap < 0 || kf->n_order < 0 || kf->kf_cap < 1) return PLVI_E_BADARG;
    if (!err || (n_win > 0 && (!win || !n_lc || (lc_cap > 0 && !lc_kf))) || (kf->n_order > 0 && !kf->order))
        return PLVI_E_BADARG;
    if (!out->n_counted || !out->n_conn || !out->kf_max || !out->w_max || !out->new_parent || !out->err)
        return PLVI_E_BADARG;
    if (n_win > kEgWin || kf->kf_cap > (1 << 24) || kf->n_order > (1 << 30)) return PLVI_E_CAPACITY;
    return PLVI_OK;
}

extern "C" int plvi_loop_connections_device(plvi_covis_graph* h, int n_win, const int* win,
                                            const plvi_covis_keyframes* kf, const plvi_local_map_pool* mp,
                                            const plvi_local_map_pool* ml, const plvi_covis_outputs* out, int lc_cap,
                                            int* d_lc_kf, int* d_n_lc, int* d_err, void* d_scratch,
                                            size_t scratch_bytes, void* stream) {
    if (int rc = eg_lc_validate(h, n_win, win, kf, mp, out, lc_cap, d_lc_kf, d_n_lc, d_err)) return rc;
    const int *ord_kf, *ord_n, *map_kf, *map_n;
    int C;
    if (int rc = plvi_covis_rows(h, &ord_kf, nullptr, &ord_n, &C)) return rc;
    if (int rc = plvi_covis_map_rows(h, &map_kf, nullptr, &map_n, nullptr)) return rc;
    const int K = kf->kf_cap;
    if (!d_scratch || scratch_bytes < plvi_loop_connections_scratch_bytes(n_win, K, C)) return PLVI_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* s = static_cast<uint8_t*>(d_scratch);
    const size_t cov_sb = plvi_covis_scratch_bytes(1, K);
    void* cov_scratch = s;
    int* rank = reinterpret_cast<int*>(s += cov_sb);
    int* d_win = reinterpret_cast<int*>(s += up256(4 * (size_t)K));
    int* snap_n = reinterpret_cast<int*>(s += up256(4 * (size_t)n_win));
    int* snap = reinterpret_cast<int*>(s + up256(4 * (size_t)n_win));
    for (int i0 = 0; i0 == 0 || i0 < n_win; i0 += kEgChunk) {  // one launch even when empty: it clears err
        EgChunk c;
        c.n = n_win - i0 < kEgChunk ? n_win - i0 : kEgChunk;
        c.base = i0;
        if (c.n > 0) memcpy(c.v, win + i0, 4 * (size_t)c.n);
        hipLaunchKernelGGL(eg_set_kernel, dim3(2), dim3(256), 0, st, d_win, d_err, c);
        PLVI_CHECK(hipGetLastError());
    }
    if (n_win == 0) return PLVI_OK;
    for (int p = 0; p < n_win; ++p) {
        const int slot = win[p];
        if (slot < 0 || slot >= K) continue;
        hipLaunchKernelGGL(eg_snapshot_kernel, dim3(1), dim3(256), 0, st, ord_kf, ord_n, C, slot, snap + (size_t)p * C,
                           snap_n + p);
        PLVI_CHECK(hipGetLastError());
        // exactly the batch call of one query, its outputs at window position p
        const plvi_covis_outputs at{out->n_counted + p, out->n_conn + p,     out->kf_max + p,
                                    out->w_max + p,     out->new_parent + p, out->err + p};
        if (int rc = plvi_covis_update_batch(h, 1, &slot, kf, mp, ml, &at, cov_scratch, cov_sb, stream)) return rc;
    }
    EgGraph g;
    memset(&g, 0, sizeof g);
    g.K = K, g.n_order = kf->n_order, g.order = kf->order, g.rank = rank;
    if (int rc = eg_rank(g, nullptr, st)) return rc;
    const EgLcArgs a{K, C, kf->n_order, n_win, lc_cap, map_kf, map_n, d_win, snap, snap_n, rank, d_lc_kf, d_n_lc, d_err};
    hipLaunchKernelGGL(eg_diff_kernel, dim3(n_win), dim3(kEgDiffThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

// The window from host tables, synchronous: out holds n_win entries each; first_conn, parent and covis are
// updated in place.
extern "C" int plvi_loop_connections(plvi_covis_graph* h, int n_win, const int* win, const plvi_covis_keyframes* kf,
                                     const plvi_local_map_pool* mp, const plvi_local_map_pool* ml,
                                     const plvi_covis_outputs* out, int lc_cap, int* lc_kf, int* n_lc, int* err) {
    if (int rc = eg_lc_validate(h, n_win, win, kf, mp, out, lc_cap, lc_kf, n_lc, err)) return rc;
    if (mp->n < 0 || (ml && ml->n < 0) || kf->kp_cap < 0 || kf->kl_cap < 0) return PLVI_E_BADARG;
    int C;
    if (int rc = plvi_covis_rows(h, nullptr, nullptr, nullptr, &C)) return rc;
    const bool with_lines = kf->ml && ml;
    const size_t K = (size_t)kf->kf_cap;
    plvi_covis_keyframes dk = *kf;
    plvi_local_map_pool dmp = *mp, dml = with_lines ? *ml : plvi_local_map_pool{};
    plvi_covis_outputs dout = *out;
    if (!with_lines) dk.ml = dk.nml = nullptr;
    HostStage hs;
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut;
    hs.field(dk.bad, In, K);
    hs.field(dk.order, In, (size_t)kf->n_order);
    hs.field(dk.mp, In, K, kf->kp_cap);
    hs.field(dk.nmp, In, K);
    hs.field(dk.ml, In, K, kf->kl_cap);
    hs.field(dk.nml, In, K);
    hs.field(dk.map_id, In, K);
    hs.field(dk.init_kf, In, K);
    hs.field(dk.first_conn, InOut, K);
    hs.field(dk.parent, InOut, K);
    hs.field(dk.covis, InOut, K, PLVI_KFDB_NEIGHBOURS);
    for (plvi_local_map_pool* p : {&dmp, &dml}) {
        if (p == &dml && !with_lines) continue;
        const size_t n = (size_t)p->n, n_obs = p->obs_off && p->obs_off[n] > 0 ? (size_t)p->obs_off[n] : 0;
        p->pos = nullptr, p->sep = nullptr, p->normal = nullptr, p->dist = nullptr, p->desc = nullptr;
        hs.field(p->bad, In, n);
        hs.field(p->obs_off, In, n + 1);
        hs.field(p->obs_kf, In, n_obs);
    }
    // in/out: the cells of positions that name no slot keep the caller's fill
    for (int** o : {&dout.n_counted, &dout.n_conn, &dout.kf_max, &dout.w_max, &dout.new_parent, &dout.err})
        hs.field(*o, InOut, (size_t)n_win);
    const auto d_lc = hs.inout(lc_kf, (size_t)n_win, (size_t)lc_cap);
    const auto d_n_lc = hs.out(n_lc, (size_t)n_win);
    const auto d_err = hs.out(err, 1);
    const size_t sb = plvi_loop_connections_scratch_bytes(n_win, kf->kf_cap, C);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_loop_connections_device(h, n_win, win, &dk, &dmp, with_lines ? &dml : nullptr, &dout, lc_cap,
                                              hs.dev(d_lc), hs.dev(d_n_lc), hs.dev(d_err), hs.dev(scr), sb, nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *err ? PLVI_E_CAPACITY : PLVI_OK;
}
