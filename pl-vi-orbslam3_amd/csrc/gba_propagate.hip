// gba_propagate.hip — the map-wide traversal behind an accepted global bundle adjustment, the second half of
// LoopClosing::RunGlobalBundleAdjustment[WithLines] (src/LoopClosing.cc:3727-3930 and its line twin), over the
// resident tables (include/plvi_frontend.h, "GBA propagation"):
//   plvi_gba_walk      the breadth-first walk of the spanning tree from the map's origins (:3727-3843): integers
//                      only.  Every 4x4 pose product, the velocity, the bias and SetPose stay with the caller.
//   plvi_gba_correct   the pass over every MapPoint / MapLine (:3847-3930): the solver's position as a bit copy,
//                      or Rwc * (Rcw_bef * X + tcw_bef) + twc of the reference keyframe, a thread per feature.
//
// The walk.  GetChilds() is a std::set<KeyFrame*>: a row is taken in ascending rank (the first position in
// `order`, n_order + slot for a slot order does not name: EgGraph::rank_of of essential_graph.hip).
//   gba_fill / gba_rank   rank[] by slot as eg_fill / eg_rank make it, and first[] = INT_MAX.
//   gba_rows_kernel       a wave per slot: every entry of the row is placed by counting the entries with a smaller
//                         (key, index), 64 entries at a time; the key of an entry that is out of range or bad is
//                         above every rank, so the usable entries come first, and their number is cnt[slot].
//   gba_walk_kernel       one 1024-thread workgroup.  A step takes up to 1024 queue entries: a scan of their
//                         usable counts gives every appended child its queue position (FIFO order falls out of
//                         the scan), then a thread per appended position finds its entry by bisection of the scan
//                         and appends, stamps and flags its child -- a star and a chain are the same code.  While
//                         the frontier fits one wave (a SLAM spanning tree is close to a chain), wave 0 runs the
//                         steps alone, with no workgroup barrier.
// Two queue entries of one step that append the same child happen only when the tables are no forest; the lower
// position is the new one there too, as in the sequential loop: first[child] takes the atomicMin of the positions.
//
// Arithmetic of the correction: cv::Mat R * X + t through cv::gemm's small-matrix path, the form frustum.hip
// takes for Frame::isInFrustum's Rcw * P + tcw (pose_row, restated here; PLVI_COMPAT_GEMM_FMA picks the
// AVX2-dispatched contraction).  Lines narrow each endpoint to float (Converter::toCvMat(Vector3d)) and widen the
// result (Converter::toVector3d).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>

#include "block_prims.h"
#include "host_stage.h"
#include "plvi_common.h"
#include "plvi_math.h"

namespace plvi {

namespace {

constexpr int kGbaThreads = 1024, kGbaWaves = kGbaThreads / kWave;
constexpr int kGbaRowThreads = 256;  // gba_rows_kernel: four slots per workgroup
constexpr int kGbaRankNone = INT_MAX;
constexpr unsigned kGbaNoKey = 0xffffffffu;
constexpr int kGbaCorrectThreads = 256;

struct WalkArgs {
    int K, n_order, n_origins, walk_cap;
    unsigned loop_kf;
    const uint8_t* bad;
    const int *order, *child_off, *child, *origins;
    unsigned* stamp;                          // kf_ba_for
    int *rank, *first, *cnt, *sorted, *queue;  // [K] each, scratch
    int* walk;
    int* walk_parent;
    uint8_t* walk_new;
    int *n_walk, *n_new, *err;
    uint8_t* visited;
};

__global__ void gba_fill_kernel(int* rank, int* first, int K) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K) return;
    rank[i] = kGbaRankNone;
    first[i] = INT_MAX;
}

__global__ void gba_rank_kernel(int* rank, int K, const int* order, int n_order) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_order) return;
    const int s = order[k];
    if (in_range(s, K)) atomicMin(rank + s, k);
}

// the sort key of a child entry: its rank, or kGbaNoKey for one the walk skips
__device__ __forceinline__ unsigned child_key(const WalkArgs& a, int c) {
    if (!in_range(c, a.K) || a.bad[c]) return kGbaNoKey;
    const int r = a.rank[c];
    return r == kGbaRankNone ? (unsigned)a.n_order + (unsigned)c : (unsigned)r;
}

// the row of slot s as [o0, o0 + len); a row that is not inside the first K entries of child is read as empty
// (a forest has at most K - 1 entries) and reported
__device__ __forceinline__ int child_row(const WalkArgs& a, int s, int* o0, bool* broken) {
    *o0 = 0;
    *broken = false;
    if (!a.child_off) return 0;
    const int b = a.child_off[s], e = a.child_off[s + 1];
    if (b < 0 || e < b || e > min(a.K, a.child_off[a.K])) {
        *broken = true;
        return 0;
    }
    *o0 = b;
    return e - b;
}

__global__ __launch_bounds__(kGbaRowThreads) void gba_rows_kernel(const WalkArgs a) {
    const int lane = threadIdx.x & (kWave - 1);
    const int s = blockIdx.x * (kGbaRowThreads / kWave) + threadIdx.x / kWave;
    if (s >= a.K) return;
    int o0;
    bool broken;
    const int len = child_row(a, s, &o0, &broken);
    if (broken && lane == 0) atomicOr(a.err, PLVI_GBA_ERR_CYCLE);
    int usable = 0;
    for (int e = lane; e < len; e += kWave) {
        const int c = a.child[o0 + e];
        const unsigned key = child_key(a, c);
        int p = 0;
        for (int j = 0; j < len; ++j) {
            const unsigned kj = child_key(a, a.child[o0 + j]);
            p += kj < key || (kj == key && j < e);
        }
        a.sorted[o0 + p] = c;  // o0 + len <= K
        usable += key != kGbaNoKey;
    }
    usable = wave_sum(usable);
    if (lane == 0) a.cnt[s] = usable;
}

// what the members of a step share: a barrier that also orders LDS and global memory among them
template <bool kBlock>
__device__ __forceinline__ void step_sync() {
    if (kBlock) {
        __syncthreads();
    } else {  // one wave: no s_barrier, but its stores are complete before another lane reads them
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// One step over the queue entries [head, head + m), m <= NT (1024 with kBlock, 64 without), by the NT threads
// t = 0 .. NT - 1; tail is the queue's end.  Returns the number of children appended, or -1 when they would pass
// the queue's K entries (nothing is appended then).  *n_new grows by this thread's new children.
template <bool kBlock>
__device__ int walk_step(const WalkArgs& a, int head, int m, int tail, int t, int* s_excl, int* s_slot, int* s_off,
                         int* s_wave, int* n_new) {
    constexpr int NT = kBlock ? kGbaThreads : kWave;
    int slot = -1, n = 0, o0 = 0;
    if (t < m) {
        slot = a.queue[head + t];
        n = a.cnt[slot];
        bool broken;
        child_row(a, slot, &o0, &broken);
    }
    int total, excl;
    if (kBlock) {
        excl = block_scan<kGbaWaves>(n, s_wave, t, &total);
    } else {
        const int incl = wave_incl_scan(n, t);
        total = __shfl(incl, kWave - 1, kWave);
        excl = incl - n;
    }
    step_sync<kBlock>();  // the arrays may still be read from the step before
    s_excl[t] = t < m ? excl : INT_MAX;
    s_slot[t] = slot;
    s_off[t] = o0;
    step_sync<kBlock>();
    if (total > a.K - tail) return -1;
    for (int t0 = 0; t0 < total; t0 += NT) {
        const int k = t0 + t;
        const bool live = k < total;
        int c = -1, parent = -1, p = 0;
        unsigned old = 0;
        if (live) {
            int lo = 0, hi = m;  // the first entry whose scan is above k, less one, owns position k
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_excl[mid] > k) hi = mid;
                else lo = mid + 1;
            }
            const int i = lo - 1;
            parent = s_slot[i];
            c = a.sorted[s_off[i] + (k - s_excl[i])];
            p = tail + k;
            atomicMin(a.first + c, p);
            old = a.stamp[c];
        }
        step_sync<kBlock>();
        if (live) {
            const bool is_new = old != a.loop_kf && a.first[c] == p;
            if (is_new) a.stamp[c] = a.loop_kf;
            a.queue[p] = c;
            if (p < a.walk_cap) {
                a.walk[p] = c;
                a.walk_parent[p] = parent;
                a.walk_new[p] = is_new;
            }
            if (a.visited) a.visited[c] = 1;
            *n_new += is_new;
        }
        step_sync<kBlock>();  // the stamps of this tile are read by the next
    }
    return total;
}

__global__ __launch_bounds__(kGbaThreads) void gba_walk_kernel(const WalkArgs a) {
    __shared__ int s_excl[kGbaThreads], s_slot[kGbaThreads], s_off[kGbaThreads];
    __shared__ int s_wave[kGbaWaves];
    __shared__ int s_head, s_tail, s_stop, s_new;
    const int tid = threadIdx.x;
    if (tid == 0) s_new = 0;

    // the queue starts as the origins in range, in the order given
    int tail = 0, e = 0;
    for (int t0 = 0; t0 < a.n_origins; t0 += kGbaThreads) {
        const int i = t0 + tid;
        const int s = i < a.n_origins ? a.origins[i] : -1;
        const bool ok = in_range(s, a.K);
        if (i < a.n_origins && !ok) e |= PLVI_GBA_ERR_ORIGIN;
        int tot;
        const int p = tail + block_scan<kGbaWaves>(ok, s_wave, tid, &tot);
        if (ok) {
            if (p < a.K) {
                a.queue[p] = s;
                if (p < a.walk_cap) {
                    a.walk[p] = s;
                    a.walk_parent[p] = -1;
                    a.walk_new[p] = 0;
                }
                if (a.visited) a.visited[s] = 1;
            } else {
                e |= PLVI_GBA_ERR_CYCLE;
            }
        }
        tail += tot;
    }
    if (e) atomicOr(a.err, e);
    if (tid == 0) {
        s_head = 0;
        s_tail = min(tail, a.K);
        s_stop = tail > a.K;
    }

    int n_new = 0;
    for (;;) {
        __syncthreads();
        int head = s_head;
        tail = s_tail;
        const bool stop = s_stop;
        __syncthreads();
        if (stop || head >= tail) break;
        if (tail - head <= kWave) {
            if (tid >= kWave) continue;
            bool cycle = false;
            while (head < tail && tail - head <= kWave) {
                const int m = tail - head;
                const int got = walk_step<false>(a, head, m, tail, tid, s_excl, s_slot, s_off, s_wave, &n_new);
                if (got < 0) {
                    cycle = true;
                    break;
                }
                head += m;
                tail += got;
            }
            if (tid == 0) {
                s_head = head;
                s_tail = tail;
                s_stop = cycle;
            }
        } else {
            const int m = min(tail - head, kGbaThreads);
            const int got = walk_step<true>(a, head, m, tail, tid, s_excl, s_slot, s_off, s_wave, &n_new);
            if (tid == 0) {
                s_head = head + m;
                s_tail = tail + max(got, 0);
                s_stop = got < 0;
            }
        }
    }
    block_add(n_new, &s_new, tid);
    __syncthreads();
    if (tid == 0) {
        *a.n_walk = tail;
        *a.n_new = s_new;
        int err = 0;
        if (s_stop) err |= PLVI_GBA_ERR_CYCLE;
        if (tail > a.walk_cap) err |= PLVI_GBA_ERR_WALK;
        if (err) atomicOr(a.err, err);
    }
}

// ---- the feature correction
struct CorrectArgs {
    int n, K, lines, fma_form, map;
    unsigned loop_kf;
    const uint8_t* bad;
    const int *map_id, *ref_kf;
    const unsigned *feat_ba_for, *kf_ba_for;
    const uint8_t* has_bef;
    const float *tcw_bef, *twc;
    const float* pos;
    const double* sep;
    const float* pos_gba;
    const double* sep_gba;
    float* out_pos;  // may be pos
    double* out_sep;  // may be sep
    uint8_t* state;
    int *counts, *err;
};

// one row of R * P + t through cv::gemm's small-matrix path (frustum.hip)
__device__ __forceinline__ float pose_row(const float* R, float px, float py, float pz, float t, bool fma_form) {
    const float s = fma_form ? rfmaf(R[2], pz, rfmaf(R[0], px, R[1] * py)) : (R[0] * px + R[1] * py) + R[2] * pz;
    return (float)((double)s + (double)t);
}

// X' = Rwc * (Rcw_bef * X + tcw_bef) + twc; a pose is the nine entries of R row-major, then t
__device__ __forceinline__ void correct_point(const float* bef, const float* twc, bool fma_form, float* X) {
    float c[3], w[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = pose_row(bef + 3 * r, X[0], X[1], X[2], bef[9 + r], fma_form);
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = pose_row(twc + 3 * r, c[0], c[1], c[2], twc[9 + r], fma_form);
#pragma unroll
    for (int r = 0; r < 3; ++r) X[r] = w[r];
}

__global__ __launch_bounds__(kGbaCorrectThreads) void gba_correct_kernel(const CorrectArgs a) {
    __shared__ int s_cnt[3];
    const int tid = threadIdx.x;
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    const long long gid = (long long)blockIdx.x * kGbaCorrectThreads + tid;
    const bool live = gid < a.n;
    const size_t id = (size_t)gid;
    int st = 0;
    if (live && !a.bad[id] && (!a.map_id || a.map_id[id] == a.map)) {
        if (a.feat_ba_for[id] == a.loop_kf) {
            st = 1;
            if (a.lines) {
#pragma unroll
                for (int c = 0; c < 6; ++c) a.out_sep[6 * id + c] = a.sep_gba[6 * id + c];
            } else {
                // a bit copy: a float register would be free to quiet a signalling NaN
                const uint32_t* src = reinterpret_cast<const uint32_t*>(a.pos_gba);
                uint32_t* dst = reinterpret_cast<uint32_t*>(a.out_pos);
#pragma unroll
                for (int c = 0; c < 3; ++c) dst[3 * id + c] = src[3 * id + c];
            }
        } else {
            const int r = a.ref_kf[id];
            if (!in_range(r, a.K)) {
                atomicOr(a.err, PLVI_GBA_ERR_REF);
            } else if (a.kf_ba_for[r] == a.loop_kf && a.has_bef[r]) {
                st = 2;
                float bef[12], twc[12];
#pragma unroll
                for (int c = 0; c < 12; ++c) {
                    bef[c] = a.tcw_bef[12 * (size_t)r + c];
                    twc[c] = a.twc[12 * (size_t)r + c];
                }
                if (a.lines) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        float X[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) X[c] = (float)a.sep[6 * id + 3 * e + c];
                        correct_point(bef, twc, a.fma_form, X);
#pragma unroll
                        for (int c = 0; c < 3; ++c) a.out_sep[6 * id + 3 * e + c] = (double)X[c];
                    }
                } else {
                    float X[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) X[c] = a.pos[3 * id + c];
                    correct_point(bef, twc, a.fma_form, X);
#pragma unroll
                    for (int c = 0; c < 3; ++c) a.out_pos[3 * id + c] = X[c];
                }
            }
        }
    }
    if (live) a.state[id] = (uint8_t)st;
#pragma unroll
    for (int k = 0; k < 3; ++k) block_add((int)(live && st == k), &s_cnt[k], tid);
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(a.counts + tid, s_cnt[tid]);
}

struct WalkLayout {
    size_t rank, first, cnt, sorted, queue, total;
};

WalkLayout walk_layout(int kf_cap) {
    const size_t col = up256(4 * (size_t)kf_cap);
    return {0, col, 2 * col, 3 * col, 4 * col, 5 * col};
}

int walk_validate(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg, const int* origins, int n_origins,
                  unsigned* kf_ba_for, const plvi_gba_walk_outputs* out) {
    if (!kf || !eg || !out || kf->kf_cap < 1 || eg->n_order < 0 || n_origins < 0 || out->walk_cap < 0)
        return PLVI_E_BADARG;
    if (!kf->bad || !kf_ba_for || (eg->n_order > 0 && !eg->order) || (n_origins > 0 && !origins))
        return PLVI_E_BADARG;
    if ((eg->child_off == nullptr) != (eg->child == nullptr)) return PLVI_E_BADARG;
    if (!out->n_walk || !out->n_new || !out->err) return PLVI_E_BADARG;
    if (out->walk_cap > 0 && (!out->walk || !out->walk_parent || !out->walk_new)) return PLVI_E_BADARG;
    if (kf->kf_cap > (1 << 24) || eg->n_order > (1 << 30)) return PLVI_E_CAPACITY;
    return PLVI_OK;
}

int correct_validate(const plvi_local_map_pool* pool, const plvi_eg_features* feat, const unsigned* feat_ba_for,
                     const void* pos_gba, const plvi_gba_poses* poses, const plvi_gba_params* p,
                     const plvi_gba_correct_outputs* out) {
    if (!pool || !feat || !poses || !p || !out || pool->n < 0 || poses->kf_cap < 1) return PLVI_E_BADARG;
    if (p->kind != PLVI_GBA_POINTS && p->kind != PLVI_GBA_LINES) return PLVI_E_BADARG;
    if (!out->counts || !out->err) return PLVI_E_BADARG;
    if (pool->n == 0) return PLVI_OK;
    const bool lines = p->kind == PLVI_GBA_LINES;
    if (!pool->bad || !feat->ref_kf || !feat_ba_for || !pos_gba || !out->state) return PLVI_E_BADARG;
    if (lines ? !pool->sep || !out->sep : !pool->pos || !out->pos) return PLVI_E_BADARG;
    if (!poses->kf_ba_for || !poses->has_bef || !poses->tcw_bef || !poses->twc) return PLVI_E_BADARG;
    return PLVI_OK;
}

}  // namespace

}  // namespace plvi

using namespace plvi;

extern "C" size_t plvi_gba_walk_scratch_bytes(int kf_cap) {
    if (kf_cap < 0) return 0;
    return walk_layout(kf_cap).total;
}

extern "C" int plvi_gba_walk_device(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg, const int* d_origins,
                                    int n_origins, unsigned loop_kf, unsigned* d_kf_ba_for,
                                    const plvi_gba_walk_outputs* out, void* d_scratch, size_t scratch_bytes,
                                    void* stream) {
    if (int rc = walk_validate(kf, eg, d_origins, n_origins, d_kf_ba_for, out)) return rc;
    const int K = kf->kf_cap;
    const WalkLayout lay = walk_layout(K);
    if (!d_scratch || scratch_bytes < lay.total) return PLVI_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    PLVI_CHECK(hipMemsetAsync(out->n_walk, 0, sizeof(int), st));
    PLVI_CHECK(hipMemsetAsync(out->n_new, 0, sizeof(int), st));
    PLVI_CHECK(hipMemsetAsync(out->err, 0, sizeof(int), st));

    uint8_t* scr = static_cast<uint8_t*>(d_scratch);
    WalkArgs a;
    memset(&a, 0, sizeof a);
    a.K = K, a.n_order = eg->n_order, a.n_origins = n_origins, a.walk_cap = out->walk_cap, a.loop_kf = loop_kf;
    a.bad = kf->bad, a.order = eg->order, a.child_off = eg->child_off, a.child = eg->child, a.origins = d_origins;
    a.stamp = d_kf_ba_for;
    a.rank = reinterpret_cast<int*>(scr + lay.rank), a.first = reinterpret_cast<int*>(scr + lay.first);
    a.cnt = reinterpret_cast<int*>(scr + lay.cnt), a.sorted = reinterpret_cast<int*>(scr + lay.sorted);
    a.queue = reinterpret_cast<int*>(scr + lay.queue);
    a.walk = out->walk, a.walk_parent = out->walk_parent, a.walk_new = out->walk_new;
    a.n_walk = out->n_walk, a.n_new = out->n_new, a.err = out->err, a.visited = out->visited;

    hipLaunchKernelGGL(gba_fill_kernel, dim3((K + 255) / 256), dim3(256), 0, st, a.rank, a.first, K);
    PLVI_CHECK(hipGetLastError());
    if (a.n_order > 0) {
        hipLaunchKernelGGL(gba_rank_kernel, dim3((a.n_order + 255) / 256), dim3(256), 0, st, a.rank, K, a.order,
                           a.n_order);
        PLVI_CHECK(hipGetLastError());
    }
    const int per = kGbaRowThreads / kWave;
    hipLaunchKernelGGL(gba_rows_kernel, dim3((K + per - 1) / per), dim3(kGbaRowThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    hipLaunchKernelGGL(gba_walk_kernel, dim3(1), dim3(kGbaThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_gba_walk(const plvi_cull_keyframes* kf, const plvi_eg_keyframes* eg, const int* origins,
                             int n_origins, unsigned loop_kf, unsigned* kf_ba_for, const plvi_gba_walk_outputs* out) {
    if (int rc = walk_validate(kf, eg, origins, n_origins, kf_ba_for, out)) return rc;
    const size_t K = (size_t)kf->kf_cap;
    if (eg->child_off && eg->child_off[K] < 0) return PLVI_E_BADARG;
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut;
    HostStage hs;
    plvi_cull_keyframes dk;
    memset(&dk, 0, sizeof dk);
    dk.kf_cap = kf->kf_cap, dk.bad = kf->bad;
    hs.field(dk.bad, In, K);
    plvi_eg_keyframes de;
    memset(&de, 0, sizeof de);
    de.n_order = eg->n_order, de.order = eg->order, de.child_off = eg->child_off, de.child = eg->child;
    hs.field(de.order, In, (size_t)eg->n_order);
    hs.field(de.child_off, In, K + 1);
    hs.field(de.child, In, eg->child_off ? (size_t)eg->child_off[K] : 0);
    const auto O = hs.in(origins, (size_t)n_origins);
    const auto S = hs.inout(kf_ba_for, K);
    // in/out: cells past the list's end, and the cells of visited the walk does not reach, keep the caller's values
    plvi_gba_walk_outputs dout = *out;
    hs.field(dout.walk, InOut, (size_t)out->walk_cap);
    hs.field(dout.walk_parent, InOut, (size_t)out->walk_cap);
    hs.field(dout.walk_new, InOut, (size_t)out->walk_cap);
    hs.field(dout.visited, InOut, K);
    hs.field(dout.n_walk, HostStage::Out, 1);
    hs.field(dout.n_new, HostStage::Out, 1);
    hs.field(dout.err, HostStage::Out, 1);
    const size_t sb = plvi_gba_walk_scratch_bytes(kf->kf_cap);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_gba_walk_device(&dk, &de, hs.dev(O), n_origins, loop_kf, hs.dev(S), &dout, hs.dev(scr), sb,
                                      nullptr))
        return rc;
    if (int rc = hs.fetch()) return rc;
    return *out->err ? PLVI_E_CAPACITY : *out->n_walk;
}

extern "C" int plvi_gba_correct_device(const plvi_local_map_pool* pool, const plvi_eg_features* feat,
                                       const unsigned* d_feat_ba_for, const void* d_pos_gba,
                                       const plvi_gba_poses* poses, const plvi_gba_params* params,
                                       const plvi_gba_correct_outputs* out, void* stream) {
    if (int rc = correct_validate(pool, feat, d_feat_ba_for, d_pos_gba, poses, params, out)) return rc;
    hipStream_t st = (hipStream_t)stream;
    PLVI_CHECK(hipMemsetAsync(out->counts, 0, 3 * sizeof(int), st));
    PLVI_CHECK(hipMemsetAsync(out->err, 0, sizeof(int), st));
    if (pool->n == 0) return PLVI_OK;
    CorrectArgs a;
    memset(&a, 0, sizeof a);
    a.n = pool->n, a.K = poses->kf_cap, a.lines = params->kind == PLVI_GBA_LINES;
    a.fma_form = (params->compat & PLVI_COMPAT_GEMM_FMA) != 0, a.map = params->map, a.loop_kf = params->loop_kf;
    a.bad = pool->bad, a.map_id = feat->map_id, a.ref_kf = feat->ref_kf;
    a.feat_ba_for = d_feat_ba_for, a.kf_ba_for = poses->kf_ba_for, a.has_bef = poses->has_bef;
    a.tcw_bef = poses->tcw_bef, a.twc = poses->twc;
    a.pos = pool->pos, a.sep = pool->sep;
    a.pos_gba = static_cast<const float*>(d_pos_gba), a.sep_gba = static_cast<const double*>(d_pos_gba);
    a.out_pos = out->pos, a.out_sep = out->sep, a.state = out->state, a.counts = out->counts, a.err = out->err;
    hipLaunchKernelGGL(gba_correct_kernel, dim3((unsigned)(((long long)a.n + kGbaCorrectThreads - 1) / kGbaCorrectThreads)),
                       dim3(kGbaCorrectThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_gba_correct(const plvi_local_map_pool* pool, const plvi_eg_features* feat,
                                const unsigned* feat_ba_for, const void* pos_gba, const plvi_gba_poses* poses,
                                const plvi_gba_params* params, const plvi_gba_correct_outputs* out) {
    if (int rc = correct_validate(pool, feat, feat_ba_for, pos_gba, poses, params, out)) return rc;
    const size_t n = (size_t)pool->n, K = (size_t)poses->kf_cap;
    const bool lines = params->kind == PLVI_GBA_LINES;
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut;
    HostStage hs;
    plvi_local_map_pool dp;
    memset(&dp, 0, sizeof dp);
    dp.n = pool->n, dp.bad = pool->bad;
    hs.field(dp.bad, In, n);
    plvi_eg_features df;
    memset(&df, 0, sizeof df);
    df.ref_kf = feat->ref_kf, df.map_id = feat->map_id;
    hs.field(df.ref_kf, In, n);
    hs.field(df.map_id, In, n);
    const auto B = hs.in(feat_ba_for, n);
    const auto Gp = lines ? Staged<float>() : hs.in(static_cast<const float*>(pos_gba), n, 3);
    const auto Gl = lines ? hs.in(static_cast<const double*>(pos_gba), n, 6) : Staged<double>();
    plvi_gba_poses dq = *poses;
    hs.field(dq.kf_ba_for, In, K);
    hs.field(dq.has_bef, In, K);
    hs.field(dq.tcw_bef, In, K, 12);
    hs.field(dq.twc, In, K, 12);
    // in/out: the rows the call leaves alone keep the caller's values.  An output that is the pool's own column is
    // staged once and read in place, as in the device form.
    plvi_gba_correct_outputs dout = *out;
    const bool alias = lines ? out->sep == pool->sep : out->pos == pool->pos;
    if (lines) {
        dout.pos = nullptr;
        dp.sep = alias ? nullptr : pool->sep;
        hs.field(dp.sep, In, n, 6);
        hs.field(dout.sep, InOut, n, 6);
    } else {
        dout.sep = nullptr;
        dp.pos = alias ? nullptr : pool->pos;
        hs.field(dp.pos, In, n, 3);
        hs.field(dout.pos, InOut, n, 3);
    }
    hs.field(dout.state, InOut, n);
    hs.field(dout.counts, HostStage::Out, 3);
    hs.field(dout.err, HostStage::Out, 1);
    if (int rc = hs.commit()) return rc;
    if (alias && lines) dp.sep = dout.sep;
    if (alias && !lines) dp.pos = dout.pos;
    const void* g = lines ? static_cast<const void*>(hs.dev(Gl)) : static_cast<const void*>(hs.dev(Gp));
    if (int rc = plvi_gba_correct_device(&dp, &df, hs.dev(B), g, &dq, params, &dout, nullptr)) return rc;
    if (int rc = hs.fetch()) return rc;
    if (*out->err) return PLVI_E_CAPACITY;
    return out->counts[1] + out->counts[2];
}
