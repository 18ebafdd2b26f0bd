// local_map.hip — Tracking::UpdateLocalMap / UpdateLocalMapWithLines (src/Tracking.cc) on the
// device: UpdateLocalKeyFrames[WithLines] (:5399-5551 / :5553-5745) and UpdateLocalPoints[AndLines]
// (:5325-5352 / :5354-5397) for every frame of a batch, plus the gathers that turn the two lists
// into the input tables of plvi_frustum_points_batch / plvi_frustum_lines_batch.  Integers only:
// the outputs equal the reference's lists entry for entry.
//
// One batch is two fills and four launches, all on the caller's stream:
//   lm_keyframes_kernel  one workgroup per frame.  The vote (:5405-5421) as a histogram over the
//                        keyframe slots, in LDS up to PLVI_LOCAL_MAP_LDS_KF slots and in global
//                        scratch above; bad voting entries written back as -1; the frame's seen-set
//                        as a bitmap over the pool.  K1 (:5456-5471) is an ordered block-scan
//                        compaction of d_kf_order, pKFmax the first position of the largest count.
//                        The expansion (:5474-5524) and the temporal walk (:5527-5544) are short
//                        and sequential: thread 0 runs them against the listed-bitmap.
//   lm_first_kernel      several workgroups per frame and feature kind: the mark pass of the
//                        first-occurrence walk (first_walk.h) in its multi-workgroup form, over
//                        the keyframes in reverse order (:5331), the table filled with 0x7f (the
//                        mnTrackReferenceForFrame stamp of :5342 / :5348).
//   lm_count_kernel      each workgroup owns a contiguous range of positions and counts the
//                        entries that hold their id's minimum.
//   lm_write_kernel      the same ranges again: the workgroup's base is the sum of the counts
//                        before it, a block scan orders the kept entries inside it, and each kept
//                        entry writes its list cell and gathers its rows (map_pool.h).
// Points and lines keep separate lists and separate stamps, so the per-keyframe interleaving of
// :5382-5395 cannot be seen in the outputs; the two kinds run as blockIdx.z = 0 / 1.
#include <climits>
#include <cstring>

#include "first_walk.h"
#include "map_pool.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kLdsKf = PLVI_LOCAL_MAP_LDS_KF;
constexpr int kKfThreads = 512, kKfWaves = kKfThreads / kWave;
constexpr int kListThreads = 256, kListWaves = kListThreads / kWave;
constexpr int kPerGroup = PLVI_LOCAL_MAP_GROUP_ENTRIES;
constexpr int kMaxGroups = PLVI_LOCAL_MAP_MAX_GROUPS;
constexpr int kNeighbours = PLVI_KFDB_NEIGHBOURS;
// the byte fill of the first-occurrence tables: above every position (PLVI_LOCAL_MAP_MAX_ENTRIES)
constexpr int kFirstNone = 0x7f7f7f7f;
static_assert(PLVI_LOCAL_MAP_MAX_ENTRIES <= kFirstNone, "a position must stay below the table's fill");

// one feature kind: 0 = MapPoints, 1 = MapLines
struct LmSide {
    int on, n, kcap, vote_cap, seen_cap, out_cap, seen_words, err_bit;
    const int *kf_tab, *kf_n;
    const uint8_t* bad;
    const int *obs_off, *obs_kf;
    const float* pos;
    const double* sep;
    const float *normal, *dist;
    const uint8_t* desc;
    int* vote;
    const int *n_vote, *seen, *n_seen;
    int* first;           // scratch [B][n]
    unsigned* seen_bits;  // scratch [B][seen_words]
    int* cnt;             // scratch [B][G]
    int *list, *n_list;
    float* o_pos;
    double* o_sep;
    float *o_normal, *o_dist;
    uint8_t *o_flags, *o_desc;
};

struct LmArgs {
    int B, kf_cap, n_order, lkf_cap, G, with_lines;
    const uint8_t* kf_bad;
    const int *order, *covis, *child_off, *child, *parent, *prev_kf, *last_kf;
    int *kfl, *nlk;      // scratch: the whole local keyframe list [B][kf_cap] and its length [B]
    int* hist_g;         // scratch [B][kf_cap], kf_cap > kLdsKf only
    unsigned* listed_g;  // scratch [B][ceil(kf_cap / 32)], likewise
    int *local_kf, *n_local_kf, *ref_kf, *err;
    LmSide s[2];
};

__device__ __forceinline__ bool is_listed(const unsigned* listed, int s) { return listed[s >> 5] >> (s & 31) & 1u; }

__global__ __launch_bounds__(kKfThreads) void lm_keyframes_kernel(LmArgs a) {
    __shared__ int s_hist[kLdsKf];
    __shared__ unsigned s_listed[kLdsKf / 32];
    __shared__ int s_wave[kKfWaves];
    __shared__ int s_max, s_pos, s_n;
    const int tid = threadIdx.x, f = blockIdx.x;
    const int K = a.kf_cap, lw = (K + 31) / 32;
    const bool in_lds = K <= kLdsKf;
    int* hist = in_lds ? s_hist : a.hist_g + (size_t)f * K;
    unsigned* listed = in_lds ? s_listed : a.listed_g + (size_t)f * lw;
    if (in_lds) {  // the global tables were cleared by the fill before the launch
        for (int i = tid; i < K; i += kKfThreads) s_hist[i] = 0;
        for (int i = tid; i < lw; i += kKfThreads) s_listed[i] = 0;
    }
    if (tid == 0) {
        s_max = 0;
        s_pos = INT_MAX;
    }
    __syncthreads();

    // The vote: every voting feature that is not bad adds 1 to each keyframe of its observation
    // list (:5405-5421; points and lines into the one counter, :5559-5592); a bad one is written
    // back as NULL (:5418 / :5442, :5589 / :5632).
    for (int k = 0; k < 2; ++k) {
        const LmSide& S = a.s[k];
        if (!S.on) continue;
        unsigned* bits = S.seen_bits + (size_t)f * S.seen_words;
        if (S.vote && (k == 0 || a.with_lines)) {
            int* vote = S.vote + (size_t)f * S.vote_cap;
            const int nv = clampi(S.n_vote[f], 0, S.vote_cap);
            for (int i = tid; i < nv; i += kKfThreads) {
                const int id = vote[i];
                if ((unsigned)id >= (unsigned)S.n) continue;
                if (S.bad[id]) {
                    vote[i] = -1;
                    continue;
                }
                if (!S.seen) atomicOr(bits + (id >> 5), 1u << (id & 31));
                vote_observations(hist, K, S.obs_off, S.obs_kf, id);
            }
        }
        // the current frame's own table where it is not the voting one (the IMU branch votes with
        // mLastFrame, :5425); a bad entry is not seen -- it is NULL by the time the search runs
        if (S.seen) {
            const int* seen = S.seen + (size_t)f * S.seen_cap;
            const int ns = clampi(S.n_seen[f], 0, S.seen_cap);
            for (int i = tid; i < ns; i += kKfThreads) {
                const int id = seen[i];
                if ((unsigned)id < (unsigned)S.n && !S.bad[id]) atomicOr(bits + (id >> 5), 1u << (id & 31));
            }
        }
    }
    __syncthreads();

    // K1 (:5456-5471): the counted keyframes in map order, the bad ones skipped; unbounded.
    int* kfl = a.kfl + (size_t)f * K;
    int n = 0;
    for (int i0 = 0; i0 < a.n_order; i0 += kKfThreads) {
        const int i = i0 + tid;
        const int slot = i < a.n_order ? a.order[i] : -1;
        int c = 0;
        bool flag = (unsigned)slot < (unsigned)K && (c = hist[slot]) > 0 && !a.kf_bad[slot];
        if (flag) {  // a slot named twice is listed once
            const unsigned bit = 1u << (slot & 31);
            flag = !(atomicOr(listed + (slot >> 5), bit) & bit);
        }
        int tot;
        const int pos = block_scan<kKfWaves>(flag, s_wave, tid, &tot);
        if (flag) {
            kfl[n + pos] = slot;
            atomicMax(&s_max, c);
        }
        n += tot;
    }
    __syncthreads();
    // pKFmax (:5463-5467): `it->second > max` with max starting at 0 keeps the first keyframe, in
    // map order, of the largest count
    const int vmax = s_max;
    if (vmax > 0)
        for (int i = tid; i < a.n_order; i += kKfThreads) {
            const int slot = a.order[i];
            if ((unsigned)slot < (unsigned)K && hist[slot] == vmax && !a.kf_bad[slot]) atomicMin(&s_pos, i);
        }
    __syncthreads();

    if (tid == 0) {
        auto add = [&](int s) {
            kfl[n++] = s;
            listed[s >> 5] |= 1u << (s & 31);
        };
        // The expansion (:5474-5524).  itEndKF is taken before the loop and the reserve of :5453
        // keeps it valid: the K1 members only, while the list holds at most 80.
        const int n1 = n;
        for (int k = 0; k < n1; ++k) {
            if (n > 80) break;  // :5477, size() > 80
            const int kf = kfl[k];
            if (a.covis)
                for (int c = 0; c < kNeighbours; ++c) {  // :5485-5497
                    const int nb = a.covis[(size_t)kf * kNeighbours + c];
                    if (nb < 0) break;
                    if (nb >= K || a.kf_bad[nb] || is_listed(listed, nb)) continue;
                    add(nb);
                    break;
                }
            if (a.child_off) {  // :5499-5512, std::set order
                const int c1 = a.child_off[kf + 1];
                for (int c = a.child_off[kf]; c < c1; ++c) {
                    const int ch = a.child[c];
                    if ((unsigned)ch >= (unsigned)K || a.kf_bad[ch] || is_listed(listed, ch)) continue;
                    add(ch);
                    break;
                }
            }
            const int p = a.parent ? a.parent[kf] : -1;  // :5514-5523: no isBad(), and the break leaves the outer loop
            if ((unsigned)p < (unsigned)K && !is_listed(listed, p)) {
                add(p);
                break;
            }
        }
        // The temporal walk (:5527-5544): at most 20 rounds; it moves on only after an insertion, so
        // a listed keyframe ends it in effect.
        if (a.last_kf && a.prev_kf && n < 80) {
            int t = a.last_kf[f];
            for (int i = 0; i < 20; ++i) {
                if ((unsigned)t >= (unsigned)K || is_listed(listed, t)) break;
                add(t);
                t = a.prev_kf[t];
            }
        }
        s_n = n;
        a.nlk[f] = n;
        a.n_local_kf[f] = n;
        a.ref_kf[f] = s_pos < INT_MAX ? a.order[s_pos] : -1;  // :5546
        a.err[f] = n > a.lkf_cap ? PLVI_LOCAL_MAP_ERR_KF : 0;
    }
    __syncthreads();
    const int nw = min(s_n, a.lkf_cap);
    for (int i = tid; i < nw; i += kKfThreads) a.local_kf[(size_t)f * a.lkf_cap + i] = kfl[i];
}

// the pool id at traversal position p of frame f, or -1: keyframes in reverse list order (:5331),
// each keyframe's table in index order; NULL and bad entries dropped (:5340, :5344)
__device__ __forceinline__ int entry_id(const LmSide& S, const int* kfl, int nlk, int p) {
    const int r = p / S.kcap, i = p - r * S.kcap;
    return KfTable{S.kf_tab, S.kf_n, S.kcap, S.n, S.bad}.at(kfl[nlk - 1 - r], i);
}

// position p is an occurrence of id: keep the smallest
__device__ __forceinline__ void record_first(const LmSide& S, int f, int id, int p) {
    atomicMin(S.first + (size_t)f * S.n + id, p);
}

__device__ __forceinline__ bool is_first(const LmSide& S, int f, int id, int p) {
    return S.first[(size_t)f * S.n + id] == p;
}

__global__ __launch_bounds__(kListThreads) void lm_first_kernel(LmArgs a) {
    const LmSide& S = a.s[blockIdx.z];
    const int f = blockIdx.y;
    if (!S.on || S.kcap <= 0) return;
    const int nlk = a.nlk[f];
    const int* kfl = a.kfl + (size_t)f * a.kf_cap;
    const int total = nlk * S.kcap;  // kf_cap * kcap <= PLVI_LOCAL_MAP_MAX_ENTRIES is checked on the host
    for (long long p = (long long)blockIdx.x * kListThreads + threadIdx.x; p < total;
         p += (long long)a.G * kListThreads) {
        const int id = entry_id(S, kfl, nlk, (int)p);
        if (id >= 0) record_first(S, f, id, (int)p);
    }
}

// workgroup b owns the positions [b * chunk, (b + 1) * chunk)
__device__ __forceinline__ void group_range(int total, int G, int b, int* p0, int* p1) {
    const int chunk = (int)(((long long)total + G - 1) / G);
    const long long lo = (long long)b * chunk, hi = lo + chunk;
    *p0 = (int)min(lo, (long long)total);
    *p1 = (int)min(hi, (long long)total);
}

__global__ __launch_bounds__(kListThreads) void lm_count_kernel(LmArgs a) {
    __shared__ int s_cnt;
    const LmSide& S = a.s[blockIdx.z];
    const int f = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    if (!S.on) return;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int c = 0;
    if (S.kcap > 0) {
        const int nlk = a.nlk[f];
        const int* kfl = a.kfl + (size_t)f * a.kf_cap;
        int p0, p1;
        group_range(nlk * S.kcap, a.G, b, &p0, &p1);
        for (int p = p0 + tid; p < p1; p += kListThreads) {
            const int id = entry_id(S, kfl, nlk, p);
            c += id >= 0 && is_first(S, f, id, p);
        }
    }
    block_add(c, &s_cnt, tid);
    __syncthreads();
    if (tid == 0) S.cnt[(size_t)f * a.G + b] = s_cnt;
}

__global__ __launch_bounds__(kListThreads) void lm_write_kernel(LmArgs a) {
    __shared__ int s_wave[kListWaves];
    __shared__ int s_id[kListThreads], s_out[kListThreads];
    const LmSide& S = a.s[blockIdx.z];
    const int f = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
    if (!S.on) return;
    // the kept entries of the workgroups before this one, and of all of them
    int before = 0, all = 0;
    for (int g = tid; g < a.G; g += kListThreads) {
        const int c = S.cnt[(size_t)f * a.G + g];
        all += c;
        if (g < b) before += c;
    }
    int tot;
    (void)block_scan<kListWaves>(before, s_wave, tid, &tot);
    const int base = tot;
    (void)block_scan<kListWaves>(all, s_wave, tid, &tot);
    if (b == 0 && tid == 0) {
        S.n_list[f] = tot;  // the full length, also above the capacity
        if (tot > S.out_cap) atomicOr(a.err + f, S.err_bit);
    }
    if (S.kcap <= 0) return;
    const int nlk = a.nlk[f];
    const int* kfl = a.kfl + (size_t)f * a.kf_cap;
    const unsigned* bits = S.seen_bits + (size_t)f * S.seen_words;
    const size_t row0 = (size_t)f * S.out_cap;
    const PoolGather g{S.pos, S.sep, S.normal, S.dist, S.desc, S.o_pos, S.o_sep, S.o_normal, S.o_dist, S.o_desc};
    int p0, p1;
    group_range(nlk * S.kcap, a.G, b, &p0, &p1);
    int run = base;
    for (int q0 = p0; q0 < p1; q0 += kListThreads) {
        const int p = q0 + tid;
        int id = -1;
        if (p < p1) {
            id = entry_id(S, kfl, nlk, p);
            if (id >= 0 && !is_first(S, f, id, p)) id = -1;  // listed earlier in the walk (:5342)
        }
        const int pos = block_scan<kListWaves>(id >= 0, s_wave, tid, &tot);
        const int out = run + pos;
        const bool wr = id >= 0 && out < S.out_cap;  // rows past the capacity are never written
        if (id >= 0) {
            s_id[pos] = wr ? id : -1;
            s_out[pos] = out;
        }
        if (wr) {
            const size_t o = row0 + out;
            S.list[o] = id;
            if (S.o_flags) {
                // bit0: mnLastFrameSeen != mnId (:5052-5069 / :5126-5161 stamp the frame's own
                // features); bit1: Observations() > 0
                const int unseen = !(bits[id >> 5] >> (id & 31) & 1u);
                const int obs = S.obs_off[id + 1] > S.obs_off[id];
                S.o_flags[o] = (uint8_t)(unseen | obs << 1);
            }
            g.rows(o, (size_t)id);
        }
        __syncthreads();
        g.descriptors<kListThreads>(tot, tid, [&](int e, size_t* at) {
            *at = row0 + s_out[e];
            return s_id[e];
        });
        run += tot;
        // the next round's block_scan synchronises before s_id / s_out are written again
    }
}

// the scratch block: [first tables | cleared tables | uncleared tables]
struct LmLayout {
    size_t first[2], first_bytes;                  // filled with 0x7f
    size_t seen[2], hist, listed, zero_bytes;      // filled with 0, offsets from the zero block
    size_t kfl, nlk, cnt[2], total;
    int seen_words[2];
};

static LmLayout lm_layout(int B, int kf_cap, int mp_n, int ml_n) {
    LmLayout L;
    const size_t b = (size_t)B;
    const int n[2] = {mp_n, ml_n};
    size_t o = 0;
    for (int k = 0; k < 2; ++k) {
        L.first[k] = o;
        o += up256(4 * b * n[k]);
    }
    L.first_bytes = o;
    const size_t z0 = o;
    for (int k = 0; k < 2; ++k) {
        L.seen_words[k] = (n[k] + 31) / 32;
        L.seen[k] = o;
        o += up256(4 * b * L.seen_words[k]);
    }
    L.hist = o;
    L.listed = o;
    if (kf_cap > kLdsKf) {
        o += up256(4 * b * kf_cap);
        L.listed = o;
        o += up256(4 * b * ((kf_cap + 31) / 32));
    }
    L.zero_bytes = o - z0;
    L.kfl = o;
    o += up256(4 * b * kf_cap);
    L.nlk = o;
    o += up256(4 * b);
    for (int k = 0; k < 2; ++k) {
        L.cnt[k] = o;
        o += up256(4 * b * kMaxGroups);
    }
    L.total = o;
    return L;
}

}  // namespace plvi

using namespace plvi;

extern "C" size_t plvi_local_map_scratch_bytes(int n_frames, int kf_cap, int mp_n, int ml_n) {
    if (n_frames < 0 || kf_cap < 0 || mp_n < 0 || ml_n < 0) return 0;
    return lm_layout(n_frames, kf_cap, mp_n, ml_n).total;
}

// The argument checks of both forms, made before any table is read (the host form reads
// child_off[kf_cap] and obs_off[n] itself): which pointers are NULL means the same in both.
static int lm_validate(int n_frames, const plvi_local_map_keyframes* kf, const plvi_local_map_pool* mp,
                       const plvi_local_map_pool* ml, const plvi_local_map_frames* fr,
                       const plvi_local_map_outputs* out) {
    if (n_frames < 0 || !kf || !mp || !fr || !out) return PLVI_E_BADARG;
    if (kf->kf_cap < 0 || kf->n_order < 0 || kf->kp_cap < 0 || kf->kl_cap < 0 || fr->vote_mp_cap < 0 ||
        fr->vote_ml_cap < 0 || fr->seen_mp_cap < 0 || fr->seen_ml_cap < 0 || out->lkf_cap < 0 || out->lmp_cap < 0 ||
        out->lml_cap < 0 || !pool_ok(mp) || (ml && !pool_ok(ml)))
        return PLVI_E_BADARG;
    if (n_frames == 0) return PLVI_OK;
    const bool with_lines = kf->ml != nullptr;  // NULL selects UpdateLocalKeyFrames / UpdateLocalPoints
    if (with_lines && (!ml || !kf->nml)) return PLVI_E_BADARG;
    const int K = kf->kf_cap;
    if ((K > 0 && !kf->bad) || (kf->n_order > 0 && !kf->order) || (kf->kp_cap > 0 && K > 0 && (!kf->mp || !kf->nmp)) ||
        (kf->child_off == nullptr) != (kf->child == nullptr))
        return PLVI_E_BADARG;
    if (!out->n_local_kf || !out->ref_kf || !out->err || !out->n_local_mp || (out->lkf_cap > 0 && !out->local_kf) ||
        (out->lmp_cap > 0 && !out->local_mp) || (with_lines && (!out->n_local_ml || (out->lml_cap > 0 && !out->local_ml))))
        return PLVI_E_BADARG;
    if ((fr->vote_mp && !fr->n_vote_mp) || (fr->vote_ml && !fr->n_vote_ml) || (fr->seen_mp && !fr->n_seen_mp) ||
        (fr->seen_ml && !fr->n_seen_ml))
        return PLVI_E_BADARG;
    // a gather needs its source row
    if ((out->mp_pos && !mp->pos) || (out->mp_normal && !mp->normal) || (out->mp_dist && !mp->dist) ||
        (out->mp_desc && !mp->desc))
        return PLVI_E_BADARG;
    if (with_lines && ((out->ml_sep && !ml->sep) || (out->ml_normal && !ml->normal) || (out->ml_dist && !ml->dist) ||
                       (out->ml_desc && !ml->desc)))
        return PLVI_E_BADARG;
    const int kbig = with_lines && kf->kl_cap > kf->kp_cap ? kf->kl_cap : kf->kp_cap;
    if (n_frames > 65535 || (long long)K * kbig > PLVI_LOCAL_MAP_MAX_ENTRIES) return PLVI_E_CAPACITY;
    return PLVI_OK;
}

extern "C" int plvi_local_map_batch(int n_frames, const plvi_local_map_keyframes* kf, const plvi_local_map_pool* mp,
                                    const plvi_local_map_pool* ml, const plvi_local_map_frames* fr,
                                    const plvi_local_map_outputs* out, void* d_scratch, size_t scratch_bytes,
                                    void* stream) {
    if (int rc = lm_validate(n_frames, kf, mp, ml, fr, out)) return rc;
    if (n_frames == 0) return PLVI_OK;
    const bool with_lines = kf->ml != nullptr;
    const int K = kf->kf_cap;
    const int kbig = with_lines && kf->kl_cap > kf->kp_cap ? kf->kl_cap : kf->kp_cap;
    const int ml_n = with_lines ? ml->n : 0;
    const LmLayout L = lm_layout(n_frames, K, mp->n, ml_n);
    if (!d_scratch || scratch_bytes < L.total) return PLVI_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    if (L.first_bytes) PLVI_CHECK(hipMemsetAsync(base, 0x7f, L.first_bytes, st));
    if (L.zero_bytes) PLVI_CHECK(hipMemsetAsync(base + L.first_bytes, 0, L.zero_bytes, st));

    LmArgs a;
    memset(&a, 0, sizeof a);
    a.B = n_frames;
    a.kf_cap = K;
    a.n_order = kf->n_order;
    a.lkf_cap = out->lkf_cap;
    a.with_lines = with_lines;
    const long long entries = (long long)K * kbig;
    a.G = (int)((entries + kPerGroup - 1) / kPerGroup);
    a.G = a.G < 1 ? 1 : a.G > kMaxGroups ? kMaxGroups : a.G;
    a.kf_bad = kf->bad;
    a.order = kf->order;
    a.covis = kf->covis;
    a.child_off = kf->child_off;
    a.child = kf->child;
    a.parent = kf->parent;
    a.prev_kf = kf->prev_kf;
    a.last_kf = fr->last_kf;
    a.kfl = reinterpret_cast<int*>(base + L.kfl);
    a.nlk = reinterpret_cast<int*>(base + L.nlk);
    a.hist_g = reinterpret_cast<int*>(base + L.hist);
    a.listed_g = reinterpret_cast<unsigned*>(base + L.listed);
    a.local_kf = out->local_kf;
    a.n_local_kf = out->n_local_kf;
    a.ref_kf = out->ref_kf;
    a.err = out->err;
    for (int k = 0; k < 2; ++k) {
        LmSide& S = a.s[k];
        const plvi_local_map_pool* p = k ? ml : mp;
        S.on = k == 0 || with_lines;
        if (!S.on) continue;
        S.n = p->n;
        S.kcap = k ? kf->kl_cap : kf->kp_cap;
        S.kf_tab = k ? kf->ml : kf->mp;
        S.kf_n = k ? kf->nml : kf->nmp;
        S.bad = p->bad;
        S.obs_off = p->obs_off;
        S.obs_kf = p->obs_kf;
        S.pos = p->pos;
        S.sep = p->sep;
        S.normal = p->normal;
        S.dist = p->dist;
        S.desc = p->desc;
        S.vote = k ? fr->vote_ml : fr->vote_mp;
        S.n_vote = k ? fr->n_vote_ml : fr->n_vote_mp;
        S.vote_cap = k ? fr->vote_ml_cap : fr->vote_mp_cap;
        S.seen = k ? fr->seen_ml : fr->seen_mp;
        S.n_seen = k ? fr->n_seen_ml : fr->n_seen_mp;
        S.seen_cap = k ? fr->seen_ml_cap : fr->seen_mp_cap;
        S.out_cap = k ? out->lml_cap : out->lmp_cap;
        S.err_bit = k ? PLVI_LOCAL_MAP_ERR_ML : PLVI_LOCAL_MAP_ERR_MP;
        S.seen_words = L.seen_words[k];
        S.first = reinterpret_cast<int*>(base + L.first[k]);
        S.seen_bits = reinterpret_cast<unsigned*>(base + L.seen[k]);
        S.cnt = reinterpret_cast<int*>(base + L.cnt[k]);
        S.list = k ? out->local_ml : out->local_mp;
        S.n_list = k ? out->n_local_ml : out->n_local_mp;
        S.o_pos = k ? nullptr : out->mp_pos;
        S.o_sep = k ? out->ml_sep : nullptr;
        S.o_normal = k ? out->ml_normal : out->mp_normal;
        S.o_dist = k ? out->ml_dist : out->mp_dist;
        S.o_flags = k ? out->ml_in_flags : out->mp_in_flags;
        S.o_desc = k ? out->ml_desc : out->mp_desc;
    }
    hipLaunchKernelGGL(lm_keyframes_kernel, dim3(n_frames), dim3(kKfThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    const dim3 grid(a.G, n_frames, with_lines ? 2 : 1);
    hipLaunchKernelGGL(lm_first_kernel, grid, dim3(kListThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lm_count_kernel, grid, dim3(kListThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lm_write_kernel, grid, dim3(kListThreads), 0, st, a);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

// One frame from host memory.  Every pointer of the four structs is a host pointer here.
extern "C" int plvi_local_map(const plvi_local_map_keyframes* kf, const plvi_local_map_pool* mp,
                              const plvi_local_map_pool* ml, const plvi_local_map_frames* fr,
                              const plvi_local_map_outputs* out) {
    if (int rc = lm_validate(1, kf, mp, ml, fr, out)) return rc;
    const bool with_lines = kf->ml != nullptr;
    const size_t K = (size_t)kf->kf_cap;
    const size_t n_child = kf->child_off && K && kf->child_off[K] > 0 ? (size_t)kf->child_off[K] : 0;
    // copies of the caller's structs: commit() turns their host pointers into device pointers
    plvi_local_map_keyframes dk = *kf;
    plvi_local_map_pool dmp = *mp, dml = ml ? *ml : plvi_local_map_pool{};
    plvi_local_map_frames df = *fr;
    plvi_local_map_outputs dout = *out;
    HostStage hs;
    const HostStage::Dir In = HostStage::In, InOut = HostStage::InOut, Out = HostStage::Out;
    hs.field(dk.bad, In, K);
    hs.field(dk.order, In, kf->n_order);
    hs.field(dk.covis, In, K, PLVI_KFDB_NEIGHBOURS);
    hs.field(dk.child_off, In, K + 1);
    hs.field(dk.child, In, n_child);
    hs.field(dk.parent, In, K);
    hs.field(dk.prev_kf, In, K);
    hs.field(dk.mp, In, K, kf->kp_cap);
    hs.field(dk.nmp, In, K);
    hs.field(dk.ml, In, K, kf->kl_cap);
    hs.field(dk.nml, In, K);
    stage_pool(hs, dmp, kPoolPoints);
    if (ml) stage_pool(hs, dml, kPoolLines);
    hs.field(df.vote_mp, InOut, fr->vote_mp_cap);  // the vote tables are in/out
    hs.field(df.n_vote_mp, In, 1);
    hs.field(df.vote_ml, InOut, fr->vote_ml_cap);
    hs.field(df.n_vote_ml, In, 1);
    hs.field(df.seen_mp, In, fr->seen_mp_cap);
    hs.field(df.n_seen_mp, In, 1);
    hs.field(df.seen_ml, In, fr->seen_ml_cap);
    hs.field(df.n_seen_ml, In, 1);
    hs.field(df.last_kf, In, 1);
    const size_t ckf = (size_t)out->lkf_cap, cmp = (size_t)out->lmp_cap, cml = (size_t)out->lml_cap;
    const auto lkf = hs.field(dout.local_kf, Out, ckf);
    const auto nkf = hs.field(dout.n_local_kf, Out, 1);
    const auto lmp = hs.field(dout.local_mp, Out, cmp);
    const auto nmp = hs.field(dout.n_local_mp, Out, 1);
    const auto lml = hs.field(dout.local_ml, Out, cml);
    const auto nml = hs.field(dout.n_local_ml, Out, 1);
    const auto ppos = hs.field(dout.mp_pos, Out, cmp, 3);
    const auto pnor = hs.field(dout.mp_normal, Out, cmp, 3);
    const auto pdis = hs.field(dout.mp_dist, Out, cmp, 2);
    const auto pfl = hs.field(dout.mp_in_flags, Out, cmp);
    const auto pde = hs.field(dout.mp_desc, Out, cmp, 32);
    const auto lsep = hs.field(dout.ml_sep, Out, cml, 6);
    const auto lnor = hs.field(dout.ml_normal, Out, cml, 3);
    const auto ldis = hs.field(dout.ml_dist, Out, cml, 2);
    const auto lfl = hs.field(dout.ml_in_flags, Out, cml);
    const auto lde = hs.field(dout.ml_desc, Out, cml, 32);
    hs.field(dout.ref_kf, Out, 1);
    const auto err = hs.field(dout.err, Out, 1);
    const size_t sb = plvi_local_map_scratch_bytes(1, kf->kf_cap, mp->n, ml ? ml->n : 0);
    const auto scr = hs.scratch<uint8_t>(sb);
    if (int rc = hs.commit()) return rc;
    if (int rc = plvi_local_map_batch(1, &dk, &dmp, ml ? &dml : nullptr, &df, &dout, hs.dev(scr), sb, nullptr))
        return rc;
    // counts first: list and gathered rows come back up to min(count, capacity);
    // n_local_ml is not written without lines
    if (!with_lines) hs.trim(nml, 0);
    for (const Staged<int> count : {nkf, nmp, nml, err})
        if (int rc = hs.fetch_one(count)) return rc;
    const size_t wkf = (size_t)std::min(*out->n_local_kf, out->lkf_cap);
    const size_t wmp = (size_t)std::min(*out->n_local_mp, out->lmp_cap);
    const size_t wml = with_lines ? (size_t)std::min(*out->n_local_ml, out->lml_cap) : 0;
    hs.trim(lkf, wkf);
    hs.trim(lmp, wmp);
    hs.trim(ppos, wmp, 3);
    hs.trim(pnor, wmp, 3);
    hs.trim(pdis, wmp, 2);
    hs.trim(pfl, wmp);
    hs.trim(pde, wmp, 32);
    hs.trim(lml, wml);
    hs.trim(lsep, wml, 6);
    hs.trim(lnor, wml, 3);
    hs.trim(ldis, wml, 2);
    hs.trim(lfl, wml);
    hs.trim(lde, wml, 32);
    if (int rc = hs.fetch()) return rc;
    return *out->err ? PLVI_E_CAPACITY : PLVI_OK;
}
