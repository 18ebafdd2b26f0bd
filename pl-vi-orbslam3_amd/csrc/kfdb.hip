// kfdb.hip — KeyFrameDatabase (src/KeyFrameDatabase.cc) on the device: add / erase / clearMap /
// clear (:46-105) and the two detectors the reference calls, DetectRelocalizationCandidates
// (:790-902, Tracking.cc:5752) and DetectNBestCandidates (:619-787, LoopClosing.cc:660).
//
// There is no inverted file.  A keyframe lives in a caller-chosen slot whose BowVector is kept
// forward (words ascending, values double, word_cap per slot) with a map id, an add sequence
// number and the two float score members that persist between queries.  The order of the
// reference's lKFsSharingWords -- query words ascending, each word's std::list in insertion
// order, a keyframe entering at its first hit -- is the order by (smallest word shared with the
// query, add sequence), which the forward tables give directly.
//
// One query batch is five launches, all on the caller's stream:
//   kfdb_connected_kernel  mode 1: marks the (query, slot) pairs of GetConnectedKeyFrames()
//   kfdb_count_kernel      |common words| and the first common word of every (query, slot): the
//                          query's words staged in LDS, a wave per slot, its lanes striding the
//                          slot's words (coalesced) and binary-searching the LDS copy; the
//                          per-query maxCommonWords by atomicMax
//   kfdb_score_kernel      L1Scoring::score of the pairs above the threshold only; the terms of
//                          64 slot words are computed in parallel and added strictly in ascending
//                          word order (a uniform loop over the ballot, one v_readlane pair per
//                          common word), so the double sum is the reference's bit for bit
//   kfdb_carry_kernel      a lane per slot walks the queries in order: a scored pair takes its
//                          new float score, an unscored one the member's latest earlier value
//                          (the stale member the accumulation reads), and the member is written
//                          back -- a batch equals its queries run one by one
//   kfdb_select_kernel     one workgroup per query: bitonic sort of the sharing list by
//                          (first word, sequence), stable compaction of the scored entries, the
//                          covisibility accumulation (a thread per entry), and the selection:
//                          mode 0 the 0.75 * bestAccScore / map / first-pBestKF filter in list
//                          order, mode 1 a stable descending sort by accScore and the first
//                          n_best unseen pBestKF of the query's map (loop) and of other, not bad,
//                          maps (merge).
#include <climits>
#include <cstring>
#include <vector>

#include "block_prims.h"
#include "host_stage.h"
#include "plvi_common.h"

namespace plvi {

typedef unsigned long long u64;

constexpr int kNeigh = PLVI_KFDB_NEIGHBOURS;
constexpr int kCountThreads = 256, kCountWaves = kCountThreads / kWave;
constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / kWave;
constexpr int kSortLds = 8192;   // longest sharing list sorted in LDS (12 bytes an entry); longer ones use global scratch
constexpr int kChunk = 64;       // slots per add / erase launch (passed by value as kernel arguments)
#ifndef PLVI_KFDB_SLOTS_PER_GROUP
#define PLVI_KFDB_SLOTS_PER_GROUP 0  // A/B knob: 0 = chosen from the launch size
#endif
#ifndef PLVI_KFDB_SINGLE_PASS
#define PLVI_KFDB_SINGLE_PASS 0      // A/B knob: 1 = score every sharing pair, no count pass first
#endif
#ifndef PLVI_KFDB_LANE_PER_SLOT
#define PLVI_KFDB_LANE_PER_SLOT 0    // A/B knob: 1 = the count pass gives every lane a slot of its own
#endif
#ifndef PLVI_KFDB_LANE0_SUM
#define PLVI_KFDB_LANE0_SUM 0        // A/B knob: 1 = the common words' terms are compacted into LDS and summed by lane 0
#endif
// 12 bytes of LDS per query word in the score kernel (double value + word id)
static_assert((size_t)PLVI_KFDB_MAX_WORDS * 12 + 1024 <= 160 * 1024, "the staged query must fit the CU's LDS");

struct ChunkArgs {
    int n;
    int row[kChunk], slot[kChunk], map[kChunk];
    unsigned seq[kChunk];
};

// minCommonWords = maxCommonWords * 0.8f (KeyFrameDatabase.cc:673 / :826): int -> float, one
// float multiply, truncation
__device__ __forceinline__ int min_common(int maxc) { return (int)((float)maxc * 0.8f); }

// number of entries of the ascending sq[0 .. nq) below w; top = the largest power of two <= nq
__device__ __forceinline__ int lower_bound_lds(const unsigned* sq, int nq, int top, unsigned w) {
    int lo = 0;
    for (int st = top; st; st >>= 1)
        if (lo + st <= nq && sq[lo + st - 1] < w) lo += st;
    return lo;
}

__global__ __launch_bounds__(256) void kfdb_add_kernel(ChunkArgs a, int slot_cap, int word_cap, unsigned n_words,
                                                       const unsigned* __restrict__ src_word,
                                                       const double* __restrict__ src_value,
                                                       const int* __restrict__ src_n, int cap, unsigned* kf_word,
                                                       double* kf_value, int* kf_n, int* kf_map, unsigned* kf_seq,
                                                       float* place_score, float* reloc_score, int* err) {
    const int e = blockIdx.x;
    if (e >= a.n) return;
    const int slot = a.slot[e], row = a.row[e];
    if ((unsigned)slot >= (unsigned)slot_cap) return;
    const int raw = src_n[row];
    const int n = clampi(raw, 0, min(cap, word_cap));
    const unsigned* sw = src_word + (size_t)row * cap;
    const double* sv = src_value + (size_t)row * cap;
    bool bad_word = false;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned w = sw[i];
        bad_word |= w >= n_words;
        kf_word[(size_t)slot * word_cap + i] = w;
        kf_value[(size_t)slot * word_cap + i] = sv[i];
    }
    if (bad_word) atomicOr(err, 2);
    if (threadIdx.x == 0) {
        if (raw > word_cap) atomicOr(err, 1);
        kf_n[slot] = n;
        kf_map[slot] = a.map[e];
        kf_seq[slot] = a.seq[e];
        place_score[slot] = 0.f;
        reloc_score[slot] = 0.f;
    }
}

__global__ void kfdb_erase_kernel(ChunkArgs a, int slot_cap, int* kf_n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < a.n && (unsigned)a.slot[e] < (unsigned)slot_cap) kf_n[a.slot[e]] = 0;
}

// all != 0: every slot, else the slots of map_id
__global__ void kfdb_clear_kernel(int slot_cap, int all, int map_id, const int* __restrict__ kf_map, int* kf_n) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < slot_cap && (all || kf_map[s] == map_id)) kf_n[s] = 0;
}

__global__ void kfdb_connected_kernel(int n_queries, int slot_cap, const int* __restrict__ conn_off,
                                      const int* __restrict__ conn_slot, int* cnt) {
    const int q = blockIdx.y;
    const int o0 = conn_off[q], len = max(conn_off[q + 1] - o0, 0);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < len; i += gridDim.x * blockDim.x) {
        const int s = conn_slot[(size_t)o0 + i];
        if ((unsigned)s < (unsigned)slot_cap) cnt[(size_t)q * slot_cap + s] = -2;
    }
}

// The terms of one slot against the staged query, added in ascending word order.  All lanes of
// the wave call this with the same slot; every lane returns the same sum.  (Keeping 4 or 8
// chunks of 64 words in flight per wave measured the same as this one-chunk loop: DESIGN.md
// section 19.)
__device__ __forceinline__ double ordered_score(const unsigned* sq, const double* sv, int nq, int top,
                                                const unsigned* __restrict__ kw, const double* __restrict__ kv,
                                                int ns, int lane) {
    double score = 0;
    for (int base = 0; base < ns; base += kWave) {
        const int i = base + lane;
        bool found = false;
        double term = 0;
        if (i < ns) {
            const unsigned w = kw[i];
            const int lo = lower_bound_lds(sq, nq, top, w);
            found = lo < nq && sq[lo] == w;
            if (found) {
                const double vi = sv[lo], wi = kv[i];
                term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);  // ScoringObject.cpp:41
            }
        }
        u64 mask = __ballot(found);
#if PLVI_KFDB_LANE0_SUM
        __shared__ double sterm[kCountWaves][kWave];
        double* st = sterm[threadIdx.x / kWave];
        if (found) st[__popcll(mask & ((1ull << lane) - 1))] = term;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (lane == 0)
            for (int k = 0, n = __popcll(mask); k < n; ++k) score += st[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#else
        // the mask is wave-uniform: a scalar loop of s_ff1, two v_readlane and one v_add_f64 per common word
        const int thi = __double2hiint(term), tlo = __double2loint(term);
        while (mask) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            score += __hiloint2double(__builtin_amdgcn_readlane(thi, b), __builtin_amdgcn_readlane(tlo, b));
        }
#endif
    }
#if PLVI_KFDB_LANE0_SUM
    score = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(score)),
                             __builtin_amdgcn_readfirstlane(__double2loint(score)));
#endif
    return -score * 0.5;  // ScoringObject.cpp:65
}

// grid (ceil(slot_cap / spb), n_queries).  cnt [q][slot]: -2 on entry marks a connected keyframe;
// on exit |common words| >= 1, or -1 where the slot is not in lKFsSharingWords.
template <bool kSingle>
__global__ __launch_bounds__(kCountThreads) void kfdb_count_kernel(
    int slot_cap, int word_cap, int spb, const unsigned* __restrict__ kf_word, const double* __restrict__ kf_value,
    const int* __restrict__ kf_n, const unsigned* __restrict__ q_word, const double* __restrict__ q_value,
    const int* __restrict__ q_n, int q_cap, int* cnt, unsigned* first, int* maxc, double* d_score, float* fsc) {
    extern __shared__ __align__(16) unsigned char lds[];
    double* sv = reinterpret_cast<double*>(lds);                                          // [q_cap], kSingle only
    unsigned* sq = reinterpret_cast<unsigned*>(lds + (kSingle ? (size_t)8 * q_cap : 0));  // [q_cap]
    __shared__ int smax;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int q = blockIdx.y;
    const int nq = clampi(q_n[q], 0, q_cap);
    for (int i = tid; i < nq; i += kCountThreads) {
        sq[i] = q_word[(size_t)q * q_cap + i];
        if (kSingle) sv[i] = q_value[(size_t)q * q_cap + i];
    }
    if (tid == 0) smax = 0;
    __syncthreads();
    int top = 0;
    if (nq > 0) top = 1 << (31 - __clz(nq));
    const int s_end = min((blockIdx.x + 1) * spb, slot_cap);
    int wmax = 0;
#if PLVI_KFDB_LANE_PER_SLOT
    for (int s = blockIdx.x * spb + tid; s < s_end; s += kCountThreads) {
        const size_t idx = (size_t)q * slot_cap + s;
        const int ns = clampi(kf_n[s], 0, word_cap);
        int c = 0;
        unsigned f = 0xffffffffu;
        if (nq > 0 && cnt[idx] != -2) {
            const unsigned* kw = kf_word + (size_t)s * word_cap;
            for (int i = 0; i < ns; ++i) {
                const unsigned w = kw[i];
                const int lo = lower_bound_lds(sq, nq, top, w);
                if (lo < nq && sq[lo] == w) {
                    ++c;
                    f = min(f, w);
                }
            }
        }
        if (c == 0) c = -1;
        cnt[idx] = c;
        first[idx] = f;
        wmax = max(wmax, c);
    }
    if (wmax > 0) atomicMax(&smax, wmax);
    __syncthreads();
    if (tid == 0 && smax > 0) atomicMax(maxc + q, smax);
    return;
#endif
    for (int s = blockIdx.x * spb + wv; s < s_end; s += kCountWaves) {
        const size_t idx = (size_t)q * slot_cap + s;
        const int ns = clampi(kf_n[s], 0, word_cap);
        int c = 0;
        unsigned f = 0xffffffffu;
        if (ns > 0 && nq > 0 && cnt[idx] != -2) {
            const unsigned* kw = kf_word + (size_t)s * word_cap;
            for (int i = lane; i < ns; i += kWave) {
                const unsigned w = kw[i];
                const int lo = lower_bound_lds(sq, nq, top, w);
                if (lo < nq && sq[lo] == w) {
                    ++c;
                    f = min(f, w);
                }
            }
            c = wave_sum(c);
#pragma unroll
            for (int m = kWave / 2; m >= 1; m >>= 1) f = min(f, (unsigned)__shfl_xor((int)f, m, kWave));
            if (kSingle && c > 0) {
                const double sc = ordered_score(sq, sv, nq, top, kw, kf_value + (size_t)s * word_cap, ns, lane);
                // the A/B build scores every sharing pair (d_score is the handle's scratch here); the
                // carry kernel applies the threshold
                if (lane == 0) fsc[idx] = (float)sc;
                if (lane == 0 && d_score) d_score[idx] = sc;
            }
        }
        if (c == 0) c = -1;
        if (lane == 0) {
            cnt[idx] = c;
            first[idx] = f;
        }
        wmax = max(wmax, c);
    }
    if (lane == 0 && wmax > 0) atomicMax(&smax, wmax);
    __syncthreads();
    if (tid == 0 && smax > 0) atomicMax(maxc + q, smax);
}

// Same grid.  Scores the pairs with cnt > minCommonWords: d_score (double, nullable) and fsc
// (the float the reference stores into the score member).
__global__ __launch_bounds__(kCountThreads) void kfdb_score_kernel(
    int slot_cap, int word_cap, int spb, const unsigned* __restrict__ kf_word, const double* __restrict__ kf_value,
    const int* __restrict__ kf_n, const unsigned* __restrict__ q_word, const double* __restrict__ q_value,
    const int* __restrict__ q_n, int q_cap, const int* __restrict__ cnt, const int* __restrict__ maxc,
    double* d_score, float* fsc) {
    extern __shared__ __align__(16) unsigned char lds[];
    double* sv = reinterpret_cast<double*>(lds);                         // [q_cap]
    unsigned* sq = reinterpret_cast<unsigned*>(lds + (size_t)8 * q_cap);  // [q_cap]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int q = blockIdx.y;
    const int minc = min_common(maxc[q]);
    const int s0 = blockIdx.x * spb, s_end = min(s0 + spb, slot_cap);
    // most workgroups hold no pair above the threshold and leave before staging anything
    int any = 0;
    for (int s = s0 + tid; s < s_end; s += kCountThreads) any |= cnt[(size_t)q * slot_cap + s] > minc;
    if (!__syncthreads_or(any)) return;
    const int nq = clampi(q_n[q], 0, q_cap);
    for (int i = tid; i < nq; i += kCountThreads) {
        sq[i] = q_word[(size_t)q * q_cap + i];
        sv[i] = q_value[(size_t)q * q_cap + i];
    }
    __syncthreads();
    int top = 0;
    if (nq > 0) top = 1 << (31 - __clz(nq));
    for (int s = s0 + wv; s < s_end; s += kCountWaves) {
        const size_t idx = (size_t)q * slot_cap + s;
        if (cnt[idx] <= minc) continue;
        const int ns = clampi(kf_n[s], 0, word_cap);
        const double sc = ordered_score(sq, sv, nq, top, kf_word + (size_t)s * word_cap,
                                        kf_value + (size_t)s * word_cap, ns, lane);
        if (lane == 0) {
            if (d_score) d_score[idx] = sc;
            fsc[idx] = (float)sc;
        }
    }
}

// A lane per slot, the queries in order.  fsc [q][slot] becomes the value of the slot's score
// member as query q's accumulation reads it; the member keeps the last write.
__global__ void kfdb_carry_kernel(int n_queries, int slot_cap, const int* __restrict__ cnt,
                                  const int* __restrict__ maxc, float* fsc, float* member,
                                  const double* __restrict__ all_score, double* d_score) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slot_cap) return;
    float m = member[s];
    for (int q = 0; q < n_queries; ++q) {
        const size_t idx = (size_t)q * slot_cap + s;
        if (cnt[idx] > min_common(maxc[q])) {
            m = fsc[idx];
            if (all_score && d_score) d_score[idx] = all_score[idx];  // PLVI_KFDB_SINGLE_PASS only
        } else {
            fsc[idx] = m;
        }
    }
    member[s] = m;
}

struct SelectArgs {
    int slot_cap, sort_cap, mode, n_best, cand_cap, n_maps;
    const int* cnt;
    const unsigned* first;
    const float* fsc;
    const int* maxc;
    const unsigned* kf_seq;
    const int* kf_map;
    const int* q_map;
    const int* covis;
    const uint8_t* map_bad;
    int *ord, *norder, *ent_best, *mark;
    float* ent_acc;
    u64* g_key;  // [q][sort_cap] when sort_cap > kSortLds
    int* g_val;
    int *cand, *ncand, *loop, *nloop, *merge, *nmerge;
};

__global__ __launch_bounds__(kSelThreads) void kfdb_select_kernel(SelectArgs a) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int s_wave[kSelWaves];
    __shared__ int s_len, s_best;
    const int tid = threadIdx.x, q = blockIdx.x;
    const int S = a.slot_cap;
    const size_t qo = (size_t)q * S;
    const bool in_lds = a.sort_cap <= kSortLds;
    u64* key = in_lds ? reinterpret_cast<u64*>(lds) : a.g_key + (size_t)q * a.sort_cap;
    int* val = in_lds ? reinterpret_cast<int*>(lds + (size_t)8 * a.sort_cap) : a.g_val + (size_t)q * a.sort_cap;
    const int* cnt = a.cnt + qo;
    const float* fsc = a.fsc + qo;
    int* ord = a.ord + qo;
    int* ent_best = a.ent_best + qo;
    float* ent_acc = a.ent_acc + qo;
    int* mark = a.mark + qo;
    const int minc = min_common(a.maxc[q]);
    const int qmap = a.q_map[q];

    // lKFsSharingWords: the slots with a common word, by (first common word, add sequence)
    if (tid == 0) {
        s_len = 0;
        s_best = 0;
    }
    __syncthreads();
    for (int s = tid; s < S; s += kSelThreads)
        if (cnt[s] >= 1) {
            const int p = atomicAdd(&s_len, 1);
            key[p] = (u64)a.first[qo + s] << 32 | a.kf_seq[s];
            val[p] = s;
        }
    __syncthreads();
    const int L = s_len;
    const int P = pow2_at_least(L, 1);
    for (int i = L + tid; i < P; i += kSelThreads) {
        key[i] = ~0ull;
        val[i] = -1;
    }
    __syncthreads();
    bitonic_sort<kSelThreads>(key, val, P, tid);
    for (int i = tid; i < L; i += kSelThreads) ord[i] = val[i];
    if (tid == 0 && a.norder) a.norder[q] = L;
    __syncthreads();

    // lScoreAndMatch: the entries above the threshold, in list order (val[0 .. n_sc))
    int n_sc = 0;
    for (int i0 = 0; i0 < L; i0 += kSelThreads) {
        const int i = i0 + tid;
        const int s = i < L ? ord[i] : -1;
        const int flag = s >= 0 && cnt[s] > minc;
        int tot;
        const int pos = block_scan<kSelWaves>(flag, s_wave, tid, &tot);
        if (flag) val[n_sc + pos] = s;
        n_sc += tot;
    }
    __syncthreads();

    // lAccScoreAndMatch (KeyFrameDatabase.cc:700-725 / :853-878)
    for (int j = tid; j < n_sc; j += kSelThreads) {
        const int s = val[j];
        float best_score = fsc[s], acc = best_score;
        int best = s;
        if (a.covis)
            for (int k = 0; k < kNeigh; ++k) {
                const int nb = a.covis[(size_t)s * kNeigh + k];
                if (nb < 0) break;
                if (nb >= S || cnt[nb] < 1) continue;  // the stamp is not this query's
                const float sc = fsc[nb];
                acc += sc;
                if (sc > best_score) {
                    best = nb;
                    best_score = sc;
                }
            }
        ent_acc[j] = acc;
        ent_best[j] = best;
        mark[best] = INT_MAX;
        if (acc > 0.f) atomicMax(&s_best, __float_as_int(acc));  // bestAccScore starts at 0: positive floats order as ints
    }
    __syncthreads();
    const float min_retain = 0.75f * __int_as_float(s_best);

    // the processing order: mode 0 the list order, mode 1 list::sort(compFirst) -- stable, descending
    if (a.mode == 1) {
        const int P2 = pow2_at_least(n_sc, 1);
        for (int j = tid; j < P2; j += kSelThreads) {
            u64 k = ~0ull;
            if (j < n_sc) {
                float acc = ent_acc[j];
                if (acc == 0.f) acc = 0.f;  // -0 and +0 compare equal
                const unsigned b = (unsigned)__float_as_int(acc);
                const unsigned asc = b & 0x80000000u ? ~b : b | 0x80000000u;
                k = (u64)(~asc) << 32 | (unsigned)j;
            }
            key[j] = k;
        }
        __syncthreads();
        bitonic_sort<kSelThreads>(key, P2, tid);
    }

    // the first entry of every pBestKF among those that pass
    for (int jp = tid; jp < n_sc; jp += kSelThreads) {
        const int j = a.mode == 1 ? (int)(key[jp] & 0xffffffffu) : jp;
        const int best = ent_best[j];
        const bool pass = a.mode == 1 || (ent_acc[j] > min_retain && a.kf_map[best] == qmap);
        if (pass) atomicMin(mark + best, jp);
    }
    __syncthreads();
    int n0 = 0, n1 = 0;
    for (int j0 = 0; j0 < n_sc; j0 += kSelThreads) {
        const int jp = j0 + tid;
        int flag = 0, best = -1;
        if (jp < n_sc) {
            const int j = a.mode == 1 ? (int)(key[jp] & 0xffffffffu) : jp;
            best = ent_best[j];
            const int m = a.kf_map[best];
            if (a.mode == 1) {
                if (mark[best] == jp) {
                    if (m == qmap) flag = 1;
                    else if (!(a.map_bad && (unsigned)m < (unsigned)a.n_maps && a.map_bad[m])) flag = 1 << 16;
                }
            } else {
                flag = ent_acc[j] > min_retain && m == qmap && mark[best] == jp;
            }
        }
        int tot;
        const int pos = block_scan<kSelWaves>(flag, s_wave, tid, &tot);
        const int p0 = n0 + (pos & 0xffff), p1 = n1 + (pos >> 16);
        if (a.mode == 1) {
            if ((flag & 1) && p0 < a.n_best) a.loop[(size_t)q * a.n_best + p0] = best;
            if ((flag >> 16) && p1 < a.n_best) a.merge[(size_t)q * a.n_best + p1] = best;
        } else if (flag && p0 < a.cand_cap) {
            a.cand[(size_t)q * a.cand_cap + p0] = best;
        }
        n0 += tot & 0xffff;
        n1 += tot >> 16;
    }
    if (tid == 0) {
        if (a.mode == 1) {
            a.nloop[q] = min(n0, a.n_best);
            a.nmerge[q] = min(n1, a.n_best);
        } else {
            a.ncand[q] = n0;
        }
    }
}

}  // namespace plvi

using namespace plvi;

struct plvi_kf_database {
    int n_words = 0, slot_cap = 0, word_cap = 0, device = 0;
    unsigned next_seq = 0;
    std::vector<uint8_t> occupied;  // host mirror: add to an occupied slot is refused before any launch
    std::vector<int> map;
    DevBuf word, value, n, dmap, seq, place, reloc, err;
    // per-query scratch, grown to the largest batch seen
    int q_alloc = 0, sort_cap = 0;
    DevBuf cnt, first, fsc, ord, ent_acc, ent_best, mark, maxc, norder, g_key, g_val, all_score;

    int grow(int n_queries) {
        if (n_queries <= q_alloc) return PLVI_OK;
        const size_t cells = (size_t)n_queries * slot_cap;
        DevBuf* four[] = {&cnt, &first, &fsc, &ord, &ent_acc, &ent_best, &mark};
        for (DevBuf* b : four) {
            if (b->p) (void)hipFree(b->p);  // waits for the work that still uses it
            b->p = nullptr;
            if (b->alloc(4 * cells)) return PLVI_E_HIP;
        }
        DevBuf* perq[] = {&maxc, &norder};
        for (DevBuf* b : perq) {
            if (b->p) (void)hipFree(b->p);
            b->p = nullptr;
            if (b->alloc(4 * (size_t)n_queries)) return PLVI_E_HIP;
        }
        if (PLVI_KFDB_SINGLE_PASS) {
            if (all_score.p) (void)hipFree(all_score.p);
            all_score.p = nullptr;
            if (all_score.alloc(8 * cells)) return PLVI_E_HIP;
        }
        if (sort_cap > kSortLds) {
            if (g_key.p) (void)hipFree(g_key.p);
            if (g_val.p) (void)hipFree(g_val.p);
            g_key.p = g_val.p = nullptr;
            if (g_key.alloc(8 * (size_t)n_queries * sort_cap) || g_val.alloc(4 * (size_t)n_queries * sort_cap))
                return PLVI_E_HIP;
        }
        q_alloc = n_queries;
        return PLVI_OK;
    }
};

extern "C" int plvi_kfdb_create(int n_words, int slot_cap, int word_cap, int scoring, int device,
                                plvi_kf_database** out) {
    if (!out) return PLVI_E_BADARG;
    *out = nullptr;
    // ScoringType L1_NORM = 0 (BowVector.h); the other five are refused
    if (scoring != 0 || n_words < 0 || slot_cap < 1 || word_cap < 1) return PLVI_E_BADARG;
    if (word_cap > PLVI_KFDB_MAX_WORDS || slot_cap > (1 << 24)) return PLVI_E_CAPACITY;
    PLVI_CHECK(hipSetDevice(device));
    plvi_kf_database* h = new plvi_kf_database;
    h->n_words = n_words;
    h->slot_cap = slot_cap;
    h->word_cap = word_cap;
    h->device = device;
    h->occupied.assign(slot_cap, 0);
    h->map.assign(slot_cap, 0);
    h->sort_cap = pow2_at_least(slot_cap, 1);
    const size_t cells = (size_t)slot_cap * word_cap;
    if (h->word.alloc(4 * cells) || h->value.alloc(8 * cells) || h->n.alloc(4 * (size_t)slot_cap) ||
        h->dmap.alloc(4 * (size_t)slot_cap) || h->seq.alloc(4 * (size_t)slot_cap) ||
        h->place.alloc(4 * (size_t)slot_cap) || h->reloc.alloc(4 * (size_t)slot_cap) || h->err.alloc(4)) {
        delete h;
        return PLVI_E_HIP;
    }
    DevBuf* zero[] = {&h->n, &h->dmap, &h->seq, &h->place, &h->reloc, &h->err};
    for (DevBuf* b : zero)
        if (hipMemset(b->p, 0, b->bytes) != hipSuccess) {
            delete h;
            return PLVI_E_HIP;
        }
    *out = h;
    return PLVI_OK;
}

extern "C" int plvi_kfdb_destroy(plvi_kf_database* h) {
    if (!h) return PLVI_E_BADARG;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return PLVI_OK;
}

extern "C" int plvi_kfdb_add_batch(plvi_kf_database* h, int n, const int* entries, const unsigned* d_bow_word,
                                   const double* d_bow_value, const int* d_bow_n, int cap, void* stream) {
    if (!h || n < 0 || cap < 0) return PLVI_E_BADARG;
    if (n == 0) return PLVI_OK;
    if (!entries || !d_bow_n || (cap > 0 && (!d_bow_word || !d_bow_value))) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    // every entry is checked before anything changes
    for (int i = 0; i < n; ++i) {
        const int row = entries[3 * (size_t)i], slot = entries[3 * (size_t)i + 1];
        if (row < 0 || slot < 0 || slot >= h->slot_cap || h->occupied[slot]) {
            for (int j = 0; j < i; ++j) h->occupied[entries[3 * (size_t)j + 1]] = 0;  // take the marks back
            return PLVI_E_BADARG;
        }
        h->occupied[slot] = 2;  // marked: a second entry naming the slot is refused like an occupied one
    }
    if ((unsigned long long)h->next_seq + (unsigned)n > 0xffffffffull) {
        for (int i = 0; i < n; ++i) h->occupied[entries[3 * (size_t)i + 1]] = 0;
        return PLVI_E_OVERFLOW;
    }
    hipStream_t st = (hipStream_t)stream;
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        ChunkArgs a;
        memset(&a, 0, sizeof a);
        a.n = n - i0 < kChunk ? n - i0 : kChunk;
        for (int e = 0; e < a.n; ++e) {
            const int* en = entries + 3 * (size_t)(i0 + e);
            a.row[e] = en[0];
            a.slot[e] = en[1];
            a.map[e] = en[2];
            a.seq[e] = h->next_seq++;
            h->occupied[en[1]] = 1;
            h->map[en[1]] = en[2];
        }
        hipLaunchKernelGGL(kfdb_add_kernel, dim3(a.n), dim3(256), 0, st, a, h->slot_cap, h->word_cap,
                           (unsigned)h->n_words, d_bow_word, d_bow_value, d_bow_n, cap, h->word.as<unsigned>(),
                           h->value.as<double>(), h->n.as<int>(), h->dmap.as<int>(), h->seq.as<unsigned>(),
                           h->place.as<float>(), h->reloc.as<float>(), h->err.as<int>());
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

extern "C" int plvi_kfdb_erase(plvi_kf_database* h, int n, const int* slots, void* stream) {
    if (!h || n < 0) return PLVI_E_BADARG;
    if (n == 0) return PLVI_OK;
    if (!slots) return PLVI_E_BADARG;
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= h->slot_cap) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    for (int i0 = 0; i0 < n; i0 += kChunk) {
        ChunkArgs a;
        memset(&a, 0, sizeof a);
        a.n = n - i0 < kChunk ? n - i0 : kChunk;
        for (int e = 0; e < a.n; ++e) {
            a.slot[e] = slots[i0 + e];
            h->occupied[slots[i0 + e]] = 0;
        }
        hipLaunchKernelGGL(kfdb_erase_kernel, dim3(1), dim3(kChunk), 0, (hipStream_t)stream, a, h->slot_cap,
                           h->n.as<int>());
        PLVI_CHECK(hipGetLastError());
    }
    return PLVI_OK;
}

static int clear_slots(plvi_kf_database* h, int all, int map_id, void* stream) {
    PLVI_CHECK(hipSetDevice(h->device));
    for (int s = 0; s < h->slot_cap; ++s)
        if (all || h->map[s] == map_id) h->occupied[s] = 0;
    hipLaunchKernelGGL(kfdb_clear_kernel, dim3((h->slot_cap + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       h->slot_cap, all, map_id, h->dmap.as<int>(), h->n.as<int>());
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_kfdb_clear_map(plvi_kf_database* h, int map_id, void* stream) {
    if (!h) return PLVI_E_BADARG;
    return clear_slots(h, 0, map_id, stream);
}

extern "C" int plvi_kfdb_clear(plvi_kf_database* h, void* stream) {
    if (!h) return PLVI_E_BADARG;
    if (int rc = clear_slots(h, 1, 0, stream)) return rc;
    h->next_seq = 0;  // no slot is left to compare an old number with
    return PLVI_OK;
}

extern "C" int plvi_kfdb_errors(plvi_kf_database* h, int* flags, void* stream) {
    if (!h) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    int e = 0;
    PLVI_CHECK(hipMemcpyAsync(&e, h->err.p, 4, hipMemcpyDeviceToHost, st));
    PLVI_CHECK(hipMemsetAsync(h->err.p, 0, 4, st));
    PLVI_CHECK(hipStreamSynchronize(st));
    if (flags) *flags = e;
    return e ? PLVI_E_OVERFLOW : PLVI_OK;
}

extern "C" int plvi_kfdb_add(plvi_kf_database* h, int slot, int map_id, const unsigned* word, const double* value,
                             int n) {
    if (!h || n < 0 || (n > 0 && (!word || !value))) return PLVI_E_BADARG;
    if (slot < 0 || slot >= h->slot_cap || h->occupied[slot]) return PLVI_E_BADARG;
    PLVI_CHECK(hipSetDevice(h->device));
    HostStage hs;
    const auto W = hs.in_or_zero(word, n);
    const auto V = hs.in_or_zero(value, n);
    const auto N = hs.in(&n, 1);
    if (int rc = hs.commit()) return rc;
    const int entry[3] = {0, slot, map_id};
    if (int rc = plvi_kfdb_add_batch(h, 1, entry, hs.dev(W), hs.dev(V), hs.dev(N), n > 0 ? n : 1, nullptr)) return rc;
    return plvi_kfdb_errors(h, nullptr, nullptr);
}

extern "C" int plvi_kfdb_query_batch(plvi_kf_database* h, int n_queries, const unsigned* d_q_word,
                                     const double* d_q_value, const int* d_q_n, int q_cap, const int* d_q_map,
                                     int mode, int n_best, const int* d_conn_off, const int* d_conn_slot,
                                     const int* d_covis, const uint8_t* d_map_bad, int n_maps, int* d_words,
                                     double* d_score, int* d_order, int* d_norder, int* d_cand, int cand_cap,
                                     int* d_ncand, int* d_loop, int* d_nloop, int* d_merge, int* d_nmerge,
                                     void* stream) {
    if (!h || n_queries < 0 || q_cap < 0 || (mode != 0 && mode != 1) || n_maps < 0) return PLVI_E_BADARG;
    if (n_queries == 0) return PLVI_OK;
    if (!d_q_n || !d_q_map || (q_cap > 0 && (!d_q_word || !d_q_value))) return PLVI_E_BADARG;
    if (mode == 0 && (cand_cap < 0 || !d_ncand || (cand_cap > 0 && !d_cand))) return PLVI_E_BADARG;
    if (mode == 1 && (n_best < 0 || n_best > 0xffff || !d_nloop || !d_nmerge || (n_best > 0 && (!d_loop || !d_merge))))
        return PLVI_E_BADARG;
    if ((d_conn_off == nullptr) != (d_conn_slot == nullptr)) return PLVI_E_BADARG;
    if (q_cap > PLVI_KFDB_MAX_WORDS || (long long)n_queries * h->slot_cap > INT_MAX || n_queries > 65535)
        return PLVI_E_CAPACITY;
    PLVI_CHECK(hipSetDevice(h->device));
    if (int rc = h->grow(n_queries)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int S = h->slot_cap;
    const size_t cells = (size_t)n_queries * S;
    int* cnt = d_words ? d_words : h->cnt.as<int>();
    int* ord = d_order ? d_order : h->ord.as<int>();
    float* member = mode == 1 ? h->place.as<float>() : h->reloc.as<float>();

    PLVI_CHECK(hipMemsetAsync(cnt, 0, 4 * cells, st));
    PLVI_CHECK(hipMemsetAsync(h->maxc.p, 0, 4 * (size_t)n_queries, st));
    if (mode == 1 && d_conn_off) {
        hipLaunchKernelGGL(kfdb_connected_kernel, dim3(4, n_queries), dim3(256), 0, st, n_queries, S, d_conn_off,
                           d_conn_slot, cnt);
        PLVI_CHECK(hipGetLastError());
    }
    // slots per workgroup: enough workgroups to fill the device, few enough to amortise the staging
    int spb = PLVI_KFDB_SLOTS_PER_GROUP;
    if (spb <= 0) {
        const long long per = (long long)S * n_queries / 2048;
        spb = per < kCountWaves ? kCountWaves : per > 64 ? 64 : (int)per;
    }
    if (PLVI_KFDB_LANE_PER_SLOT) spb = 64;  // a lane per slot: one wave's worth of slots per workgroup
    const dim3 grid((S + spb - 1) / spb, n_queries);
    const size_t lds_count = (size_t)4 * q_cap + 16, lds_score = (size_t)12 * q_cap + 16;
    // (the static_assert on PLVI_KFDB_MAX_WORDS keeps the staged query within what launch_lds accepts)
    if (PLVI_KFDB_SINGLE_PASS) {
        if (int rc = launch_lds<kfdb_count_kernel<true>>(
                grid, dim3(kCountThreads), lds_score, st, S, h->word_cap, spb, h->word.as<unsigned>(),
                h->value.as<double>(), h->n.as<int>(), d_q_word, d_q_value, d_q_n, q_cap, cnt, h->first.as<unsigned>(),
                h->maxc.as<int>(), h->all_score.as<double>(), h->fsc.as<float>()))
            return rc;
    } else {
        if (int rc = launch_lds<kfdb_count_kernel<false>>(
                grid, dim3(kCountThreads), lds_count, st, S, h->word_cap, spb, h->word.as<unsigned>(),
                h->value.as<double>(), h->n.as<int>(), d_q_word, d_q_value, d_q_n, q_cap, cnt, h->first.as<unsigned>(),
                h->maxc.as<int>(), d_score, h->fsc.as<float>()))
            return rc;
        if (int rc = launch_lds<kfdb_score_kernel>(grid, dim3(kCountThreads), lds_score, st, S, h->word_cap, spb,
                                                   h->word.as<unsigned>(), h->value.as<double>(), h->n.as<int>(),
                                                   d_q_word, d_q_value, d_q_n, q_cap, cnt, h->maxc.as<int>(), d_score,
                                                   h->fsc.as<float>()))
            return rc;
    }
    hipLaunchKernelGGL(kfdb_carry_kernel, dim3((S + 255) / 256), dim3(256), 0, st, n_queries, S, cnt,
                       h->maxc.as<int>(), h->fsc.as<float>(), member,
                       PLVI_KFDB_SINGLE_PASS ? h->all_score.as<double>() : nullptr, d_score);
    PLVI_CHECK(hipGetLastError());

    SelectArgs a;
    a.slot_cap = S;
    a.sort_cap = h->sort_cap;
    a.mode = mode;
    a.n_best = n_best;
    a.cand_cap = cand_cap;
    a.n_maps = n_maps;
    a.cnt = cnt;
    a.first = h->first.as<unsigned>();
    a.fsc = h->fsc.as<float>();
    a.maxc = h->maxc.as<int>();
    a.kf_seq = h->seq.as<unsigned>();
    a.kf_map = h->dmap.as<int>();
    a.q_map = d_q_map;
    a.covis = d_covis;
    a.map_bad = d_map_bad;
    a.ord = ord;
    a.norder = d_norder;
    a.ent_best = h->ent_best.as<int>();
    a.mark = h->mark.as<int>();
    a.ent_acc = h->ent_acc.as<float>();
    a.g_key = h->g_key.as<u64>();
    a.g_val = h->g_val.as<int>();
    a.cand = d_cand;
    a.ncand = d_ncand;
    a.loop = d_loop;
    a.nloop = d_nloop;
    a.merge = d_merge;
    a.nmerge = d_nmerge;
    const size_t lds_sel = h->sort_cap <= kSortLds ? (size_t)12 * h->sort_cap : 16;
    return launch_lds<kfdb_select_kernel>(dim3(n_queries), dim3(kSelThreads), lds_sel, st, a);
}

extern "C" int plvi_kfdb_query(plvi_kf_database* h, const unsigned* q_word, const double* q_value, int q_n, int q_map,
                               int mode, int n_best, const int* conn, int n_conn, const int* covis,
                               const uint8_t* map_bad, int n_maps, int* cand, int cand_cap, int* loop, int* n_loop,
                               int* merge, int* n_merge) {
    if (!h || q_n < 0 || n_conn < 0 || n_maps < 0 || (mode != 0 && mode != 1)) return PLVI_E_BADARG;
    if ((q_n > 0 && (!q_word || !q_value)) || (n_conn > 0 && !conn)) return PLVI_E_BADARG;
    if (mode == 0 && (cand_cap < 0 || (cand_cap > 0 && !cand))) return PLVI_E_BADARG;
    if (mode == 1 && (n_best < 0 || !n_loop || !n_merge || (n_best > 0 && (!loop || !merge)))) return PLVI_E_BADARG;
    if (q_n > PLVI_KFDB_MAX_WORDS) return PLVI_E_CAPACITY;
    PLVI_CHECK(hipSetDevice(h->device));
    const int q_cap = q_n > 0 ? q_n : 1, nb = n_best > 0 ? n_best : 1, cc = cand_cap > 0 ? cand_cap : 1;
    // q_n, q_map, conn_off[2]; then the counts that come back: ncand, nloop, nmerge
    int c[7] = {q_n, q_map, 0, n_conn, 0, 0, 0};
    HostStage hs;
    const auto W = hs.in_or_zero(q_word, q_n);
    const auto V = hs.in_or_zero(q_value, q_n);
    const auto Bad = hs.in(map_bad, n_maps);
    const auto Conn = hs.in_or_zero(conn, n_conn), Cov = hs.in(covis, h->slot_cap, kNeigh), C = hs.inout(c, 7);
    const auto Cand = hs.out_or_scratch(mode == 0 ? cand : nullptr, cc);
    const auto Loop = hs.out_or_scratch(mode == 1 ? loop : nullptr, nb);
    const auto Merge = hs.out_or_scratch(mode == 1 ? merge : nullptr, nb);
    if (int rc = hs.commit()) return rc;
    int* dC = hs.dev(C);
    if (int rc = plvi_kfdb_query_batch(h, 1, hs.dev(W), hs.dev(V), dC, q_cap, dC + 1, mode, n_best, dC + 2,
                                       hs.dev(Conn), hs.dev(Cov), hs.dev(Bad), n_maps, nullptr, nullptr, nullptr,
                                       nullptr, hs.dev(Cand), cand_cap, dC + 4, hs.dev(Loop), dC + 5, hs.dev(Merge),
                                       dC + 6, nullptr))
        return rc;
    // counts first: the lists come back up to them
    if (int rc = hs.fetch_one(C)) return rc;
    hs.trim(Cand, std::min(c[4], cand_cap));
    hs.trim(Loop, c[5]);
    hs.trim(Merge, c[6]);
    if (int rc = hs.fetch()) return rc;
    if (mode == 0) return c[4];
    *n_loop = c[5];
    *n_merge = c[6];
    return c[5] + c[6];
}
