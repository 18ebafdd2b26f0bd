// distinctive.hip — MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:330-404) and
// MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:264-331) as one batched search
// over a pool of descriptor rows and a CSR observation list: per feature the all-pairs
// ORBmatcher::DescriptorDistance of its N rows, per row the element floor((N-1)/2) of its
// sorted distances (self-distance 0 included), and the first row with the smallest such
// median.  Integers only.  The observation maps, isBad(), the mutexes and the write of
// mDescriptor stay with the caller.
//
// Two regimes, chosen per feature by its clamped list length:
//   <= 64 entries (almost every feature: a keyframe's points have 2-30 observations):
//     distinctive_small_kernel<S>.  A segment of S lanes serves one feature, S = the power
//     of two >= min(max_obs, 64), at least 8, so 64 / S features share a wave.  Lane i owns
//     row i in 8 VGPRs, row j is read back from a 2 KB per-wave LDS image at a
//     segment-uniform address, and the S distances stay in registers (the loop over j is
//     unrolled; an absent j holds a sentinel above 256).  The k-th smallest is a 9-step
//     binary search on the value with a count per step -- no sort --, and the argmin a
//     segment-wide minimum of (median << 6 | position).
//   > 64 entries: distinctive_large_kernel.  ceil(max_obs / 32) workgroups per feature each
//     stage the list's rows in LDS once; a wave takes four rows i at a time, its lanes stride
//     over j, and every distance is computed once and counted into a per-(wave, row)
//     257-bin LDS histogram (N*N values are not stored: 1448^2 do not fit), which a
//     wave-wide prefix sum turns into the k-th smallest.  Each wave's minimum of
//     (median << 11 | position) goes into best_pos[f] by atomicMin (preset to 0x7f7f7f7f by a
//     memset node), and the small kernel, which runs after it on the stream, decodes it.
//     Splitting a long list over workgroups is what keeps one N = 1448 feature (N*N work)
//     from holding up a launch of N = 10 features; workgroups of short features exit at
//     once.  The large kernel and the memset are only launched when max_obs > 64.
#include <climits>
#include <cstring>
#include <vector>

#include "block_prims.h"
#include "host_stage.h"
#include "plvi_common.h"

namespace plvi {

constexpr int kSmallMax = 64;                             // longest list of the small path
constexpr int kLargeThreads = 256, kLargeWaves = kLargeThreads / kWave;
constexpr int kLargeRows = 4;                             // rows i a wave serves per pass over j
constexpr int kHistPitch = 260;                           // 257 bins, padded to a multiple of 4
constexpr int kHistDump = 257;                            // a padding bin: counts of ignored entries, never read
#ifndef PLVI_DISTINCTIVE_ROWS_PER_GROUP
#define PLVI_DISTINCTIVE_ROWS_PER_GROUP 32  // A/B knob (tools/build_variant.sh); DESIGN.md section 18
#endif
constexpr int kLargeRowsPerGroup = PLVI_DISTINCTIVE_ROWS_PER_GROUP;  // a long list gets ceil(max_obs / this) workgroups
constexpr int kPosBits = 11;                              // position field of the large path's key
constexpr int kKeyNone = 0x7f7f7f7f;                      // the memset pattern: above every key
static_assert(PLVI_DISTINCTIVE_MAX_OBS <= (1 << kPosBits), "the position must fit the key");
static_assert((256 << kPosBits | ((1 << kPosBits) - 1)) < kKeyNone, "every key is below the preset");

__device__ __forceinline__ int list_length(const int* __restrict__ obs_off, int f, int max_obs) {
    return max(min(obs_off[f + 1] - obs_off[f], max_obs), 0);
}

template <int S>
__global__ __launch_bounds__(256) void distinctive_small_kernel(
    int n_feat, const uint8_t* __restrict__ pool, int pool_rows, const int* __restrict__ obs_off,
    const int* __restrict__ obs_row, int max_obs, int* __restrict__ best_pos, int* __restrict__ best_median,
    uint8_t* __restrict__ out_desc) {
    __shared__ uint4 sdesc[256 / kWave][kWave][2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int sl = lane & (S - 1), segbase = lane - sl;
    const long long fl = ((long long)blockIdx.x * (256 / kWave) + wv) * (kWave / S) + lane / S;
    const bool live = fl < n_feat;
    const int f = live ? (int)fl : 0;
    const int o0 = live ? obs_off[f] : 0;
    const int len = live ? list_length(obs_off, f, max_obs) : 0;
    const bool large = len > kSmallMax;  // served by distinctive_large_kernel, decoded below
    int row = -1;
    if (!large && sl < len) row = obs_row[(size_t)o0 + sl];
    const bool valid = (unsigned)row < (unsigned)pool_rows;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (valid) {
        const uint4* pr = reinterpret_cast<const uint4*>(pool + (size_t)row * 32);
        a0 = pr[0];
        a1 = pr[1];
    }
    sdesc[wv][lane][0] = a0;
    sdesc[wv][lane][1] = a1;
    const unsigned long long ball = __ballot(valid);
    const unsigned long long segmask = S == 64 ? ball : (ball >> segbase) & ((1ull << (S & 63)) - 1);
    const int N = __popcll(segmask), k = (N - 1) >> 1;  // vDists[0.5*(N-1)]
    // the wave's own LDS writes, read back by the same wave: no workgroup barrier
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    int d[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
        const uint4 b0 = sdesc[wv][segbase + j][0], b1 = sdesc[wv][segbase + j][1];
        d[j] = (segmask >> j) & 1 ? hamming256(a0, a1, b0, b1) : 512;
    }
    // the smallest v in [0, 256] with #{j : d[j] <= v} > k is the k-th smallest (0-based)
    int lo = 0, hi = 256;
#pragma unroll 1
    for (int step = 0; step < 9; ++step) {
        const int mid = (lo + hi) >> 1;
        int c = 0;
#pragma unroll
        for (int j = 0; j < S; ++j) c += d[j] <= mid;
        if (c > k) hi = mid;
        else lo = mid + 1;
    }
    // first wins: the minimum of (median, position) over the segment
    int key = valid ? (lo << 6 | sl) : INT_MAX;
#pragma unroll
    for (int m = S / 2; m >= 1; m >>= 1) key = min(key, __shfl_xor(key, m, kWave));
    if (!live) return;
    if (large) {
        if (sl == 0) {
            const int lk = best_pos[f];
            const bool any = lk != kKeyNone;
            const int pos = lk & ((1 << kPosBits) - 1);
            best_pos[f] = any ? pos : -1;
            best_median[f] = any ? lk >> kPosBits : -1;
            if (any && out_desc) {
                const uint4* pr = reinterpret_cast<const uint4*>(pool + (size_t)obs_row[(size_t)o0 + pos] * 32);
                uint4* po = reinterpret_cast<uint4*>(out_desc + (size_t)f * 32);
                po[0] = pr[0];
                po[1] = pr[1];
            }
        }
        return;
    }
    const bool any = key != INT_MAX;
    if (sl == 0) {
        best_pos[f] = any ? key & 63 : -1;
        best_median[f] = any ? key >> 6 : -1;
    }
    if (any && out_desc && sl == (key & 63)) {
        uint4* po = reinterpret_cast<uint4*>(out_desc + (size_t)f * 32);
        po[0] = a0;
        po[1] = a1;
    }
}

// The k-th smallest (0-based) of a 257-bin histogram, by one wave; the bins are left zero.
__device__ __forceinline__ int hist_kth(unsigned* __restrict__ h, int k, int lane) {
    uint4* h4 = reinterpret_cast<uint4*>(h);
    const uint4 c = h4[lane];  // bins 4*lane .. 4*lane + 3
    h4[lane] = make_uint4(0, 0, 0, 0);
    if (lane == 0) h[256] = 0;
    const int s = (int)(c.x + c.y + c.z + c.w);
    const int incl = wave_incl_scan(s, lane);
    const unsigned long long above = __ballot(incl > k);
    if (!above) return 256;  // the k-th value lies in bin 256
    const int L = __ffsll((long long)above) - 1;
    const int excl = incl - s;
    int v = 4 * lane + 3;
    if (excl + (int)c.x > k) v = 4 * lane;
    else if (excl + (int)(c.x + c.y) > k) v = 4 * lane + 1;
    else if (excl + (int)(c.x + c.y + c.z) > k) v = 4 * lane + 2;
    return __shfl(v, L, kWave);
}

__global__ __launch_bounds__(kLargeThreads) void distinctive_large_kernel(
    int split, const uint8_t* __restrict__ pool, int pool_rows, const int* __restrict__ obs_off,
    const int* __restrict__ obs_row, int max_obs, int cap, int* __restrict__ best_key) {
    extern __shared__ __align__(16) unsigned char lds[];
    // cap = max_obs rounded up to a multiple of 4: the histograms are read 16 bytes at a time
    uint4* sdesc = reinterpret_cast<uint4*>(lds);                                   // [cap][2]
    int* sok = reinterpret_cast<int*>(lds + (size_t)32 * cap);                      // [cap]
    unsigned* hist = reinterpret_cast<unsigned*>(sok + cap);                        // [waves][rows][kHistPitch]
    int* scnt = reinterpret_cast<int*>(hist + kLargeWaves * kLargeRows * kHistPitch);
    const int f = blockIdx.x / split, c = blockIdx.x - f * split;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int o0 = obs_off[f], len = list_length(obs_off, f, max_obs);
    // a short list belongs to the small kernel; a workgroup past the end of the list has no row
    if (len <= kSmallMax || c * kLargeWaves * kLargeRows >= len) return;
    if (tid == 0) *scnt = 0;
    for (int b = tid; b < kLargeWaves * kLargeRows * kHistPitch; b += kLargeThreads) hist[b] = 0;
    __syncthreads();
    // Every workgroup of the feature stages the whole list at its list positions (no compaction:
    // the workgroups divide the rows by position, so all of them must see the same layout); an
    // ignored entry keeps its slot, flagged, and is counted in no histogram.
    for (int t = tid; t < len; t += kLargeThreads) {
        const int row = obs_row[(size_t)o0 + t];
        const bool ok = (unsigned)row < (unsigned)pool_rows;
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
        if (ok) {
            const uint4* pr = reinterpret_cast<const uint4*>(pool + (size_t)row * 32);
            r0 = pr[0];
            r1 = pr[1];
            atomicAdd(scnt, 1);
        }
        sok[t] = ok;
        sdesc[2 * t] = r0;
        sdesc[2 * t + 1] = r1;
    }
    __syncthreads();
    const int N = *scnt, k = (N - 1) >> 1;
    unsigned* h = hist + (size_t)wv * kLargeRows * kHistPitch;
    int best = INT_MAX;
    for (int i0 = (c * kLargeWaves + wv) * kLargeRows; i0 < len; i0 += split * kLargeWaves * kLargeRows) {
        uint4 a0[kLargeRows], a1[kLargeRows];
#pragma unroll
        for (int r = 0; r < kLargeRows; ++r) {
            const int i = min(i0 + r, len - 1);
            a0[r] = sdesc[2 * i];
            a1[r] = sdesc[2 * i + 1];
        }
        for (int j = lane; j < len; j += kWave) {
            const uint4 b0 = sdesc[2 * j], b1 = sdesc[2 * j + 1];
            const bool ok = sok[j] != 0;  // an ignored entry goes to a padding bin that is never read
#pragma unroll
            for (int r = 0; r < kLargeRows; ++r)
                atomicAdd(&h[r * kHistPitch + (ok ? hamming256(a0[r], a1[r], b0, b1) : kHistDump)], 1u);
        }
        // the wave's own LDS atomics, read back by the same wave
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
        for (int r = 0; r < kLargeRows; ++r) {
            const int med = hist_kth(h + r * kHistPitch, k, lane);
            if (i0 + r < len && sok[i0 + r]) best = min(best, med << kPosBits | (i0 + r));
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (lane == 0 && best != INT_MAX) atomicMin(best_key + f, best);
}

static size_t large_lds_bytes(int cap) {
    return (size_t)36 * cap + 4 * (size_t)kLargeWaves * kLargeRows * kHistPitch + 16;
}

template <int S>
static void launch_small(int n_feat, const uint8_t* d_pool, int pool_rows, const int* d_obs_off, const int* d_obs_row,
                         int max_obs, int* d_best_pos, int* d_best_median, uint8_t* d_out_desc, hipStream_t st) {
    const int per_block = 256 / S;
    const int blocks = (int)(((long long)n_feat + per_block - 1) / per_block);
    hipLaunchKernelGGL(distinctive_small_kernel<S>, dim3(blocks), dim3(256), 0, st, n_feat, d_pool, pool_rows, d_obs_off,
                       d_obs_row, max_obs, d_best_pos, d_best_median, d_out_desc);
}

}  // namespace plvi

using namespace plvi;

extern "C" int plvi_distinctive_descriptors_batch(int n_feat, const uint8_t* d_pool, int pool_rows,
                                                  const int* d_obs_off, const int* d_obs_row, int max_obs,
                                                  int* d_best_pos, int* d_best_median, uint8_t* d_out_desc,
                                                  void* stream) {
    if (n_feat < 0 || pool_rows < 0 || max_obs < 0) return PLVI_E_BADARG;
    if (n_feat == 0) return PLVI_OK;
    if (!d_obs_off || !d_best_pos || !d_best_median) return PLVI_E_BADARG;
    if (max_obs > 0 && pool_rows > 0 && (!d_pool || !d_obs_row)) return PLVI_E_BADARG;
    if (max_obs > PLVI_DISTINCTIVE_MAX_OBS) return PLVI_E_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    if (max_obs > kSmallMax) {
        const int split = (max_obs + kLargeRowsPerGroup - 1) / kLargeRowsPerGroup;
        const int cap = (max_obs + 3) & ~3;
        const size_t smem = large_lds_bytes(cap);
        if ((long long)n_feat * split > INT_MAX) return PLVI_E_CAPACITY;
        // (max_obs <= PLVI_DISTINCTIVE_MAX_OBS keeps smem near 90 KB: launch_lds cannot refuse after the memset)
        PLVI_CHECK(hipMemsetAsync(d_best_pos, kKeyNone & 0xff, 4 * (size_t)n_feat, st));
        if (int rc = launch_lds<distinctive_large_kernel>(dim3(n_feat * split), dim3(kLargeThreads), smem, st, split,
                                                          d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, cap,
                                                          d_best_pos))
            return rc;
    }
    if (max_obs <= 8)
        launch_small<8>(n_feat, d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, d_best_pos, d_best_median,
                        d_out_desc, st);
    else if (max_obs <= 16)
        launch_small<16>(n_feat, d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, d_best_pos, d_best_median,
                         d_out_desc, st);
    else if (max_obs <= 32)
        launch_small<32>(n_feat, d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, d_best_pos, d_best_median,
                         d_out_desc, st);
    else
        launch_small<64>(n_feat, d_pool, pool_rows, d_obs_off, d_obs_row, max_obs, d_best_pos, d_best_median,
                         d_out_desc, st);
    PLVI_CHECK(hipGetLastError());
    return PLVI_OK;
}

extern "C" int plvi_distinctive_descriptors(const uint8_t* pool, int pool_rows, const int* obs_off, const int* obs_row,
                                            int n_feat, int* best_pos, int* best_median, uint8_t* out_desc) {
    if (n_feat < 0 || pool_rows < 0) return PLVI_E_BADARG;
    if (n_feat == 0) return 0;
    if (!obs_off || !best_pos || !best_median || obs_off[0] < 0) return PLVI_E_BADARG;
    int max_obs = 0;
    for (int i = 0; i < n_feat; ++i) {
        if (obs_off[i + 1] < obs_off[i]) return PLVI_E_BADARG;
        max_obs = obs_off[i + 1] - obs_off[i] > max_obs ? obs_off[i + 1] - obs_off[i] : max_obs;
    }
    const size_t n_obs = (size_t)obs_off[n_feat];
    if ((n_obs && !obs_row) || (pool_rows && !pool)) return PLVI_E_BADARG;
    if (max_obs > PLVI_DISTINCTIVE_MAX_OBS) return PLVI_E_CAPACITY;
    // rows with best_pos = -1 stay as the caller left them: the rows come back into a copy
    std::vector<uint8_t> rows(out_desc ? 32 * (size_t)n_feat : 0);
    HostStage st;
    const auto P = st.in_or_zero(pool, pool_rows, 32);
    const auto O = st.in(obs_off, n_feat + 1);
    const auto R = st.in_or_zero(obs_row, n_obs);
    const auto B = st.out(best_pos, n_feat);
    const auto M = st.out(best_median, n_feat);
    const auto D = st.out_or_scratch(out_desc ? rows.data() : nullptr, n_feat, 32);
    if (int rc = st.commit()) return rc;
    if (int rc = plvi_distinctive_descriptors_batch(n_feat, st.dev(P), pool_rows, st.dev(O), st.dev(R), max_obs,
                                                    st.dev(B), st.dev(M), st.dev(D), nullptr))
        return rc;
    if (int rc = st.fetch()) return rc;
    int count = 0;
    for (int i = 0; i < n_feat; ++i) {
        if (best_pos[i] < 0) continue;
        ++count;
        if (out_desc) memcpy(out_desc + 32 * (size_t)i, rows.data() + 32 * (size_t)i, 32);
    }
    return count;
}
