// block_prims.h — the wave and workgroup primitives the kernels share: the 256-bit Hamming
// distance, wave and workgroup scans, the wave sum and the workgroup count built on it, the bitonic
// sort of keys in LDS or global memory, and the small integer helpers that go with them.
//
// Barrier contracts of the block-wide functions (every thread of the workgroup calls them, with
// uniform arguments apart from v and tid):
//   block_scan        barrier, s_wave written, barrier, s_wave read.  No barrier at the end: the
//                     leading barrier of the next call protects s_wave, so it may be called again
//                     at once with the same s_wave.  It orders nothing but s_wave for the caller
//                     after its second barrier: what a thread writes from the result is seen by
//                     the others only after a barrier of the caller's (or the next call's).
//   block_add         no barrier: *s_counter is initialised before a barrier of the caller's ahead of
//                     the call, and holds the sum after a barrier of the caller's behind it.
//   block_scan_array  s[] must be complete before the call (a barrier of the caller's); ends with
//                     a barrier, after which every thread sees the scanned s[].  s_tmp as s_wave.
//   bitonic_sort      key[] (and val[]) must be complete before the call (a barrier of the
//                     caller's); every stage ends with a barrier, so the sorted keys are visible
//                     on return.  n < 2 runs no stage and no barrier.
#pragma once
#include "plvi_common.h"

namespace plvi {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// 0 <= v < n: the test of a slot against a table, or of an id against a pool
__device__ __forceinline__ bool in_range(int v, int n) { return (unsigned)v < (unsigned)n; }

// the smallest lo * 2^k >= n (lo a power of two)
__host__ __device__ __forceinline__ int pow2_at_least(int n, int lo) {
    int p = lo;
    while (p < n) p <<= 1;
    return p;
}

// Hamming distance of the 256-bit descriptors (a0, a1) and (b0, b1): ORBmatcher::DescriptorDistance
__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 b0, const uint4 b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// ... of (a0, a1) and the 32 bytes at b (16-aligned)
__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint8_t* __restrict__ b) {
    const uint4* pb = reinterpret_cast<const uint4*>(b);
    return hamming256(a0, a1, pb[0], pb[1]);
}

// inclusive scan of v over the wave
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const int up = __shfl_up(v, m, kWave);
        if (lane >= m) v += up;
    }
    return v;
}

// the sum of v over the wave, in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// adds every thread's v to *s_counter (LDS): one atomicAdd a wave, none for a wave that sums to zero
template <class T>
__device__ __forceinline__ void block_add(T v, T* s_counter, int tid) {
    v = wave_sum(v);
    if ((tid & (kWave - 1)) == 0 && v) atomicAdd(s_counter, v);
}

// exclusive scan of v over a workgroup of NW waves; *total = the sum.  s_wave: NW ints of LDS.
template <int NW>
__device__ int block_scan(int v, int* s_wave, int tid, int* total) {
    const int lane = tid & (kWave - 1), wv = tid / kWave;
    const int incl = wave_incl_scan(v, lane);
    __syncthreads();  // s_wave may still be read from the previous call
    if (lane == kWave - 1) s_wave[wv] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int x = s_wave[w];
        if (w < wv) base += x;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

// exclusive scan of s[0, n) in place by a workgroup of NT threads, each taking a contiguous
// run; returns the sum.  s_tmp: NT / kWave ints of LDS.
template <int NT>
__device__ int block_scan_array(int* s, int n, int* s_tmp) {
    const int tid = threadIdx.x;
    const int per = (n + NT - 1) / NT, b0 = min(n, tid * per), b1 = min(n, b0 + per);
    int local = 0;
    for (int i = b0; i < b1; ++i) local += s[i];
    int tot;
    int run = block_scan<NT / kWave>(local, s_tmp, tid, &tot);
    for (int i = b0; i < b1; ++i) {
        const int v = s[i];
        s[i] = run;
        run += v;
    }
    __syncthreads();
    return tot;
}

// ascending bitonic sort of key[0, n), n a power of two, by a workgroup of NT threads; with kVal,
// val[] is carried along (the network is not stable: equal keys may swap their vals)
template <int NT, bool kVal, class Key>
__device__ __forceinline__ void bitonic_network(Key* key, int* val, int n, int tid) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (n >> 1); t += NT) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const bool up = (i & k) == 0;
                const Key a = key[i], b = key[p];
                if ((a > b) == up) {
                    key[i] = b;
                    key[p] = a;
                    if (kVal) {
                        const int va = val[i];
                        val[i] = val[p];
                        val[p] = va;
                    }
                }
            }
            __syncthreads();
        }
}

template <int NT, class Key>
__device__ void bitonic_sort(Key* key, int n, int tid) {
    bitonic_network<NT, false>(key, nullptr, n, tid);
}

template <int NT, class Key>
__device__ void bitonic_sort(Key* key, int* val, int n, int tid) {
    bitonic_network<NT, true>(key, val, n, tid);
}

}  // namespace plvi
