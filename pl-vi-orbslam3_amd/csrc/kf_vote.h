// kf_vote.h — the keyframe vote shared by lm_keyframes_kernel (local_map.hip) and
// covis_count_kernel (covis.hip): a feature adds 1 to every keyframe of its observation list, in
// a histogram over the keyframe slots (LDS or global), and the ordered block scan both kernels
// compact `order` with.
#pragma once
#include "plvi_common.h"

namespace plvi {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// exclusive scan of v over a workgroup of NW waves (every thread calls it); *total = the sum
template <int NW>
__device__ int block_scan(int v, int* s_wave, int tid, int* total) {
    const int lane = tid & (kWave - 1), wv = tid / kWave;
    int incl = v;
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const int up = __shfl_up(incl, m, kWave);
        if (lane >= m) incl += up;
    }
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

// the observation list of feature id votes into hist[0, K); a slot outside is ignored
__device__ __forceinline__ void vote_observations(int* hist, int K, const int* obs_off, const int* obs_kf, int id) {
    const int o1 = obs_off[id + 1];
    for (int o = obs_off[id]; o < o1; ++o) {
        const int kf = obs_kf[o];
        if ((unsigned)kf < (unsigned)K) atomicAdd(hist + kf, 1);
    }
}

}  // namespace plvi
