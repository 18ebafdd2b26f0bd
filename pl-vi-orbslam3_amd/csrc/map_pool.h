// map_pool.h — what the local-map update and the covisibility graph share
// about a plvi_local_map_pool: its argument check, its staging for their
// host forms, and the keyframe vote over its observation lists.
#pragma once
#include "host_stage.h"

namespace plvi {

inline bool pool_ok(const plvi_local_map_pool* p) {
    return p->n >= 0 && (p->n == 0 || (p->bad && p->obs_off && p->obs_kf));
}

// Stage a pool (a copy of the caller's struct, turned into the device-side
// struct by commit()): the observation CSR, and with `gather` the attribute
// rows a gather reads, pos for MapPoints and sep for MapLines.
enum PoolRows { kPoolObs, kPoolPoints, kPoolLines };

inline void stage_pool(HostStage& hs, plvi_local_map_pool& p, PoolRows rows) {
    const size_t n = (size_t)p.n;
    const size_t n_obs = p.obs_off && n && p.obs_off[n] > 0 ? (size_t)p.obs_off[n] : 0;
    hs.field(p.bad, HostStage::In, n);
    hs.field(p.obs_off, HostStage::In, n + 1);
    hs.field(p.obs_kf, HostStage::In, n_obs);
    if (rows != kPoolPoints) p.pos = nullptr;
    if (rows != kPoolLines) p.sep = nullptr;
    if (rows == kPoolObs) {
        p.normal = p.dist = nullptr;
        p.desc = nullptr;
    }
    hs.field(p.pos, HostStage::In, n, 3);
    hs.field(p.sep, HostStage::In, n, 6);
    hs.field(p.normal, HostStage::In, n, 3);
    hs.field(p.dist, HostStage::In, n, 2);
    hs.field(p.desc, HostStage::In, n, 32);
}

// The keyframe vote of lm_keyframes_kernel (local_map.hip) and covis_count_kernel (covis.hip):
// the observation list of feature id adds 1 to hist[kf] for each of its keyframes, hist[0, K)
// a histogram over the keyframe slots (LDS or global); a slot outside is ignored.
__device__ __forceinline__ void vote_observations(int* hist, int K, const int* obs_off, const int* obs_kf, int id) {
    const int o1 = obs_off[id + 1];
    for (int o = obs_off[id]; o < o1; ++o) {
        const int kf = obs_kf[o];
        if ((unsigned)kf < (unsigned)K) atomicAdd(hist + kf, 1);
    }
}

}  // namespace plvi
