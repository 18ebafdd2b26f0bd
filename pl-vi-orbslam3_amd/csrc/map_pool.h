// map_pool.h — what the local-map update and the covisibility graph share
// about a plvi_local_map_pool: its argument check and its staging for their
// host forms.
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

}  // namespace plvi
