// map_pool.h — what the map-side modules share about a plvi_local_map_pool:
// its argument check, its staging for their host forms, the keyframe vote
// over its observation lists, and the gather of its attribute rows.
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

// The attribute gather of lm_write_kernel (local_map.hip) and loop_gather_kernel (loop_window.hip):
// pool rows into the rows of a list, in the layouts of plvi_frustum_*_batch.  A null destination is
// skipped; its source is then not read.
struct PoolGather {
    const float* pos;
    const double* sep;
    const float *normal, *dist;
    const uint8_t* desc;
    float* o_pos;
    double* o_sep;
    float *o_normal, *o_dist;
    uint8_t* o_desc;

    // one thread: the pos / sep / normal / dist rows of pool entry id into list row `at`
    __device__ __forceinline__ void rows(size_t at, size_t id) const {
        if (o_pos) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o_pos[3 * at + k] = pos[3 * id + k];
        }
        if (o_sep) {
#pragma unroll
            for (int k = 0; k < 6; ++k) o_sep[6 * at + k] = sep[6 * id + k];
        }
        if (o_normal) {
#pragma unroll
            for (int k = 0; k < 3; ++k) o_normal[3 * at + k] = normal[3 * id + k];
        }
        if (o_dist) {
            o_dist[2 * at] = dist[2 * id];
            o_dist[2 * at + 1] = dist[2 * id + 1];
        }
    }

    // NT threads: n descriptors, 32-byte rows as 8 dwords, 8 consecutive lanes a row.  row(e, &at) is
    // the pool id of the e-th and sets its list row, or is negative to skip it.
    template <int NT, class Row>
    __device__ __forceinline__ void descriptors(int n, int tid, Row row) const {
        if (!o_desc) return;
        const unsigned* src = reinterpret_cast<const unsigned*>(desc);
        unsigned* dst = reinterpret_cast<unsigned*>(o_desc);
        for (int k = tid; k < n * 8; k += NT) {
            size_t at;
            const int id = row(k >> 3, &at);
            if (id >= 0) dst[at * 8 + (k & 7)] = src[(size_t)id * 8 + (k & 7)];
        }
    }
};

}  // namespace plvi
