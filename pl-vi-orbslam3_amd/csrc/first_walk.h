// first_walk.h — the first-occurrence walk of the map-side kernels (ba_window.hip, loop_window.hip,
// local_map.hip).  The reference decides "first come" with a stamp or a std::set along a fixed traversal
// of keyframe tables; here the rows of the traversal are laid end to end, position e = r * cap + i, and
// the smallest position wins:
//   mark     atomicMin of every live entry's position into first[], a table keyed by pool id;
//   compact  in order, the entries that hold their id's minimum.
// No step of either pass waits for the row before it.  A position is below kNoPos, which the callers'
// host checks see to (rows * cap <= PLVI_LOCAL_MAP_MAX_ENTRIES).
//
// The table-reset rule: first[] must read "none" (any value above every position) at each id the walk
// meets.  A caller either fills the table itself (ba_window.hip clears first[n] per query, local_map.hip
// memsets 0x7f) or passes reset = true, and first_mark writes kNoPos at exactly the ids it will meet, so
// the table needs no fill and the cost does not depend on the pool size (loop_window.hip).
//
// Barrier contracts (every thread of the workgroup calls, with uniform arguments; tid is threadIdx.x):
//   first_mark     the caller's fill of first[], if any, must be complete (a barrier of the caller's).
//                  Each pass ends with a barrier, so first[] is final and visible on return.
//   first_compact  first[] must be final (first_mark's last barrier).  It is block_scan calls and the
//                  caller's emit: no barrier at the end, so what emit wrote is seen by the other threads
//                  only after a barrier of the caller's; s_wave may be reused at once.
#pragma once
#include "block_prims.h"

namespace plvi {

constexpr unsigned kNoPos = 0xffffffffu;  // no position yet: above every position of a walk

// a keyframe feature table with the pool its entries name
struct KfTable {
    const int *tab, *ntab;  // [K][cap], [K]
    int cap, n;             // the row length and the pool size
    const uint8_t* bad;     // [n]

    __device__ __forceinline__ int len(int s) const { return clampi(ntab[s], 0, cap); }
    __device__ __forceinline__ int raw(int s, unsigned i) const { return tab[(size_t)s * cap + i]; }
    __device__ __forceinline__ bool live(int id) const { return in_range(id, n) && !bad[id]; }
    // the live pool id at index i of slot s's row (s in range), or -1
    __device__ __forceinline__ int at(int s, int i, int len_s) const {
        if (!in_range(i, len_s)) return -1;
        const int id = raw(s, i);
        return live(id) ? id : -1;
    }
    __device__ __forceinline__ int at(int s, int i) const { return at(s, i, len(s)); }
};

// first[id] = the smallest e in [0, total) with id_at(e) == id, for every id >= 0 that id_at names
template <int NT, class IdAt>
__device__ __forceinline__ void first_mark(unsigned total, unsigned* first, IdAt id_at, bool reset) {
    for (int pass = reset ? 0 : 1; pass < 2; ++pass) {
        for (unsigned e = threadIdx.x; e < total; e += NT) {
            const int id = id_at(e);
            if (id < 0) continue;
            if (pass == 0)
                first[id] = kNoPos;
            else
                atomicMin(first + id, e);
        }
        __syncthreads();
    }
}

// the position-to-id map of the row walk: the entries of rows[r]'s table that are live and pass pred
template <class Pred>
__device__ __forceinline__ auto row_walk(const int* rows, const KfTable& v, Pred pred) {
    return [=](unsigned e) {
        const unsigned r = e / (unsigned)v.cap;
        const int id = v.at(rows[r], (int)(e - r * (unsigned)v.cap));
        return id >= 0 && pred(id) ? id : -1;
    };
}

// The ordered compaction of the row walk marked by first_mark(n_rows * cap, first, row_walk(rows, v, pred)):
// emit(at, id, e) for the at-th kept entry, in traversal order; returns their number.  A thread takes PER
// consecutive positions (one division, then stepping), one block scan per NT * PER positions.
// s_wave: NT / kWave ints of LDS.
template <int NT, int PER, class Pred, class Emit>
__device__ __forceinline__ int first_compact(const int* rows, int n_rows, const KfTable& v, const unsigned* first,
                                             Pred pred, int* s_wave, Emit emit) {
    const int tid = threadIdx.x;
    const unsigned cap = (unsigned)v.cap, total = (unsigned)n_rows * cap;
    int n_kept = 0;
    for (unsigned base = 0; base < total; base += NT * PER) {
        const unsigned e0 = base + (unsigned)tid * PER;
        int ids[PER];
        unsigned flags = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) ids[k] = -1;
        if (e0 < total) {
            unsigned r = e0 / cap, i = e0 - r * cap;
            int s = rows[r], m = v.len(s);
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (e0 + k >= total) break;
                if ((int)i < m) ids[k] = v.raw(s, i);
                if (++i == cap && ++r < (unsigned)n_rows) {  // the next row
                    i = 0;
                    s = rows[r];
                    m = v.len(s);
                }
            }
#pragma unroll
            for (int k = 0; k < PER; ++k)
                if (v.live(ids[k]) && pred(ids[k]) && first[ids[k]] == e0 + k) flags |= 1u << k;
        }
        int tot;
        int at = n_kept + block_scan<NT / kWave>(__popc(flags), s_wave, tid, &tot);
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (flags >> k & 1) emit(at++, ids[k], e0 + k);
        n_kept += tot;
    }
    return n_kept;
}

}  // namespace plvi
