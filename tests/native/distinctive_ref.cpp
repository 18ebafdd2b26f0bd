// distinctive_ref.cpp — a sequential host restatement of MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:330-404) and MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:264-331, identical from
// the point where vDescriptors is filled), in the reference's own shape: a float Distances[N][N] (on the heap
// here, a VLA there), ORBmatcher::DescriptorDistance, std::sort on a vector<int>, the index 0.5*(N-1) and a
// strict `<` from INT_MAX.  The list conventions are those of plvi_distinctive_descriptors_batch: a CSR list of
// pool rows per feature, its length clamped to [0, max_obs], a row outside the pool ignored, the answer reported
// as the position inside the list (ignored entries counted).
// Built on demand by tests/test_distinctive.py.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

// ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:2350-2366): eight 32-bit words, the bit-twiddling popcount
int descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int i = 0; i < 8; ++i) {
        uint32_t pa, pb;
        memcpy(&pa, a + 4 * i, 4);
        memcpy(&pb, b + 4 * i, 4);
        unsigned v = pa ^ pb;
        v = v - ((v >> 1) & 0x55555555);
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
        dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
}

}  // namespace

// Returns the number of features with best_pos >= 0.  out_desc may be NULL; a row is written only then.
extern "C" int distinctive_ref(int n_feat, const uint8_t* pool, int pool_rows, const int* obs_off, const int* obs_row,
                               int max_obs, int* best_pos, int* best_median, uint8_t* out_desc) {
    int count = 0;
    for (int f = 0; f < n_feat; ++f) {
        const int len = std::max(std::min(obs_off[f + 1] - obs_off[f], max_obs), 0);
        std::vector<const uint8_t*> vDescriptors;
        std::vector<int> pos;
        for (int t = 0; t < len; ++t) {
            const int row = obs_row[(size_t)obs_off[f] + t];
            if (row < 0 || row >= pool_rows) continue;
            vDescriptors.push_back(pool + (size_t)row * 32);
            pos.push_back(t);
        }
        best_pos[f] = best_median[f] = -1;
        if (vDescriptors.empty()) continue;  // :366: mDescriptor stays
        const size_t N = vDescriptors.size();
        std::vector<float> Distances(N * N);
        for (size_t i = 0; i < N; i++) {
            Distances[i * N + i] = 0;
            for (size_t j = i + 1; j < N; j++) {
                int distij = descriptor_distance(vDescriptors[i], vDescriptors[j]);
                Distances[i * N + j] = distij;
                Distances[j * N + i] = distij;
            }
        }
        int BestMedian = INT_MAX;
        int BestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            std::vector<int> vDists(Distances.begin() + i * N, Distances.begin() + (i + 1) * N);
            std::sort(vDists.begin(), vDists.end());
            int median = vDists[0.5 * (N - 1)];
            if (median < BestMedian) {
                BestMedian = median;
                BestIdx = i;
            }
        }
        best_pos[f] = pos[BestIdx];
        best_median[f] = BestMedian;
        if (out_desc) memcpy(out_desc + (size_t)f * 32, vDescriptors[BestIdx], 32);
        ++count;
    }
    return count;
}
