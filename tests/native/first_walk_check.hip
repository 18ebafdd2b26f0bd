// first_walk_check.hip -- the first-occurrence walk of csrc/first_walk.h (first_mark + first_compact in
// a one-workgroup kernel of 1024 threads, and first_mark alone over a functor) against a host first-come
// loop that inserts into a std::set along the traversal, and the attribute gather of csrc/map_pool.h
// against a host copy.  Exact equality.  Exit 0 = every case identical.  Test infrastructure.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "../../pl-vi-orbslam3_amd/csrc/first_walk.h"
#include "../../pl-vi-orbslam3_amd/csrc/map_pool.h"

using namespace plvi;

static int g_bad = 0, g_cases = 0;
static std::mt19937 g_rng(22);

#define HIP_OK(expr)                                               \
    do {                                                           \
        if ((expr) != hipSuccess) {                                \
            printf("HIP error at line %d: %s\n", __LINE__, #expr); \
            exit(2);                                               \
        }                                                          \
    } while (0)

static void report(bool ok, const char* what, int a, int b, int c, int d) {
    ++g_cases;
    if (!ok) {
        if (g_bad < 10) printf("MISMATCH %s (%d, %d, %d, %d)\n", what, a, b, c, d);
        ++g_bad;
    }
}

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n;
    explicit Dev(size_t n_) : n(n_) { HIP_OK(hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1))); }
    explicit Dev(const std::vector<T>& v) : Dev(v.size()) { put(v); }
    ~Dev() { (void)hipFree(p); }
    void put(const std::vector<T>& v) { HIP_OK(hipMemcpy(p, v.data(), sizeof(T) * n, hipMemcpyHostToDevice)); }
    void fill(int byte) { HIP_OK(hipMemset(p, byte, sizeof(T) * std::max<size_t>(n, 1))); }
    std::vector<T> get() const {
        std::vector<T> v(n);
        HIP_OK(hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost));
        return v;
    }
};

// ---------------------------------------------------------------- mark + compaction over rows
constexpr int kThreads = 1024, kPer = 8;
constexpr int kFill = -77;  // the caller's fill of the output cells

struct WalkArgs {
    KfTable v;
    const int* rows;
    int n_rows;
    const uint8_t* in_map;  // the extra predicate, or null
    unsigned* first;
    int reset, out_cap;
    int *out_id, *out_e, *count;
};

__global__ __launch_bounds__(kThreads) void walk_kernel(WalkArgs a) {
    __shared__ int s_wave[kThreads / kWave];
    const auto pred = [&](int id) { return !a.in_map || a.in_map[id]; };
    first_mark<kThreads>((unsigned)a.n_rows * (unsigned)a.v.cap, a.first, row_walk(a.rows, a.v, pred), a.reset);
    const int n = first_compact<kThreads, kPer>(a.rows, a.n_rows, a.v, a.first, pred, s_wave,
                                                [&](int at, int id, unsigned e) {
                                                    if (at >= a.out_cap) return;
                                                    a.out_id[at] = id;
                                                    a.out_e[at] = (int)e;
                                                });
    if (threadIdx.x == 0) *a.count = n;
}

// One table of n_rows + 2 keyframe slots walked in a shuffled order: ntab cycles through 0, cap, in
// between, negative and above cap; ids are -1, >= n, bad, repeats of the entry before or of the row
// before, or uniform over the pool.  Run with every cell available and with half the count.
static void check_walk(int cap, int n_rows, bool small_pool, bool with_pred, bool reset) {
    const int K = n_rows + 2, total = n_rows * cap, n = small_pool ? 50 : total + 17;
    std::vector<int> tab((size_t)K * cap), ntab(K), rows(K);
    std::vector<uint8_t> bad(n), in_map(n);
    for (auto& b : bad) b = g_rng() % 10 == 0;
    for (auto& m : in_map) m = g_rng() % 5 != 0;
    for (int s = 0; s < K; ++s) {
        const int lens[5] = {0, cap, (int)(g_rng() % (cap + 1)), -3, cap + 5};
        ntab[s] = lens[s % 5];
        for (int i = 0; i < cap; ++i) {
            const unsigned r = g_rng() % 20;
            const int wild[3] = {n, n + 7, INT_MAX};
            int& id = tab[(size_t)s * cap + i];
            if (r < 2) id = -1;
            else if (r == 2) id = wild[g_rng() % 3];
            else if (r < 5 && i > 0) id = tab[(size_t)s * cap + i - 1];
            else if (r < 7 && s > 0) id = tab[(size_t)(s - 1) * cap + i];
            else id = (int)(g_rng() % n);
        }
    }
    std::iota(rows.begin(), rows.end(), 0);
    std::shuffle(rows.begin(), rows.end(), g_rng);

    std::vector<int> exp_id, exp_e;
    std::set<int> seen;
    for (int r = 0; r < n_rows; ++r) {
        const int s = rows[r], len = std::min(std::max(ntab[s], 0), cap);
        for (int i = 0; i < len; ++i) {
            const int id = tab[(size_t)s * cap + i];
            if (id < 0 || id >= n || bad[id] || (with_pred && !in_map[id])) continue;
            if (seen.insert(id).second) {
                exp_id.push_back(id);
                exp_e.push_back(r * cap + i);
            }
        }
    }
    const int count = (int)exp_id.size();

    Dev<int> d_tab(tab), d_ntab(ntab), d_rows(rows), d_id((size_t)total + 1), d_e((size_t)total + 1), d_count(1);
    Dev<uint8_t> d_bad(bad), d_map(in_map);
    Dev<unsigned> d_first((size_t)n);
    const int caps[2] = {total, count / 2};
    for (int out_cap : caps) {
        d_first.fill(reset ? 0xA5 : 0xFF);
        d_id.put(std::vector<int>((size_t)total + 1, kFill));
        d_e.put(std::vector<int>((size_t)total + 1, kFill));
        WalkArgs a{KfTable{d_tab.p, d_ntab.p, cap, n, d_bad.p}, d_rows.p, n_rows, with_pred ? d_map.p : nullptr,
                   d_first.p, reset, out_cap, d_id.p, d_e.p, d_count.p};
        hipLaunchKernelGGL(walk_kernel, dim3(1), dim3(kThreads), 0, nullptr, a);
        HIP_OK(hipDeviceSynchronize());
        const std::vector<int> id = d_id.get(), e = d_e.get();
        bool ok = d_count.get()[0] == count;  // the full count, also above the capacity
        for (int at = 0; at <= total; ++at) {
            const bool kept = at < std::min(count, out_cap);
            ok &= id[at] == (kept ? exp_id[at] : kFill) && e[at] == (kept ? exp_e[at] : kFill);
        }
        report(ok, "first_mark + first_compact", cap, n_rows, small_pool * 4 + with_pred * 2 + reset, out_cap);
    }
}

// ---------------------------------------------------------------- the mark pass over a functor
constexpr int kMergeJ = 6, kMergeN1 = 5, kMergePool = 12;

__global__ __launch_bounds__(kThreads) void mark_kernel(const int* ids, int J, int n1, unsigned* first, int reset) {
    const auto id_at = [&](unsigned e) {
        const int j = (int)(e / (unsigned)n1);
        return ids[j * n1 + (int)(e - (unsigned)j * (unsigned)n1)];
    };
    first_mark<kThreads>((unsigned)J * (unsigned)n1, first, id_at, reset);
}

static void check_merge_form(bool reset) {
    std::vector<int> ids(kMergeJ * kMergeN1);
    for (int& id : ids) id = g_rng() % 4 == 0 ? -1 : (int)(g_rng() % (kMergePool - 2));  // two ids never met
    const unsigned fill = reset ? 0xA5A5A5A5u : kNoPos;
    std::vector<unsigned> expect(kMergePool, fill);
    for (int e = (int)ids.size() - 1; e >= 0; --e)
        if (ids[e] >= 0) expect[ids[e]] = (unsigned)e;
    Dev<int> d_ids(ids);
    Dev<unsigned> d_first((size_t)kMergePool);
    d_first.fill(reset ? 0xA5 : 0xFF);
    hipLaunchKernelGGL(mark_kernel, dim3(1), dim3(kThreads), 0, nullptr, d_ids.p, kMergeJ, kMergeN1, d_first.p, reset);
    HIP_OK(hipDeviceSynchronize());
    report(d_first.get() == expect, "first_mark over a functor", kMergeJ, kMergeN1, reset, 0);
}

// ---------------------------------------------------------------- the attribute gather
constexpr int kGather = 256;

__global__ __launch_bounds__(kGather) void gather_kernel(PoolGather g, const int* list, int n_list) {
    const int tid = threadIdx.x, base = blockIdx.x * kGather, n = min(n_list - base, kGather);
    if (tid < n && list[base + tid] >= 0) g.rows((size_t)(base + tid), (size_t)list[base + tid]);
    g.descriptors<kGather>(max(n, 0), tid, [&](int e, size_t* at) { return list[*at = base + e]; });
}

template <class T>
static bool rows_equal(const std::vector<T>& out, const std::vector<T>& src, const std::vector<int>& list, int w,
                       bool on, T fill) {
    bool ok = true;
    for (size_t at = 0; at < list.size(); ++at)
        for (int k = 0; k < w; ++k)
            ok &= out[at * w + k] == (on && list[at] >= 0 ? src[(size_t)list[at] * w + k] : fill);
    return ok;
}

// n rows of a pool of 300 in list order, one row in seven skipped; `mask` names the destinations that are set
static void check_gather(int n, unsigned mask) {
    const int pool = 300;
    std::vector<float> pos(pool * 3), normal(pool * 3), dist(pool * 2);
    std::vector<double> sep(pool * 6);
    std::vector<uint8_t> desc(pool * 32);
    for (auto& x : pos) x = (float)(int)g_rng();
    for (auto& x : normal) x = (float)(int)g_rng();
    for (auto& x : dist) x = (float)(int)g_rng();
    for (auto& x : sep) x = (double)(int)g_rng();
    for (auto& x : desc) x = (uint8_t)g_rng();
    std::vector<int> list(n);
    for (int& id : list) id = g_rng() % 7 == 0 ? -1 : (int)(g_rng() % pool);
    Dev<float> d_pos(pos), d_normal(normal), d_dist(dist), o_pos((size_t)n * 3), o_normal((size_t)n * 3),
        o_dist((size_t)n * 2);
    Dev<double> d_sep(sep), o_sep((size_t)n * 6);
    Dev<uint8_t> d_desc(desc), o_desc((size_t)n * 32);
    Dev<int> d_list(list);
    o_pos.fill(0), o_normal.fill(0), o_dist.fill(0), o_sep.fill(0), o_desc.fill(0);
    const PoolGather g{d_pos.p, d_sep.p, d_normal.p, d_dist.p, d_desc.p,
                       mask & 1 ? o_pos.p : nullptr, mask & 2 ? o_sep.p : nullptr, mask & 4 ? o_normal.p : nullptr,
                       mask & 8 ? o_dist.p : nullptr, mask & 16 ? o_desc.p : nullptr};
    hipLaunchKernelGGL(gather_kernel, dim3((n + kGather - 1) / kGather + 1), dim3(kGather), 0, nullptr, g, d_list.p, n);
    HIP_OK(hipDeviceSynchronize());
    const bool ok = rows_equal(o_pos.get(), pos, list, 3, mask & 1, 0.f) &&
                    rows_equal(o_sep.get(), sep, list, 6, mask & 2, 0.0) &&
                    rows_equal(o_normal.get(), normal, list, 3, mask & 4, 0.f) &&
                    rows_equal(o_dist.get(), dist, list, 2, mask & 8, 0.f) &&
                    rows_equal(o_desc.get(), desc, list, 32, mask & 16, (uint8_t)0);
    report(ok, "PoolGather", n, (int)mask, 0, 0);
}

int main() {
    const int caps[] = {1, 3, 8, 13, 64}, n_rows[] = {0, 1, 2, 6, 31};
    // totals around the scan block of kThreads * kPer = 8192 positions: {cap, rows}
    const int large[][2] = {{1, 8191}, {1, 8192}, {1, 8193}, {3, 2731}, {1, 16389}};
    for (int flags = 0; flags < 8; ++flags) {
        const bool small_pool = flags & 4, with_pred = flags & 2, reset = flags & 1;
        for (int cap : caps)
            for (int nr : n_rows) check_walk(cap, nr, small_pool, with_pred, reset);
        for (const auto& l : large) check_walk(l[0], l[1], small_pool, with_pred, reset);
    }
    check_merge_form(false);
    check_merge_form(true);
    const int gather_rows[] = {0, 1, 255, 256, 257};
    for (int n : gather_rows)
        for (unsigned mask : {31u, 21u, 10u}) check_gather(n, mask);
    printf("%d cases, %d mismatching\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
