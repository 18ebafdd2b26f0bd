// block_prims_check.hip -- every primitive of csrc/block_prims.h in a one-workgroup kernel
// against the host: block_scan and block_scan_array vs std::partial_sum, block_add vs
// std::accumulate, bitonic_sort vs std::sort, hamming256 vs a bit loop, pow2_at_least vs its
// definition.  Exact equality.
// Exit 0 = every case identical.  Test infrastructure.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "../../pl-vi-orbslam3_amd/csrc/block_prims.h"

using namespace plvi;
typedef unsigned long long u64;

static int g_bad = 0, g_cases = 0;
static std::mt19937 g_rng(18);

#define HIP_OK(expr)                                               \
    do {                                                           \
        if ((expr) != hipSuccess) {                                \
            printf("HIP error at line %d: %s\n", __LINE__, #expr); \
            exit(2);                                               \
        }                                                          \
    } while (0)

static void report(bool ok, const char* what, int a, int b, int c) {
    ++g_cases;
    if (!ok) {
        if (g_bad < 10) printf("MISMATCH %s (%d, %d, %d)\n", what, a, b, c);
        ++g_bad;
    }
}

template <class T>
struct Dev {
    T* p = nullptr;
    size_t n;
    explicit Dev(size_t n_) : n(n_) { HIP_OK(hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1))); }
    explicit Dev(const std::vector<T>& v) : Dev(v.size()) {
        HIP_OK(hipMemcpy(p, v.data(), sizeof(T) * n, hipMemcpyHostToDevice));
    }
    ~Dev() { (void)hipFree(p); }
    std::vector<T> get() const {
        std::vector<T> v(n);
        HIP_OK(hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost));
        return v;
    }
};

// ---------------------------------------------------------------- block_scan
// two scans back to back through the same s_wave: the reuse contract
template <int NW>
__global__ __launch_bounds__(NW * kWave) void scan_kernel(const int* a, const int* b, int* out) {
    __shared__ int s_wave[NW];
    const int tid = threadIdx.x, NT = NW * kWave;
    int ta, tb;
    const int pa = block_scan<NW>(a[tid], s_wave, tid, &ta);
    const int pb = block_scan<NW>(b[tid], s_wave, tid, &tb);
    out[tid] = pa;
    out[NT + tid] = pb;
    out[2 * NT + tid] = ta;
    out[3 * NT + tid] = tb;
}

static std::vector<int> scan_input(int n, int kind) {
    std::vector<int> v(n);
    for (int& x : v) {
        const unsigned r = g_rng();
        x = kind == 0 ? 0 : kind == 1 ? 1 : (r % 4 == 0 ? 0 : r % 4 == 1 ? 1 : (int)(r >> 12));  // large: < 2^20
    }
    return v;
}

template <int NW>
static void check_scan() {
    const int NT = NW * kWave;
    for (int ka = 0; ka < 3; ++ka)
        for (int kb = 0; kb < 3; ++kb) {
            const std::vector<int> a = scan_input(NT, ka), b = scan_input(NT, kb);
            Dev<int> da(a), db(b), dout((size_t)4 * NT);
            hipLaunchKernelGGL(scan_kernel<NW>, dim3(1), dim3(NT), 0, nullptr, da.p, db.p, dout.p);
            HIP_OK(hipDeviceSynchronize());
            const std::vector<int> out = dout.get();
            std::vector<int> ea(NT + 1, 0), eb(NT + 1, 0);
            std::partial_sum(a.begin(), a.end(), ea.begin() + 1);
            std::partial_sum(b.begin(), b.end(), eb.begin() + 1);
            bool ok = true;
            for (int t = 0; t < NT; ++t)
                ok &= out[t] == ea[t] && out[NT + t] == eb[t] && out[2 * NT + t] == ea[NT] && out[3 * NT + t] == eb[NT];
            report(ok, "block_scan", NW, ka, kb);
        }
}

// ---------------------------------------------------------------- block_add
// two counters through the one pattern of the callers: initialise, barrier, add, barrier, read
template <int NW>
__global__ __launch_bounds__(NW * kWave) void add_kernel(const int* a, const int* b, int* out) {
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    if (tid == 0) s_cnt[0] = s_cnt[1] = 0;
    __syncthreads();
    block_add(a[tid], &s_cnt[0], tid);
    block_add(b[tid], &s_cnt[1], tid);
    __syncthreads();
    out[tid] = s_cnt[0];
    out[NW * kWave + tid] = s_cnt[1];
}

template <int NW>
static void check_add() {
    const int NT = NW * kWave;
    for (int ka = 0; ka < 3; ++ka)
        for (int kb = 0; kb < 3; ++kb) {
            std::vector<int> a = scan_input(NT, ka), b = scan_input(NT, kb);
            if (kb == 2) std::fill(b.begin(), b.begin() + kWave, 0);  // a wave of zeros among the others
            Dev<int> da(a), db(b), dout((size_t)2 * NT);
            hipLaunchKernelGGL(add_kernel<NW>, dim3(1), dim3(NT), 0, nullptr, da.p, db.p, dout.p);
            HIP_OK(hipDeviceSynchronize());
            const std::vector<int> out = dout.get();
            const int ea = std::accumulate(a.begin(), a.end(), 0), eb = std::accumulate(b.begin(), b.end(), 0);
            bool ok = true;
            for (int t = 0; t < NT; ++t) ok &= out[t] == ea && out[NT + t] == eb;
            report(ok, "block_add", NW, ka, kb);
        }
}

// ---------------------------------------------------------------- block_scan_array
constexpr int kArrayMax = 64 * 48 + 1;  // the line grid of stereo.hip: kLGridCells + 1

__global__ __launch_bounds__(256) void scan_array_kernel(int* data, int n, int* total) {
    __shared__ int s[kArrayMax], s_tmp[256 / kWave];
    for (int i = threadIdx.x; i < n; i += 256) s[i] = data[i];
    __syncthreads();
    const int tot = block_scan_array<256>(s, n, s_tmp);
    for (int i = threadIdx.x; i < n; i += 256) data[i] = s[i];
    total[threadIdx.x] = tot;
}

static void check_scan_array() {
    const int sizes[] = {0, 1, 255, 256, 257, 480 + 1, kArrayMax};  // 481: nRows + 1 of a 480-row image
    for (int n : sizes)
        for (int kind = 0; kind < 3; ++kind) {
            const std::vector<int> v = scan_input(n, kind);
            Dev<int> d(v), dt(256);
            hipLaunchKernelGGL(scan_array_kernel, dim3(1), dim3(256), 0, nullptr, d.p, n, dt.p);
            HIP_OK(hipDeviceSynchronize());
            const std::vector<int> out = d.get(), tot = dt.get();
            std::vector<int> e(n + 1, 0);
            std::partial_sum(v.begin(), v.end(), e.begin() + 1);
            bool ok = true;
            for (int i = 0; i < n; ++i) ok &= out[i] == e[i];
            for (int t = 0; t < 256; ++t) ok &= tot[t] == e[n];
            report(ok, "block_scan_array", n, kind, 0);
        }
}

// ---------------------------------------------------------------- bitonic_sort
template <int NT, class Key, bool kVal>
__global__ __launch_bounds__(NT) void sort_kernel(Key* gkey, int* gval, int n) {
    extern __shared__ __align__(16) unsigned char lds[];
    Key* key = reinterpret_cast<Key*>(lds);
    int* val = reinterpret_cast<int*>(key + n);
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += NT) {
        key[i] = gkey[i];
        if (kVal) val[i] = gval[i];
    }
    __syncthreads();
    if (kVal) bitonic_sort<NT>(key, val, n, tid);
    else bitonic_sort<NT>(key, n, tid);
    for (int i = tid; i < n; i += NT) {
        gkey[i] = key[i];
        if (kVal) gval[i] = val[i];
    }
}

template <int NT, class Key, bool kVal>
static void check_sort() {
    const int sizes[] = {2, 256, 512, 8192};  // 8192: the assign_grid limit, 1 << kGridKeyBits
    for (int n : sizes)
        for (int kind = 0; kind < 2; ++kind) {
            // kind 0: a handful of distinct keys; kind 1: random high bits.  The last quarter (of n = 2: the
            // last key) is the ~0 padding the callers fill a power of two with.
            std::vector<Key> k(n);
            std::vector<int> v(n);
            const int live = n == 2 ? 1 : n - n / 4;
            for (int i = 0; i < n; ++i) {
                const Key r = (Key)(((u64)g_rng() << 32) | g_rng());
                k[i] = i >= live ? (Key)~(Key)0 : kind == 0 ? (Key)(r % 7) << (4 * sizeof(Key)) : r | 1;
                v[i] = i >= live ? -1 : i;
            }
            std::shuffle(k.begin(), k.begin() + live, g_rng);
            Dev<Key> dk(k);
            Dev<int> dv(v);
            const size_t smem = (sizeof(Key) + (kVal ? 4 : 0)) * (size_t)n;
            const int rc = launch_lds<sort_kernel<NT, Key, kVal>>(dim3(1), dim3(NT), smem, nullptr, dk.p, dv.p, n);
            if (rc) {
                report(false, "bitonic_sort launch", NT, n, rc);
                continue;
            }
            HIP_OK(hipDeviceSynchronize());
            const std::vector<Key> ok_ = dk.get();
            const std::vector<int> ov = dv.get();
            std::vector<Key> ek = k;
            std::sort(ek.begin(), ek.end());
            bool ok = ok_ == ek;
            if (kVal) {  // every (key, val) pair survives; the order of vals among equal keys is free
                std::vector<std::pair<Key, int>> got(n), exp(n);
                for (int i = 0; i < n; ++i) {
                    got[i] = {ok_[i], ov[i]};
                    exp[i] = {k[i], v[i]};
                }
                std::sort(got.begin(), got.end());
                std::sort(exp.begin(), exp.end());
                ok &= got == exp;
            }
            report(ok, kVal ? "bitonic_sort+val" : "bitonic_sort", NT, n, (int)sizeof(Key) * 10 + kind);
        }
}

template <int NT>
static void check_sorts() {
    check_sort<NT, unsigned, false>();
    check_sort<NT, unsigned, true>();
    check_sort<NT, u64, false>();
    check_sort<NT, u64, true>();
}

// ---------------------------------------------------------------- hamming256
__global__ void hamming_kernel(const uint4* a, const uint4* b, int n, int* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = hamming256(a[2 * i], a[2 * i + 1], b[2 * i], b[2 * i + 1]);
    out[n + i] = hamming256(a[2 * i], a[2 * i + 1], reinterpret_cast<const uint8_t*>(b + 2 * i));
}

static void check_hamming() {
    const int dists[] = {0, 1, 255, 256, 3, 64, 100, 128, 129, 200};
    const int n = (int)(sizeof(dists) / sizeof(dists[0])) * 4;
    std::vector<uint4> a(2 * n), b(2 * n);
    std::vector<int> expect(n);
    for (int i = 0; i < n; ++i) {
        unsigned wa[8], wb[8];
        for (int w = 0; w < 8; ++w) wb[w] = wa[w] = g_rng();
        std::vector<int> bit(256);
        std::iota(bit.begin(), bit.end(), 0);
        std::shuffle(bit.begin(), bit.end(), g_rng);
        for (int k = 0; k < dists[i % 10]; ++k) wb[bit[k] >> 5] ^= 1u << (bit[k] & 31);
        int d = 0;
        for (int k = 0; k < 256; ++k) d += ((wa[k >> 5] >> (k & 31)) & 1u) != ((wb[k >> 5] >> (k & 31)) & 1u);
        expect[i] = d;
        a[2 * i] = make_uint4(wa[0], wa[1], wa[2], wa[3]);
        a[2 * i + 1] = make_uint4(wa[4], wa[5], wa[6], wa[7]);
        b[2 * i] = make_uint4(wb[0], wb[1], wb[2], wb[3]);
        b[2 * i + 1] = make_uint4(wb[4], wb[5], wb[6], wb[7]);
    }
    Dev<uint4> da(a), db(b);
    Dev<int> dout((size_t)2 * n);
    hipLaunchKernelGGL(hamming_kernel, dim3(1), dim3(64), 0, nullptr, da.p, db.p, n, dout.p);
    HIP_OK(hipDeviceSynchronize());
    const std::vector<int> out = dout.get();
    for (int i = 0; i < n; ++i)
        report(expect[i] == dists[i % 10] && out[i] == expect[i] && out[n + i] == expect[i], "hamming256", i, out[i],
               expect[i]);
}

// ---------------------------------------------------------------- wave_sum / wave_incl_scan
__global__ void wave_kernel(const int* in, int* out) {
    const int lane = threadIdx.x;
    out[lane] = wave_sum(in[lane]);
    out[kWave + lane] = wave_incl_scan(in[lane], lane);
}

static void check_wave() {
    const std::vector<int> v = scan_input(kWave, 2);
    Dev<int> d(v), dout((size_t)2 * kWave);
    hipLaunchKernelGGL(wave_kernel, dim3(1), dim3(kWave), 0, nullptr, d.p, dout.p);
    HIP_OK(hipDeviceSynchronize());
    const std::vector<int> out = dout.get();
    std::vector<int> e(kWave);
    std::partial_sum(v.begin(), v.end(), e.begin());
    bool ok = true;
    for (int l = 0; l < kWave; ++l) ok &= out[l] == e[kWave - 1] && out[kWave + l] == e[l];
    report(ok, "wave_sum / wave_incl_scan", 0, 0, 0);
}

int main() {
    const int pin[][3] = {{0, 256, 256},   {1, 256, 256},   {256, 256, 256},   {257, 256, 512}, {8192, 256, 8192},
                          {8193, 256, 16384}, {0, 1, 1},    {1, 1, 1},         {3, 1, 4}};
    for (const auto& p : pin) report(pow2_at_least(p[0], p[1]) == p[2], "pow2_at_least", p[0], p[1], p[2]);
    check_scan<1>();
    check_scan<4>();
    check_scan<8>();   // tri_match_kernel's 512 threads
    check_scan<16>();  // kfdb_select_kernel's 1024
    check_add<1>();
    check_add<4>();   // lm_count_kernel's 256 threads
    check_add<16>();  // ba_window_kernel's and loop_bow_merge_kernel's 1024
    check_scan_array();
    check_sorts<64>();
    check_sorts<256>();
    check_sorts<1024>();  // kSelThreads
    check_hamming();
    check_wave();
    printf("%d cases, %d mismatching\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
