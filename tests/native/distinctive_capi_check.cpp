// distinctive_capi_check.cpp — a C++11 caller of plvi_distinctive_descriptors[_batch] through
// include/plvi_frontend.h only, the way the INTEGRATION.md shims of
// MapPoint / MapLine::ComputeDistinctiveDescriptors call them.
// Usage: distinctive_capi_check <in.bin> <out.bin>
//
// in.bin (written by tests/test_distinctive_capi_native.py): int32 n_feat, pool_rows, n_obs;
// the pool [pool_rows][32]; obs_off [n_feat + 1]; obs_row [n_obs].
// out.bin: int32 count (or error), best_pos [n_feat], best_median [n_feat], out_desc
// [n_feat][32] (pre-filled with 0xA5); then int32 status of an empty batch call, of a list one
// longer than PLVI_DISTINCTIVE_MAX_OBS and of a decreasing obs_off.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plvi_frontend.h"

namespace {

FILE* g_in;

template <class T>
std::vector<T> take(size_t n) {
    std::vector<T> v(n ? n : 1);
    if (n && fread(v.data(), sizeof(T), n, g_in) != n) exit(3);
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    if (!g_in) return 3;
    const std::vector<int32_t> hd = take<int32_t>(3);
    const int n_feat = hd[0], pool_rows = hd[1], n_obs = hd[2];
    const std::vector<uint8_t> pool = take<uint8_t>((size_t)pool_rows * 32);
    const std::vector<int32_t> obs_off = take<int32_t>((size_t)n_feat + 1);
    const std::vector<int32_t> obs_row = take<int32_t>(n_obs);
    fclose(g_in);

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    // the caller copies out_desc row i into mDescriptor only where best_pos[i] >= 0
    std::vector<int32_t> best_pos(n_feat ? n_feat : 1, -7), best_median(n_feat ? n_feat : 1, -7);
    std::vector<uint8_t> out_desc((size_t)(n_feat ? n_feat : 1) * 32, 0xA5);
    const int32_t n = plvi_distinctive_descriptors(pool.data(), pool_rows, obs_off.data(), obs_row.data(), n_feat,
                                                   best_pos.data(), best_median.data(), out_desc.data());
    fwrite(&n, 4, 1, o);
    fwrite(best_pos.data(), 4, n_feat, o);
    fwrite(best_median.data(), 4, n_feat, o);
    fwrite(out_desc.data(), 32, n_feat, o);

    // an empty batch is valid and launches nothing
    const int32_t rc_empty =
        plvi_distinctive_descriptors_batch(0, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    // a list above the limit and a decreasing offset are refused before anything is launched
    const std::vector<int32_t> zeros(PLVI_DISTINCTIVE_MAX_OBS + 1, 0);
    const int32_t long_off[2] = {0, PLVI_DISTINCTIVE_MAX_OBS + 1}, bad_off[3] = {0, 2, 1};
    int32_t bp[2], bm[2];
    const int32_t rc_long = plvi_distinctive_descriptors(pool.data(), pool_rows, long_off, zeros.data(), 1, bp, bm, nullptr);
    const int32_t rc_bad = plvi_distinctive_descriptors(pool.data(), pool_rows, bad_off, zeros.data(), 2, bp, bm, nullptr);
    fwrite(&rc_empty, 4, 1, o);
    fwrite(&rc_long, 4, 1, o);
    fwrite(&rc_bad, 4, 1, o);
    fclose(o);
    return 0;
}
