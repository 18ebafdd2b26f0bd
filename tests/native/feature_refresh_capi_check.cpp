// feature_refresh_capi_check.cpp — a C++11 caller of plvi_feature_refresh[_batch] that includes only
// include/plvi_frontend.h, the way a shim of UpdateNormalAndDepth + ComputeDistinctiveDescriptors does.
//   feature_refresh_capi_check --sizes          prints the header's constants and struct sizes
//   feature_refresh_capi_check in.bin out.bin   runs both forms on the tables of in.bin (blocks of [int bytes][bytes],
//                                               see tests/test_feature_refresh_capi_native.py) and writes every
//                                               output, then the status of a few refused calls.
#include <cstdio>
#include <cstring>
#include <vector>

#include "plvi_frontend.h"

namespace {

typedef std::vector<unsigned char> Bytes;

std::vector<Bytes> read_blocks(const char* path) {
    std::vector<Bytes> blocks;
    FILE* f = fopen(path, "rb");
    if (!f) return blocks;
    int n;
    while (fread(&n, 4, 1, f) == 1) {
        Bytes b(n);
        if (n && fread(b.data(), 1, n, f) != (size_t)n) break;
        blocks.push_back(b);
    }
    fclose(f);
    return blocks;
}

void put(FILE* f, const void* p, size_t bytes) {
    const int n = (int)bytes;
    fwrite(&n, 4, 1, f);
    if (n) fwrite(p, 1, n, f);
}
void put(FILE* f, const Bytes& b) { put(f, b.data(), b.size()); }
void put(FILE* f, const std::vector<int>& v) { put(f, v.data(), 4 * v.size()); }

template <class T>
const T* ptr(const Bytes& b) { return reinterpret_cast<const T*>(b.data()); }
template <class T>
T* ptr(Bytes& b) { return reinterpret_cast<T*>(b.data()); }

struct Dev {
    std::vector<void*> all;
    bool ok = true;
    void* up(const void* src, size_t bytes) {
        void* d = nullptr;
        if (plvi_device_malloc(&d, bytes ? bytes : 1) != 0) ok = false;
        all.push_back(d);
        if (d && src && bytes && plvi_memcpy(d, src, bytes, 1) != 0) ok = false;  // no src: scratch
        return d;
    }
    void* up(const Bytes& b) { return up(b.data(), b.size()); }
    void down(Bytes& dst, const void* d) {
        if (dst.size() && plvi_memcpy(dst.data(), d, dst.size(), 2) != 0) ok = false;
    }
    ~Dev() {
        for (size_t i = 0; i < all.size(); ++i)
            if (all[i]) plvi_device_free(all[i]);
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--sizes")) {
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d\n", PLVI_REFRESH_POINTS, PLVI_REFRESH_LINES, PLVI_REFRESH_NORMAL,
               PLVI_REFRESH_DESC, PLVI_REFRESH_ERR_ROWS, PLVI_REFRESH_ERR_REF, PLVI_REFRESH_ERR_LEVEL,
               PLVI_REFRESH_ERR_KEYPOINT, PLVI_REFRESH_MAX_LEVELS, PLVI_COMPAT_SCALEADD_FMA,
               (int)sizeof(plvi_refresh_keyframes), (int)sizeof(plvi_refresh_params), (int)sizeof(plvi_refresh_outputs));
        return 0;
    }
    if (argc != 3) return 2;
    // blocks: header ints, scale, kf bad / ow / cnt / info / desc, feature bad / obs_off / obs_kf / obs_idx / ref_kf /
    // pos, the columns normal / dist / desc, ids
    std::vector<Bytes> b = read_blocks(argv[1]);
    if (b.size() != 17) return 3;
    const int* h = ptr<int>(b[0]);
    const int kf_cap = h[0], cap = h[1], n = h[2], n_ids = h[3], max_obs = h[4], row_cap = h[5], compat = h[6],
              n_levels = h[7];
    plvi_refresh_params prm;
    memset(&prm, 0, sizeof prm);
    prm.kind = PLVI_REFRESH_POINTS, prm.what = PLVI_REFRESH_NORMAL | PLVI_REFRESH_DESC, prm.n_levels = n_levels;
    prm.max_obs = max_obs, prm.row_cap = row_cap, prm.compat = compat;
    memcpy(prm.scale, b[1].data(), 4 * (size_t)n_levels);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;

    for (int form = 0; form < 2; ++form) {  // 0: the host form, 1: the device form
        Bytes normal = b[13], dist = b[14], desc = b[15];
        Bytes state((size_t)n_ids, 0x55), best_pos(4 * (size_t)n_ids, 0x55), best_median(4 * (size_t)n_ids, 0x55);
        std::vector<int> scalars(2, -7);
        int rc;
        if (form == 0) {
            plvi_refresh_keyframes kf = {kf_cap, cap, b[2].data(), ptr<float>(b[3]), ptr<int>(b[4]), b[5].data(),
                                         b[6].data()};
            plvi_local_map_pool pool;
            memset(&pool, 0, sizeof pool);
            pool.n = n, pool.bad = b[7].data(), pool.obs_off = ptr<int>(b[8]), pool.obs_kf = ptr<int>(b[9]);
            pool.pos = ptr<float>(b[12]);
            plvi_ba_features feat = {ptr<int>(b[10]), nullptr};
            plvi_eg_features ref = {ptr<int>(b[11]), nullptr, nullptr, nullptr};
            plvi_refresh_outputs o = {ptr<float>(normal), ptr<float>(dist), desc.data(), state.data(),
                                      ptr<int>(best_pos), ptr<int>(best_median), &scalars[0], &scalars[1]};
            rc = plvi_feature_refresh(&kf, &pool, &feat, &ref, &prm, ptr<int>(b[16]), n_ids, &o);
        } else {
            Dev d;
            plvi_refresh_keyframes kf = {kf_cap, cap, (const uint8_t*)d.up(b[2]), (const float*)d.up(b[3]),
                                         (const int*)d.up(b[4]), (const uint8_t*)d.up(b[5]), (const uint8_t*)d.up(b[6])};
            plvi_local_map_pool pool;
            memset(&pool, 0, sizeof pool);
            pool.n = n, pool.bad = (const uint8_t*)d.up(b[7]), pool.obs_off = (const int*)d.up(b[8]);
            pool.obs_kf = (const int*)d.up(b[9]), pool.pos = (const float*)d.up(b[12]);
            plvi_ba_features feat = {(const int*)d.up(b[10]), nullptr};
            plvi_eg_features ref = {(const int*)d.up(b[11]), nullptr, nullptr, nullptr};
            // the pool's own columns, written in place through the outputs
            pool.normal = (const float*)d.up(normal), pool.dist = (const float*)d.up(dist);
            pool.desc = (const uint8_t*)d.up(desc);
            int* d_scalars = (int*)d.up(scalars.data(), 8);
            plvi_refresh_outputs o = {const_cast<float*>(pool.normal), const_cast<float*>(pool.dist),
                                      const_cast<uint8_t*>(pool.desc), (uint8_t*)d.up(state),
                                      (int*)d.up(best_pos), (int*)d.up(best_median), d_scalars, d_scalars + 1};
            const size_t sb = plvi_feature_refresh_scratch_bytes(n_ids, row_cap);
            void* scratch = d.up(nullptr, sb);
            const int* d_ids = (const int*)d.up(b[16]);
            rc = plvi_feature_refresh_batch(&kf, &pool, &feat, &ref, &prm, d_ids, n_ids, &o, scratch, sb, nullptr);
            if (plvi_device_synchronize() != 0) d.ok = false;
            d.down(normal, o.normal), d.down(dist, o.dist), d.down(desc, o.desc), d.down(state, o.state);
            d.down(best_pos, o.best_pos), d.down(best_median, o.best_median);
            if (plvi_memcpy(scalars.data(), d_scalars, 8, 2) != 0 || !d.ok) return 5;
            if (form == 1) {  // refusals, nothing launched
                std::vector<int> refused;
                plvi_refresh_params bad = prm;
                bad.what = 0;
                refused.push_back(plvi_feature_refresh_batch(&kf, &pool, &feat, &ref, &bad, d_ids, n_ids, &o, scratch, sb, nullptr));
                bad = prm, bad.kind = 2;
                refused.push_back(plvi_feature_refresh_batch(&kf, &pool, &feat, &ref, &bad, d_ids, n_ids, &o, scratch, sb, nullptr));
                bad = prm, bad.max_obs = PLVI_DISTINCTIVE_MAX_OBS + 1;
                refused.push_back(plvi_feature_refresh_batch(&kf, &pool, &feat, &ref, &bad, d_ids, n_ids, &o, scratch, sb, nullptr));
                bad = prm, bad.n_levels = PLVI_REFRESH_MAX_LEVELS + 1;
                refused.push_back(plvi_feature_refresh_batch(&kf, &pool, &feat, &ref, &bad, d_ids, n_ids, &o, scratch, sb, nullptr));
                refused.push_back(plvi_feature_refresh_batch(&kf, &pool, &feat, &ref, &prm, d_ids, n_ids, &o, scratch, sb - 1, nullptr));
                refused.push_back(plvi_feature_refresh_batch(&kf, &pool, &feat, nullptr, &prm, d_ids, n_ids, &o, scratch, sb, nullptr));
                refused.push_back((int)plvi_feature_refresh_scratch_bytes(-1, 4));
                refused.push_back((int)sb);
                put(out, std::vector<int>(1, rc));
                put(out, scalars), put(out, normal), put(out, dist), put(out, desc), put(out, state);
                put(out, best_pos), put(out, best_median), put(out, refused);
                continue;
            }
        }
        put(out, std::vector<int>(1, rc));
        put(out, scalars), put(out, normal), put(out, dist), put(out, desc), put(out, state);
        put(out, best_pos), put(out, best_median);
    }
    fclose(out);
    return 0;
}
