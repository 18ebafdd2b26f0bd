// gba_propagate_capi_check.cpp — a C++11 caller of plvi_gba_walk[_device] and plvi_gba_correct[_device] that
// includes only include/plvi_frontend.h, the way a shim of RunGlobalBundleAdjustment's second half does.
//   gba_propagate_capi_check --sizes          prints the header's constants and struct sizes
//   gba_propagate_capi_check in.bin out.bin   runs both forms of both calls on the tables of in.bin (blocks of
//                                             [int bytes][bytes], see tests/test_gba_propagate_capi_native.py) and
//                                             writes every output, then the status of a few refused calls.
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
        printf("%d %d %d %d %d %d %d %d %d %d %d\n", PLVI_GBA_POINTS, PLVI_GBA_LINES, PLVI_GBA_ERR_ORIGIN,
               PLVI_GBA_ERR_CYCLE, PLVI_GBA_ERR_WALK, PLVI_GBA_ERR_REF, PLVI_COMPAT_GEMM_FMA,
               (int)sizeof(plvi_gba_walk_outputs), (int)sizeof(plvi_gba_poses), (int)sizeof(plvi_gba_params),
               (int)sizeof(plvi_gba_correct_outputs));
        return 0;
    }
    if (argc != 3) return 2;
    // blocks: header ints; keyframes bad / order / child_off / child; origins; kf_ba_for; features bad / ref_kf /
    // map_id / ba_for / pos_gba / pos; poses kf_ba_for / has_bef / tcw_bef / twc
    std::vector<Bytes> b = read_blocks(argv[1]);
    if (b.size() != 17) return 3;
    const int* h = ptr<int>(b[0]);
    const int kf_cap = h[0], n_order = h[1], n_origins = h[2], n = h[4], walk_cap = h[7];
    const unsigned loop_kf = (unsigned)h[3];
    plvi_gba_params prm = {PLVI_GBA_POINTS, loop_kf, h[5], h[6]};
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;

    for (int form = 0; form < 2; ++form) {  // 0: the host forms, 1: the device forms
        Bytes stamps = b[6], pos = b[12];
        Bytes walk(4 * (size_t)walk_cap, 0x55), parent(4 * (size_t)walk_cap, 0x55), is_new((size_t)walk_cap, 0x55);
        Bytes visited((size_t)kf_cap, 0), state((size_t)n, 0x55);
        std::vector<int> ws(3, -7), cs(4, -7);
        int rc_walk, rc_correct;
        plvi_cull_keyframes kf;
        plvi_eg_keyframes eg;
        plvi_local_map_pool pool;
        plvi_eg_features feat;
        memset(&kf, 0, sizeof kf), memset(&eg, 0, sizeof eg), memset(&pool, 0, sizeof pool), memset(&feat, 0, sizeof feat);
        kf.kf_cap = kf_cap, eg.n_order = n_order, pool.n = n;
        if (form == 0) {
            kf.bad = b[1].data();
            eg.order = ptr<int>(b[2]), eg.child_off = ptr<int>(b[3]), eg.child = ptr<int>(b[4]);
            plvi_gba_walk_outputs wo = {walk_cap, ptr<int>(walk), ptr<int>(parent), is_new.data(), &ws[0], &ws[1],
                                        &ws[2], visited.data()};
            rc_walk = plvi_gba_walk(&kf, &eg, ptr<int>(b[5]), n_origins, loop_kf, ptr<unsigned>(stamps), &wo);
            pool.bad = b[7].data(), pool.pos = ptr<float>(pos);
            feat.ref_kf = ptr<int>(b[8]), feat.map_id = ptr<int>(b[9]);
            plvi_gba_poses poses = {kf_cap, ptr<unsigned>(b[13]), b[14].data(), ptr<float>(b[15]), ptr<float>(b[16])};
            plvi_gba_correct_outputs co = {ptr<float>(pos), nullptr, state.data(), &cs[0], &cs[3]};  // in place
            rc_correct = plvi_gba_correct(&pool, &feat, ptr<unsigned>(b[10]), b[11].data(), &poses, &prm, &co);
        } else {
            Dev d;
            kf.bad = (const uint8_t*)d.up(b[1]);
            eg.order = (const int*)d.up(b[2]), eg.child_off = (const int*)d.up(b[3]), eg.child = (const int*)d.up(b[4]);
            unsigned* d_stamps = (unsigned*)d.up(stamps);
            int* d_ws = (int*)d.up(ws.data(), 12);
            plvi_gba_walk_outputs wo = {walk_cap, (int*)d.up(walk), (int*)d.up(parent), (uint8_t*)d.up(is_new),
                                        d_ws, d_ws + 1, d_ws + 2, (uint8_t*)d.up(visited)};
            const size_t sb = plvi_gba_walk_scratch_bytes(kf_cap);
            void* scratch = d.up(nullptr, sb);
            const int* d_origins = (const int*)d.up(b[5]);
            rc_walk = plvi_gba_walk_device(&kf, &eg, d_origins, n_origins, loop_kf, d_stamps, &wo, scratch, sb, nullptr);
            pool.bad = (const uint8_t*)d.up(b[7]), pool.pos = (const float*)d.up(pos);
            feat.ref_kf = (const int*)d.up(b[8]), feat.map_id = (const int*)d.up(b[9]);
            plvi_gba_poses poses = {kf_cap, (const unsigned*)d.up(b[13]), (const uint8_t*)d.up(b[14]),
                                    (const float*)d.up(b[15]), (const float*)d.up(b[16])};
            int* d_cs = (int*)d.up(cs.data(), 16);
            // the pool's own column, written in place through the outputs
            plvi_gba_correct_outputs co = {const_cast<float*>(pool.pos), nullptr, (uint8_t*)d.up(state), d_cs, d_cs + 3};
            const unsigned* d_ba = (const unsigned*)d.up(b[10]);
            const void* d_gba = d.up(b[11]);
            rc_correct = plvi_gba_correct_device(&pool, &feat, d_ba, d_gba, &poses, &prm, &co, nullptr);
            if (plvi_device_synchronize() != 0) d.ok = false;
            d.down(walk, wo.walk), d.down(parent, wo.walk_parent), d.down(is_new, wo.walk_new);
            d.down(visited, wo.visited), d.down(stamps, d_stamps), d.down(pos, co.pos), d.down(state, co.state);
            if (plvi_memcpy(ws.data(), d_ws, 12, 2) != 0 || plvi_memcpy(cs.data(), d_cs, 16, 2) != 0 || !d.ok) return 5;
            // refusals, nothing launched
            std::vector<int> refused;
            refused.push_back(plvi_gba_walk_device(&kf, &eg, d_origins, n_origins, loop_kf, d_stamps, &wo, scratch, sb - 1, nullptr));
            refused.push_back(plvi_gba_walk_device(&kf, &eg, d_origins, -1, loop_kf, d_stamps, &wo, scratch, sb, nullptr));
            plvi_eg_keyframes part = eg;
            part.child = nullptr;
            refused.push_back(plvi_gba_walk_device(&kf, &part, d_origins, n_origins, loop_kf, d_stamps, &wo, scratch, sb, nullptr));
            plvi_gba_params bad = prm;
            bad.kind = 2;
            refused.push_back(plvi_gba_correct_device(&pool, &feat, d_ba, d_gba, &poses, &bad, &co, nullptr));
            refused.push_back(plvi_gba_correct_device(&pool, &feat, nullptr, d_gba, &poses, &prm, &co, nullptr));
            refused.push_back((int)plvi_gba_walk_scratch_bytes(-1));
            refused.push_back((int)sb);
            put(out, refused);
        }
        put(out, std::vector<int>(1, rc_walk));
        put(out, ws), put(out, walk), put(out, parent), put(out, is_new), put(out, visited), put(out, stamps);
        put(out, std::vector<int>(1, rc_correct));
        put(out, cs), put(out, pos), put(out, state);
    }
    fclose(out);
    return 0;
}
