// covis_capi_check.cpp — a C++11 caller of the plvi_covis_* entry points through
// include/plvi_frontend.h only, the way the INTEGRATION.md shims of KeyFrame::UpdateConnections call
// them.  Usage: covis_capi_check --sizes | covis_capi_check <in.bin> <out.bin>
//
// --sizes prints the header's constants and struct sizes (no device needed): PLVI_COVIS_LDS_KF,
// PLVI_COVIS_MAX_CONN, PLVI_COVIS_TH, PLVI_COVIS_MAX_QUERIES, sizeof(plvi_covis_keyframes),
// sizeof(plvi_covis_outputs).
//
// Both files are sequences of blocks: int32 byte count, then the bytes.
// in.bin (written by tests/test_covis_capi_native.py): a header of int32 kf_cap, n_order, kp_cap,
// kl_cap, n_mp, n_ml, conn_cap, n_queries; then kf_bad, order, kf_mp, nmp, kf_ml, nml, init_kf,
// first_conn, parent, mp_bad, mp_obs_off, mp_obs_kf, ml_bad, ml_obs_off, ml_obs_kf, q_slot.
// out.bin: twice -- the host form (plvi_covis_update, query by query) and ONE plvi_covis_update_batch
// over device tables, each on a graph of its own -- a block of int32 [n_queries][6] (n_counted,
// n_conn, kf_max, w_max, new_parent, err), first_conn, parent, covis, and per slot a block of int32
// n_map, n_ord, err and the four tables of plvi_covis_download; then a block of six int32: the
// statuses of a slot named twice, a slot out of range, an empty batch and a conn_cap above the
// limit, then GetWeight(q[0], q[1]) and the length of GetCovisiblesByWeight(q[0], 15) through the
// batch getters.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plvi_frontend.h"

namespace {

FILE *g_in, *g_out;

std::vector<char> take() {
    int32_t n = 0;
    if (fread(&n, 4, 1, g_in) != 1 || n < 0) exit(3);
    std::vector<char> v((size_t)n + 8, 0);
    if (n && fread(v.data(), 1, (size_t)n, g_in) != (size_t)n) exit(3);
    return v;
}

void put(const void* p, size_t bytes) {
    const int32_t n = (int32_t)bytes;
    fwrite(&n, 4, 1, g_out);
    if (bytes) fwrite(p, 1, bytes, g_out);
}

template <class T>
const T* as(const std::vector<char>& v) {
    return reinterpret_cast<const T*>(v.data());
}

struct Dev {
    void* p;
    Dev(const void* src, size_t bytes) : p(nullptr) {
        if (plvi_device_malloc(&p, bytes ? bytes : 4)) exit(4);
        if (src && bytes && plvi_memcpy(p, src, bytes, 1)) exit(4);
    }
    ~Dev() { plvi_device_free(p); }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    template <class T>
    std::vector<T> down(size_t n) const {
        std::vector<T> v(n ? n : 1);
        if (n && plvi_memcpy(v.data(), p, n * sizeof(T), 2)) exit(4);
        return v;
    }
};

void put_graph(plvi_covis_graph* g, int K, int C) {
    std::vector<int> mk(C), mw(C), ok(C), ow(C);
    for (int s = 0; s < K; ++s) {
        int n[3] = {0, 0, 0};
        if (plvi_covis_download(g, s, mk.data(), mw.data(), &n[0], ok.data(), ow.data(), &n[1], &n[2])) exit(5);
        put(n, sizeof n);
        put(mk.data(), 4 * (size_t)n[0]);
        put(mw.data(), 4 * (size_t)n[0]);
        put(ok.data(), 4 * (size_t)n[1]);
        put(ow.data(), 4 * (size_t)n[1]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--sizes")) {
        printf("%d %d %d %d %zu %zu\n", PLVI_COVIS_LDS_KF, PLVI_COVIS_MAX_CONN, PLVI_COVIS_TH, PLVI_COVIS_MAX_QUERIES,
               sizeof(plvi_covis_keyframes), sizeof(plvi_covis_outputs));
        return 0;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: %s --sizes | in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) return 3;
    const std::vector<char> hd = take();
    const int32_t* h = as<int32_t>(hd);
    const int K = h[0], n_order = h[1], kp_cap = h[2], kl_cap = h[3], n_mp = h[4], n_ml = h[5], C = h[6], B = h[7];
    const std::vector<char> kf_bad = take(), order = take(), kf_mp = take(), nmp = take(), kf_ml = take(), nml = take(),
                            init_kf = take(), first0 = take(), parent0 = take(), mp_bad = take(), mp_off = take(),
                            mp_obs = take(), ml_bad = take(), ml_off = take(), ml_obs = take(), qv = take();
    const int* q = as<int>(qv);

    // ---- the host form, query by query
    {
        plvi_covis_graph* g = nullptr;
        if (plvi_covis_create(K, C, 0, &g)) return 5;
        std::vector<uint8_t> first(as<uint8_t>(first0), as<uint8_t>(first0) + K);
        std::vector<int> parent(as<int>(parent0), as<int>(parent0) + K), covis((size_t)K * PLVI_KFDB_NEIGHBOURS, -7);
        plvi_covis_keyframes kf;
        memset(&kf, 0, sizeof kf);
        kf.kf_cap = K;
        kf.n_order = n_order;
        kf.kp_cap = kp_cap;
        kf.kl_cap = kl_cap;
        kf.bad = as<uint8_t>(kf_bad);
        kf.order = as<int>(order);
        kf.mp = as<int>(kf_mp);
        kf.nmp = as<int>(nmp);
        kf.ml = as<int>(kf_ml);
        kf.nml = as<int>(nml);
        kf.init_kf = as<uint8_t>(init_kf);
        kf.first_conn = first.data();
        kf.parent = parent.data();
        kf.covis = covis.data();
        plvi_local_map_pool mp, ml;
        memset(&mp, 0, sizeof mp);
        memset(&ml, 0, sizeof ml);
        mp.n = n_mp;
        mp.bad = as<uint8_t>(mp_bad);
        mp.obs_off = as<int>(mp_off);
        mp.obs_kf = as<int>(mp_obs);
        ml.n = n_ml;
        ml.bad = as<uint8_t>(ml_bad);
        ml.obs_off = as<int>(ml_off);
        ml.obs_kf = as<int>(ml_obs);
        std::vector<int> res((size_t)B * 6, -7);
        for (int i = 0; i < B; ++i) {
            int* r = res.data() + 6 * (size_t)i;
            plvi_covis_outputs out = {r, r + 1, r + 2, r + 3, r + 4, r + 5};
            if (plvi_covis_update(g, q[i], &kf, &mp, &ml, &out)) return 6;
        }
        put(res.data(), 4 * res.size());
        put(first.data(), first.size());
        put(parent.data(), 4 * parent.size());
        put(covis.data(), 4 * covis.size());
        put_graph(g, K, C);
        plvi_covis_destroy(g);
    }

    // ---- the batch form over device tables
    plvi_covis_graph* g = nullptr;
    if (plvi_covis_create(K, C, 0, &g)) return 5;
    std::vector<int> covis0((size_t)K * PLVI_KFDB_NEIGHBOURS, -7), res0((size_t)B * 6 + 6, -7);
    const size_t Ks = (size_t)K;
    Dev d_bad(kf_bad.data(), Ks), d_order(order.data(), 4 * (size_t)n_order), d_kmp(kf_mp.data(), 4 * Ks * kp_cap),
        d_nmp(nmp.data(), 4 * Ks), d_kml(kf_ml.data(), 4 * Ks * kl_cap), d_nml(nml.data(), 4 * Ks),
        d_init(init_kf.data(), Ks), d_first(first0.data(), Ks), d_parent(parent0.data(), 4 * Ks),
        d_covis(covis0.data(), 4 * covis0.size()), d_mbad(mp_bad.data(), (size_t)n_mp),
        d_moff(mp_off.data(), 4 * ((size_t)n_mp + 1)), d_mobs(mp_obs.data(), 4 * (size_t)as<int>(mp_off)[n_mp]),
        d_lbad(ml_bad.data(), (size_t)n_ml), d_loff(ml_off.data(), 4 * ((size_t)n_ml + 1)),
        d_lobs(ml_obs.data(), 4 * (size_t)as<int>(ml_off)[n_ml]), d_res(res0.data(), 4 * res0.size());
    plvi_covis_keyframes kf;
    memset(&kf, 0, sizeof kf);
    kf.kf_cap = K;
    kf.n_order = n_order;
    kf.kp_cap = kp_cap;
    kf.kl_cap = kl_cap;
    kf.bad = d_bad.as<uint8_t>();
    kf.order = d_order.as<int>();
    kf.mp = d_kmp.as<int>();
    kf.nmp = d_nmp.as<int>();
    kf.ml = d_kml.as<int>();
    kf.nml = d_nml.as<int>();
    kf.init_kf = d_init.as<uint8_t>();
    kf.first_conn = d_first.as<uint8_t>();
    kf.parent = d_parent.as<int>();
    kf.covis = d_covis.as<int>();
    plvi_local_map_pool mp, ml;
    memset(&mp, 0, sizeof mp);
    memset(&ml, 0, sizeof ml);
    mp.n = n_mp;
    mp.bad = d_mbad.as<uint8_t>();
    mp.obs_off = d_moff.as<int>();
    mp.obs_kf = d_mobs.as<int>();
    ml.n = n_ml;
    ml.bad = d_lbad.as<uint8_t>();
    ml.obs_off = d_loff.as<int>();
    ml.obs_kf = d_lobs.as<int>();
    // struct-of-arrays outputs: six rows of B + 1 ints
    int* r = d_res.as<int>();
    const int stride = B + 1;
    plvi_covis_outputs out = {r, r + stride, r + 2 * stride, r + 3 * stride, r + 4 * stride, r + 5 * stride};
    const size_t sb = plvi_covis_scratch_bytes(B, K);
    Dev scratch(nullptr, sb);
    if (plvi_covis_update_batch(g, B, q, &kf, &mp, &ml, &out, scratch.p, sb, nullptr)) return 7;
    if (plvi_device_synchronize()) return 7;
    const std::vector<int> rows = d_res.down<int>(res0.size());
    std::vector<int> res((size_t)B * 6);
    for (int i = 0; i < B; ++i)
        for (int k = 0; k < 6; ++k) res[6 * (size_t)i + k] = rows[(size_t)k * stride + i];
    put(res.data(), 4 * res.size());
    put(d_first.down<uint8_t>(Ks).data(), Ks);
    put(d_parent.down<int>(Ks).data(), 4 * Ks);
    put(d_covis.down<int>(covis0.size()).data(), 4 * covis0.size());
    put_graph(g, K, C);

    // ---- statuses and the getters
    int st[6];
    const int twice[2] = {q[0], q[0]}, outside[1] = {K};
    st[0] = plvi_covis_update_batch(g, 2, twice, &kf, &mp, &ml, &out, scratch.p, sb, nullptr);
    st[1] = plvi_covis_update_batch(g, 1, outside, &kf, &mp, &ml, &out, scratch.p, sb, nullptr);
    st[2] = plvi_covis_update_batch(g, 0, nullptr, &kf, &mp, &ml, &out, nullptr, 0, nullptr);
    plvi_covis_graph* g2 = nullptr;
    st[3] = plvi_covis_create(K, PLVI_COVIS_MAX_CONN + 1, 0, &g2);
    const int ab[3] = {q[0], q[1], 15};
    Dev d_ab(ab, sizeof ab), d_get(nullptr, 8);
    if (plvi_covis_weight_batch(g, 1, d_ab.as<int>(), d_ab.as<int>() + 1, d_get.as<int>(), nullptr)) return 8;
    if (plvi_covis_by_weight_batch(g, 1, d_ab.as<int>(), d_ab.as<int>() + 2, d_get.as<int>() + 1, nullptr)) return 8;
    if (plvi_device_synchronize()) return 8;
    const std::vector<int> got = d_get.down<int>(2);
    st[4] = got[0];
    st[5] = got[1];
    put(st, sizeof st);
    plvi_covis_destroy(g);
    fclose(g_out);
    return 0;
}
