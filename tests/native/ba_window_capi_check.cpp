// ba_window_capi_check.cpp — a C++11 caller of plvi_ba_window[_batch] that includes only include/plvi_frontend.h,
// the way the INTEGRATION.md shim of Optimizer::LocalBundleAdjustment does.
//
// --sizes prints the header's constants and struct sizes (no device needed): PLVI_BA_LDS_KF, PLVI_BA_MAX_OPT,
// PLVI_BA_MAX_FIXED_INERTIAL, PLVI_BA_INERTIAL, PLVI_BA_EDGE_LINE, PLVI_BA_ERR_QUERY, sizeof of the four structs.
//
// IN OUT: IN is a sequence of blocks, each an int32 byte count and the bytes --
//   ints   kf_cap kp_cap cand_stride mp_n q_slot lkf_cap fkf_cap feat_cap edge_cap
//   then   bad init_kf mp nmp kp_info cand n_cand kf_id kf_map_id  mp_bad mp_obs_off mp_obs_kf mp_obs_idx mp_map_id
// PLVI_BA_POINTS runs once through the host form and once through the batch form on device copies, into tables
// filled with -7 (edge_kind 121); OUT gets, per form, the blocks
//   ints n_local_kf n_fixed_kf num_fixed init_in_local non_fixed n_local_feat n_mono n_stereo n_line err
//   | local_kf | fixed_kf | local_feat | edge_feat | edge_kf | edge_idx | edge_cam | edge_kind
// and last a block of statuses: the batch form without its scratch, with a scratch one byte short, with n_queries
// 65536, with mode 7, and plvi_ba_window_scratch_bytes(2, kf_cap, mp_n, 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "plvi_frontend.h"

typedef std::vector<unsigned char> Bytes;

static bool take(FILE* f, Bytes& b) {
    int n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return false;
    b.resize(n);
    return n == 0 || fread(b.data(), 1, n, f) == (size_t)n;
}

static void put(FILE* f, const void* p, size_t bytes) {
    const int n = (int)bytes;
    fwrite(&n, 4, 1, f);
    fwrite(p, 1, bytes, f);
}

template <class T>
static const T* as(const Bytes& b) {
    return b.empty() ? NULL : reinterpret_cast<const T*>(b.data());
}

struct Dev {  // device copies, freed at exit
    std::vector<void*> all;
    template <class T>
    T* up(const void* host, size_t bytes) {
        void* d = NULL;
        if (plvi_device_malloc(&d, bytes ? bytes : 4) != PLVI_OK) exit(3);
        all.push_back(d);
        if (host && bytes && plvi_memcpy(d, host, bytes, 1) != PLVI_OK) exit(3);
        return static_cast<T*>(d);
    }
    template <class T>
    const T* up(const Bytes& b) { return b.empty() ? NULL : up<T>(b.data(), b.size()); }
    ~Dev() {
        for (size_t i = 0; i < all.size(); ++i) plvi_device_free(all[i]);
    }
};

struct Out {  // one query's outputs on the host, pre-filled
    std::vector<int> scal, local_kf, fixed_kf, local_feat, edge_feat, edge_kf, edge_idx, edge_cam;
    std::vector<unsigned char> edge_kind;
    Out(const int* caps)
        : scal(10, -7), local_kf(caps[0] ? caps[0] : 1, -7), fixed_kf(caps[1] ? caps[1] : 1, -7),
          local_feat(caps[2] ? caps[2] : 1, -7), edge_feat(caps[3] ? caps[3] : 1, -7), edge_kf(edge_feat),
          edge_idx(edge_feat), edge_cam(edge_feat), edge_kind(edge_feat.size(), 121) {}
    void write(FILE* f) const {
        put(f, scal.data(), 4 * scal.size());
        const std::vector<int>* v[] = {&local_kf, &fixed_kf, &local_feat, &edge_feat, &edge_kf, &edge_idx, &edge_cam};
        for (size_t i = 0; i < 7; ++i) put(f, v[i]->data(), 4 * v[i]->size());
        put(f, edge_kind.data(), edge_kind.size());
    }
};

static void point_scalars(plvi_ba_outputs& o, int* s) {
    o.n_local_kf = s + 0;
    o.n_fixed_kf = s + 1;
    o.num_fixed = s + 2;
    o.init_in_local = s + 3;
    o.non_fixed = s + 4;
    o.n_local_feat = s + 5;
    o.n_mono = s + 6;
    o.n_stereo = s + 7;
    o.n_line = s + 8;
    o.err = s + 9;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--sizes")) {
        printf("%d %d %d %d %d %d %zu %zu %zu %zu\n", PLVI_BA_LDS_KF, PLVI_BA_MAX_OPT, PLVI_BA_MAX_FIXED_INERTIAL,
               (int)PLVI_BA_INERTIAL, (int)PLVI_BA_EDGE_LINE, (int)PLVI_BA_ERR_QUERY, sizeof(plvi_ba_features),
               sizeof(plvi_ba_params), sizeof(plvi_ba_queries), sizeof(plvi_ba_outputs));
        return 0;
    }
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    Bytes ints, b[14];
    if (!take(in, ints) || ints.size() != 9 * 4) return 2;
    for (int i = 0; i < 14; ++i)
        if (!take(in, b[i])) return 2;
    fclose(in);
    const int* I = as<int>(ints);
    const int kf_cap = I[0], kp_cap = I[1], cand_stride = I[2], mp_n = I[3], q_slot = I[4];
    const int* caps = I + 5;
    const int n_kf_in_map = 0;

    plvi_cull_keyframes kf;
    memset(&kf, 0, sizeof kf);
    kf.kf_cap = kf_cap;
    kf.kp_cap = kp_cap;
    kf.cand_stride = cand_stride;
    kf.bad = as<uint8_t>(b[0]);
    kf.init_kf = as<uint8_t>(b[1]);
    kf.mp = as<int>(b[2]);
    kf.nmp = as<int>(b[3]);
    kf.kp_info = as<uint8_t>(b[4]);
    kf.cand = as<int>(b[5]);
    kf.n_cand = as<int>(b[6]);
    kf.kf_id = as<unsigned>(b[7]);
    const int* kf_map = as<int>(b[8]);
    plvi_local_map_pool mp;
    memset(&mp, 0, sizeof mp);
    mp.n = mp_n;
    mp.bad = as<uint8_t>(b[9]);
    mp.obs_off = as<int>(b[10]);
    mp.obs_kf = as<int>(b[11]);
    plvi_ba_features fmp = {as<int>(b[12]), as<int>(b[13])};
    plvi_ba_params params = {PLVI_BA_POINTS, 10};
    plvi_ba_queries qs = {&q_slot, &n_kf_in_map};

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;

    // ---- the host form
    Out h(caps);
    plvi_ba_outputs ho;
    memset(&ho, 0, sizeof ho);
    ho.lkf_cap = caps[0];
    ho.fkf_cap = caps[1];
    ho.feat_cap = caps[2];
    ho.edge_cap = caps[3];
    point_scalars(ho, h.scal.data());
    ho.local_kf = h.local_kf.data();
    ho.fixed_kf = h.fixed_kf.data();
    ho.local_feat = h.local_feat.data();
    ho.edge_feat = h.edge_feat.data();
    ho.edge_kf = h.edge_kf.data();
    ho.edge_idx = h.edge_idx.data();
    ho.edge_cam = h.edge_cam.data();
    ho.edge_kind = h.edge_kind.data();
    int rc = plvi_ba_window(&kf, kf_map, &mp, &fmp, NULL, NULL, &params, &qs, &ho);
    if (rc != PLVI_OK && rc != PLVI_E_CAPACITY) return 4;
    h.write(out);

    // ---- the batch form on device copies
    Dev dev;
    plvi_cull_keyframes dk = kf;
    dk.bad = dev.up<uint8_t>(b[0]);
    dk.init_kf = dev.up<uint8_t>(b[1]);
    dk.mp = dev.up<int>(b[2]);
    dk.nmp = dev.up<int>(b[3]);
    dk.kp_info = dev.up<uint8_t>(b[4]);
    dk.cand = dev.up<int>(b[5]);
    dk.n_cand = dev.up<int>(b[6]);
    dk.kf_id = dev.up<unsigned>(b[7]);
    const int* dmap = dev.up<int>(b[8]);
    plvi_local_map_pool dmp = mp;
    dmp.bad = dev.up<uint8_t>(b[9]);
    dmp.obs_off = dev.up<int>(b[10]);
    dmp.obs_kf = dev.up<int>(b[11]);
    plvi_ba_features dfmp = {dev.up<int>(b[12]), dev.up<int>(b[13])};
    plvi_ba_queries dq = {dev.up<int>(&q_slot, 4), dev.up<int>(&n_kf_in_map, 4)};
    Out d(caps);
    plvi_ba_outputs dout = ho;
    point_scalars(dout, dev.up<int>(d.scal.data(), 40));
    dout.local_kf = dev.up<int>(d.local_kf.data(), 4 * d.local_kf.size());
    dout.fixed_kf = dev.up<int>(d.fixed_kf.data(), 4 * d.fixed_kf.size());
    dout.local_feat = dev.up<int>(d.local_feat.data(), 4 * d.local_feat.size());
    dout.edge_feat = dev.up<int>(d.edge_feat.data(), 4 * d.edge_feat.size());
    dout.edge_kf = dev.up<int>(d.edge_kf.data(), 4 * d.edge_kf.size());
    dout.edge_idx = dev.up<int>(d.edge_idx.data(), 4 * d.edge_idx.size());
    dout.edge_cam = dev.up<int>(d.edge_cam.data(), 4 * d.edge_cam.size());
    dout.edge_kind = dev.up<uint8_t>(d.edge_kind.data(), d.edge_kind.size());
    const size_t sb = plvi_ba_window_scratch_bytes(1, kf_cap, mp_n, 0);
    void* scratch = dev.up<uint8_t>(NULL, sb);
    if (plvi_ba_window_batch(1, &dk, dmap, &dmp, &dfmp, NULL, NULL, &params, &dq, &dout, scratch, sb, NULL) != PLVI_OK)
        return 5;
    if (plvi_device_synchronize() != PLVI_OK) return 5;
    int* s = d.scal.data();
    plvi_memcpy(s, dout.n_local_kf, 40, 2);
    plvi_memcpy(d.local_kf.data(), dout.local_kf, 4 * d.local_kf.size(), 2);
    plvi_memcpy(d.fixed_kf.data(), dout.fixed_kf, 4 * d.fixed_kf.size(), 2);
    plvi_memcpy(d.local_feat.data(), dout.local_feat, 4 * d.local_feat.size(), 2);
    plvi_memcpy(d.edge_feat.data(), dout.edge_feat, 4 * d.edge_feat.size(), 2);
    plvi_memcpy(d.edge_kf.data(), dout.edge_kf, 4 * d.edge_kf.size(), 2);
    plvi_memcpy(d.edge_idx.data(), dout.edge_idx, 4 * d.edge_idx.size(), 2);
    plvi_memcpy(d.edge_cam.data(), dout.edge_cam, 4 * d.edge_cam.size(), 2);
    plvi_memcpy(d.edge_kind.data(), dout.edge_kind, d.edge_kind.size(), 2);
    d.write(out);

    // ---- refusals
    plvi_ba_params bad_mode = {7, 10};
    const int st[5] = {
        plvi_ba_window_batch(1, &dk, dmap, &dmp, &dfmp, NULL, NULL, &params, &dq, &dout, NULL, sb, NULL),
        plvi_ba_window_batch(1, &dk, dmap, &dmp, &dfmp, NULL, NULL, &params, &dq, &dout, scratch, sb - 1, NULL),
        plvi_ba_window_batch(65536, &dk, dmap, &dmp, &dfmp, NULL, NULL, &params, &dq, &dout, scratch, sb, NULL),
        plvi_ba_window_batch(1, &dk, dmap, &dmp, &dfmp, NULL, NULL, &bad_mode, &dq, &dout, scratch, sb, NULL),
        (int)plvi_ba_window_scratch_bytes(2, kf_cap, mp_n, 0)};
    put(out, st, sizeof st);
    fclose(out);
    return 0;
}
