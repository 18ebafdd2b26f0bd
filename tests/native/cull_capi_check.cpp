// cull_capi_check.cpp — a C++11 caller of plvi_keyframe_culling[_batch] that includes only
// include/plvi_frontend.h, the way the INTEGRATION.md shim of LocalMapping::KeyFrameCullingWithLines does.
//
// --sizes prints the header's constants and struct sizes (no device needed): PLVI_CULL_MAX_CHANGED,
// PLVI_CULL_SPEC, PLVI_CULL_NEEDS_NORM, PLVI_CULL_DEFERRED, PLVI_CULL_ERR_QUERY, sizeof of the five structs.
//
// IN OUT: IN is a sequence of blocks, each an int32 byte count and the bytes --
//   ints   kf_cap kp_cap kl_cap cand_stride mp_n ml_n q_slot n_kf_in_map out_cap changed_cap monocular slam_mode
//   then   bad init_kf not_erase mp nmp kp_info ml nml kl_info cand n_cand
//          mp_bad mp_obs_off mp_obs_kf mp_obs_idx mp_nobs  ml_bad ml_obs_off ml_obs_kf ml_obs_idx ml_nobs
// The non-inertial lines function runs once through the host form and once through the batch form on device
// copies, into tables filled with -7 (outcome 121); OUT gets, per form, the blocks
//   ints n_visited stop n_kf_in_map err n_changed | outcome | n_mps | n_mls | n_redundant | changed_slot | changed_kind
// and last a block of statuses: the batch form without its scratch, with a scratch one byte short, with n_queries
// 65536, and plvi_keyframe_culling_scratch_bytes(2).
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

struct Out {
    int q[5];
    std::vector<unsigned char> outcome;
    std::vector<int> n_mps, n_mls, n_red, ch_slot, ch_kind;
    Out(int out_cap, int changed_cap)
        : outcome(out_cap, 121), n_mps(out_cap, -7), n_mls(out_cap, -7), n_red(out_cap, -7), ch_slot(changed_cap, -7),
          ch_kind(changed_cap, -7) {
        for (int i = 0; i < 5; ++i) q[i] = -7;
    }
    void write(FILE* f) const {
        put(f, q, sizeof q);
        put(f, outcome.data(), outcome.size());
        put(f, n_mps.data(), 4 * n_mps.size());
        put(f, n_mls.data(), 4 * n_mls.size());
        put(f, n_red.data(), 4 * n_red.size());
        put(f, ch_slot.data(), 4 * ch_slot.size());
        put(f, ch_kind.data(), 4 * ch_kind.size());
    }
};

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--sizes")) {
        printf("%d %d %d %d %d %zu %zu %zu %zu %zu\n", PLVI_CULL_MAX_CHANGED, PLVI_CULL_SPEC, PLVI_CULL_NEEDS_NORM,
               PLVI_CULL_DEFERRED, PLVI_CULL_ERR_QUERY, sizeof(plvi_cull_keyframes), sizeof(plvi_cull_features),
               sizeof(plvi_cull_params), sizeof(plvi_cull_queries), sizeof(plvi_cull_outputs));
        return 0;
    }
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    Bytes hdr, b[21];
    if (!take(in, hdr) || hdr.size() != 48) return 2;
    for (int i = 0; i < 21; ++i)
        if (!take(in, b[i])) return 2;
    fclose(in);
    const int* h = as<int>(hdr);
    const int K = h[0], kp_cap = h[1], kl_cap = h[2], stride = h[3], mp_n = h[4], ml_n = h[5], out_cap = h[8],
              changed_cap = h[9];
    const int q_slot = h[6], n_kf = h[7], zero = 0;
    plvi_cull_params par;
    par.redundant_th = 0.9f;
    par.monocular = h[10];
    par.inertial = 0;
    par.slam_mode = h[11];

    // ---- the host form
    plvi_cull_keyframes kf;
    memset(&kf, 0, sizeof kf);
    kf.kf_cap = K;
    kf.kp_cap = kp_cap;
    kf.kl_cap = kl_cap;
    kf.cand_stride = stride;
    kf.bad = as<uint8_t>(b[0]);
    kf.init_kf = as<uint8_t>(b[1]);
    kf.not_erase = as<uint8_t>(b[2]);
    kf.mp = as<int>(b[3]);
    kf.nmp = as<int>(b[4]);
    kf.kp_info = as<uint8_t>(b[5]);
    kf.ml = as<int>(b[6]);
    kf.nml = as<int>(b[7]);
    kf.kl_info = as<uint8_t>(b[8]);
    kf.cand = as<int>(b[9]);
    kf.n_cand = as<int>(b[10]);
    plvi_local_map_pool mp, ml;
    memset(&mp, 0, sizeof mp);
    memset(&ml, 0, sizeof ml);
    mp.n = mp_n;
    mp.bad = as<uint8_t>(b[11]);
    mp.obs_off = as<int>(b[12]);
    mp.obs_kf = as<int>(b[13]);
    plvi_cull_features fmp = {as<int>(b[14]), as<int>(b[15])};
    ml.n = ml_n;
    ml.bad = as<uint8_t>(b[16]);
    ml.obs_off = as<int>(b[17]);
    ml.obs_kf = as<int>(b[18]);
    plvi_cull_features fml = {as<int>(b[19]), as<int>(b[20])};
    plvi_cull_queries qs;
    memset(&qs, 0, sizeof qs);
    qs.q_slot = &q_slot;
    qs.abort_ba = &zero;
    qs.n_kf_in_map = &n_kf;
    qs.imu_init = &zero;
    qs.inertial_ba2 = &zero;

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    {
        Out o(out_cap, changed_cap);
        plvi_cull_outputs po = {out_cap, changed_cap, &o.q[0], &o.q[1], &o.q[2], &o.q[3], o.outcome.data(),
                                o.n_mps.data(), o.n_mls.data(), o.n_red.data(), &o.q[4], o.ch_slot.data(),
                                o.ch_kind.data()};
        const int rc = plvi_keyframe_culling(&kf, &mp, &fmp, &ml, &fml, &par, &qs, &po);
        if (rc != PLVI_OK && rc != PLVI_E_CAPACITY) return 4;
        o.write(out);
    }

    // ---- the batch form on device copies
    int st[4];
    {
        Dev d;
        plvi_cull_keyframes dk = kf;
        dk.bad = d.up<uint8_t>(b[0]);
        dk.init_kf = d.up<uint8_t>(b[1]);
        dk.not_erase = d.up<uint8_t>(b[2]);
        dk.mp = d.up<int>(b[3]);
        dk.nmp = d.up<int>(b[4]);
        dk.kp_info = d.up<uint8_t>(b[5]);
        dk.ml = d.up<int>(b[6]);
        dk.nml = d.up<int>(b[7]);
        dk.kl_info = d.up<uint8_t>(b[8]);
        dk.cand = d.up<int>(b[9]);
        dk.n_cand = d.up<int>(b[10]);
        plvi_local_map_pool dmp = mp, dml = ml;
        dmp.bad = d.up<uint8_t>(b[11]);
        dmp.obs_off = d.up<int>(b[12]);
        dmp.obs_kf = d.up<int>(b[13]);
        plvi_cull_features dfmp = {d.up<int>(b[14]), d.up<int>(b[15])};
        dml.bad = d.up<uint8_t>(b[16]);
        dml.obs_off = d.up<int>(b[17]);
        dml.obs_kf = d.up<int>(b[18]);
        plvi_cull_features dfml = {d.up<int>(b[19]), d.up<int>(b[20])};
        const int qhost[5] = {q_slot, 0, n_kf, 0, 0};
        const int* dq = d.up<int>(qhost, sizeof qhost);
        plvi_cull_queries dqs;
        memset(&dqs, 0, sizeof dqs);
        dqs.q_slot = dq;
        dqs.abort_ba = dq + 1;
        dqs.n_kf_in_map = dq + 2;
        dqs.imu_init = dq + 3;
        dqs.inertial_ba2 = dq + 4;
        Out o(out_cap, changed_cap);
        int* dper = d.up<int>(o.q, sizeof o.q);
        plvi_cull_outputs po = {out_cap, changed_cap, dper, dper + 1, dper + 2, dper + 3,
                                d.up<uint8_t>(o.outcome.data(), o.outcome.size()),
                                d.up<int>(o.n_mps.data(), 4 * o.n_mps.size()),
                                d.up<int>(o.n_mls.data(), 4 * o.n_mls.size()),
                                d.up<int>(o.n_red.data(), 4 * o.n_red.size()), dper + 4,
                                d.up<int>(o.ch_slot.data(), 4 * o.ch_slot.size()),
                                d.up<int>(o.ch_kind.data(), 4 * o.ch_kind.size())};
        const size_t sb = plvi_keyframe_culling_scratch_bytes(1);
        void* scratch = d.up<unsigned char>(NULL, sb);
        if (plvi_keyframe_culling_batch(1, &dk, &dmp, &dfmp, &dml, &dfml, &par, &dqs, &po, scratch, sb, NULL) != PLVI_OK)
            return 5;
        if (plvi_device_synchronize() != PLVI_OK) return 5;
        plvi_memcpy(o.q, dper, sizeof o.q, 2);
        plvi_memcpy(o.outcome.data(), po.outcome, o.outcome.size(), 2);
        plvi_memcpy(o.n_mps.data(), po.n_mps, 4 * o.n_mps.size(), 2);
        plvi_memcpy(o.n_mls.data(), po.n_mls, 4 * o.n_mls.size(), 2);
        plvi_memcpy(o.n_red.data(), po.n_redundant, 4 * o.n_red.size(), 2);
        plvi_memcpy(o.ch_slot.data(), po.changed_slot, 4 * o.ch_slot.size(), 2);
        plvi_memcpy(o.ch_kind.data(), po.changed_kind, 4 * o.ch_kind.size(), 2);
        o.write(out);
        st[0] = plvi_keyframe_culling_batch(1, &dk, &dmp, &dfmp, &dml, &dfml, &par, &dqs, &po, NULL, sb, NULL);
        st[1] = plvi_keyframe_culling_batch(1, &dk, &dmp, &dfmp, &dml, &dfml, &par, &dqs, &po, scratch, sb - 1, NULL);
        st[2] = plvi_keyframe_culling_batch(65536, &dk, &dmp, &dfmp, &dml, &dfml, &par, &dqs, &po, scratch, sb, NULL);
        st[3] = (int)plvi_keyframe_culling_scratch_bytes(2);
    }
    put(out, st, sizeof st);
    fclose(out);
    return 0;
}
