// local_map_capi_check.cpp — a C++11 caller of the plvi_local_map_* entry points through
// include/plvi_frontend.h only, the way the INTEGRATION.md shim of Tracking::UpdateLocalMap calls
// them.  Usage: local_map_capi_check <in.bin> <out.bin>
//
// Both files are sequences of blocks: int32 byte count, then the bytes.
// in.bin (written by tests/test_local_map_capi_native.py): a header of int32 kf_cap, n_order,
// kp_cap, kl_cap, n_mp, n_ml, n_frames, vote_cap, vote_lcap, seen_cap; then kf_bad, order, covis, child_off,
// child, parent, prev_kf, kf_mp, nmp, kf_ml, nml; mp_bad, mp_obs_off, mp_obs_kf, mp_pos, mp_desc;
// ml_bad, ml_obs_off, ml_obs_kf, ml_sep; vote_mp [n_frames][vote_cap], n_vote_mp, vote_ml
// [n_frames][vote_lcap], n_vote_ml, last_kf, seen_mp [n_frames][seen_cap] (the current frame's own table, apart
// from the voting one), n_seen_mp.
// out.bin: per frame the host form (plvi_local_map) -- a block of int32 status, n_local_kf, ref_kf,
// n_local_mp, n_local_ml, err, then local_kf, local_mp, mp_in_flags, mp_pos, mp_desc, local_ml,
// ml_sep and the vote tables as written back; then the same blocks per frame from ONE
// plvi_local_map_batch call over all frames (device tables, capacities = the pool sizes); then a
// block of statuses: a negative n_frames, a negative capacity, a scratch block one byte short,
// n_frames above the limit, an empty batch.
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

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!g_in || !g_out) return 3;
    const std::vector<char> hd = take();
    const int32_t* h = as<int32_t>(hd);
    const int K = h[0], n_order = h[1], kp_cap = h[2], kl_cap = h[3], n_mp = h[4], n_ml = h[5], B = h[6], vcap = h[7],
              vlcap = h[8], scap = h[9];
    const std::vector<char> kf_bad = take(), order = take(), covis = take(), child_off = take(), child = take(),
                            parent = take(), prev_kf = take(), kf_mp = take(), nmp = take(), kf_ml = take(),
                            nml = take(), mp_bad = take(), mp_off = take(), mp_obs = take(), mp_pos = take(),
                            mp_desc = take(), ml_bad = take(), ml_off = take(), ml_obs = take(), ml_sep = take();
    std::vector<char> vote_mp = take();
    const std::vector<char> n_vote_mp = take();
    std::vector<char> vote_ml = take();
    const std::vector<char> n_vote_ml = take(), last_kf = take(), seen_mp = take(), n_seen_mp = take();

    // ---- the host form, one frame at a time
    plvi_local_map_keyframes kf;
    memset(&kf, 0, sizeof kf);
    kf.kf_cap = K;
    kf.n_order = n_order;
    kf.kp_cap = kp_cap;
    kf.kl_cap = kl_cap;
    kf.bad = as<uint8_t>(kf_bad);
    kf.order = as<int>(order);
    kf.covis = as<int>(covis);
    kf.child_off = as<int>(child_off);
    kf.child = as<int>(child);
    kf.parent = as<int>(parent);
    kf.prev_kf = as<int>(prev_kf);
    kf.mp = as<int>(kf_mp);
    kf.nmp = as<int>(nmp);
    kf.ml = as<int>(kf_ml);
    kf.nml = as<int>(nml);
    plvi_local_map_pool mp, ml;
    memset(&mp, 0, sizeof mp);
    memset(&ml, 0, sizeof ml);
    mp.n = n_mp;
    mp.bad = as<uint8_t>(mp_bad);
    mp.obs_off = as<int>(mp_off);
    mp.obs_kf = as<int>(mp_obs);
    mp.pos = as<float>(mp_pos);
    mp.desc = as<uint8_t>(mp_desc);
    ml.n = n_ml;
    ml.bad = as<uint8_t>(ml_bad);
    ml.obs_off = as<int>(ml_off);
    ml.obs_kf = as<int>(ml_obs);
    ml.sep = as<double>(ml_sep);
    std::vector<int> vm0(as<int>(vote_mp), as<int>(vote_mp) + (size_t)B * vcap),
        vl0(as<int>(vote_ml), as<int>(vote_ml) + (size_t)B * vlcap);
    for (int f = 0; f < B; ++f) {
        std::vector<int> vm(vm0.begin() + (size_t)f * vcap, vm0.begin() + (size_t)(f + 1) * vcap),
            vl(vl0.begin() + (size_t)f * vlcap, vl0.begin() + (size_t)(f + 1) * vlcap);
        vm.push_back(0);
        vl.push_back(0);
        plvi_local_map_frames fr;
        memset(&fr, 0, sizeof fr);
        fr.vote_mp = vm.data();
        fr.n_vote_mp = as<int>(n_vote_mp) + f;
        fr.vote_mp_cap = vcap;
        fr.vote_ml = vl.data();
        fr.n_vote_ml = as<int>(n_vote_ml) + f;
        fr.vote_ml_cap = vlcap;
        fr.last_kf = as<int>(last_kf) + f;
        fr.seen_mp = as<int>(seen_mp) + (size_t)f * scap;
        fr.n_seen_mp = as<int>(n_seen_mp) + f;
        fr.seen_mp_cap = scap;
        std::vector<int> lkf(K + 1, -7), lmp(n_mp + 1, -7), lml(n_ml + 1, -7);
        std::vector<uint8_t> fl(n_mp + 1, 0x55), de((size_t)32 * n_mp + 32, 0x55);
        std::vector<float> pos((size_t)3 * n_mp + 3, -7.f);
        std::vector<double> sep((size_t)6 * n_ml + 6, -7.);
        int n[5] = {-7, -7, -7, -7, -7};  // n_local_kf, ref_kf, n_local_mp, n_local_ml, err
        plvi_local_map_outputs out;
        memset(&out, 0, sizeof out);
        out.lkf_cap = K;
        out.lmp_cap = n_mp;
        out.lml_cap = n_ml;
        out.local_kf = lkf.data();
        out.n_local_kf = &n[0];
        out.ref_kf = &n[1];
        out.local_mp = lmp.data();
        out.n_local_mp = &n[2];
        out.local_ml = lml.data();
        out.n_local_ml = &n[3];
        out.mp_pos = pos.data();
        out.mp_in_flags = fl.data();
        out.mp_desc = de.data();
        out.ml_sep = sep.data();
        out.err = &n[4];
        const int32_t head[6] = {plvi_local_map(&kf, &mp, &ml, &fr, &out), n[0], n[1], n[2], n[3], n[4]};
        if (head[0] < 0) return 5;
        put(head, sizeof head);
        put(lkf.data(), 4 * (size_t)n[0]);
        put(lmp.data(), 4 * (size_t)n[2]);
        put(fl.data(), (size_t)n[2]);
        put(pos.data(), 12 * (size_t)n[2]);
        put(de.data(), 32 * (size_t)n[2]);
        put(lml.data(), 4 * (size_t)n[3]);
        put(sep.data(), 48 * (size_t)n[3]);
        put(vm.data(), 4 * (size_t)vcap);
        put(vl.data(), 4 * (size_t)vlcap);
    }

    // ---- the batch form: everything resident, one call
    const size_t nchild = (size_t)(as<int>(child_off)[K]), nobs_mp = (size_t)(as<int>(mp_off)[n_mp]),
                 nobs_ml = (size_t)(as<int>(ml_off)[n_ml]);
    Dev d_bad(kf.bad, K), d_order(kf.order, 4 * (size_t)n_order), d_covis(kf.covis, 40 * (size_t)K),
        d_coff(kf.child_off, 4 * (size_t)(K + 1)), d_child(kf.child, 4 * nchild), d_parent(kf.parent, 4 * (size_t)K),
        d_prev(kf.prev_kf, 4 * (size_t)K), d_kmp(kf.mp, 4 * (size_t)K * kp_cap), d_nmp(kf.nmp, 4 * (size_t)K),
        d_kml(kf.ml, 4 * (size_t)K * kl_cap), d_nml(kf.nml, 4 * (size_t)K);
    Dev d_pbad(mp.bad, n_mp), d_poff(mp.obs_off, 4 * (size_t)(n_mp + 1)), d_pobs(mp.obs_kf, 4 * nobs_mp),
        d_ppos(mp.pos, 12 * (size_t)n_mp), d_pdesc(mp.desc, 32 * (size_t)n_mp);
    Dev d_lbad(ml.bad, n_ml), d_loff(ml.obs_off, 4 * (size_t)(n_ml + 1)), d_lobs(ml.obs_kf, 4 * nobs_ml),
        d_lsep(ml.sep, 48 * (size_t)n_ml);
    Dev d_vm(vm0.data(), 4 * (size_t)B * vcap), d_nvm(as<int>(n_vote_mp), 4 * (size_t)B),
        d_vl(vl0.data(), 4 * (size_t)B * vlcap), d_nvl(as<int>(n_vote_ml), 4 * (size_t)B),
        d_last(as<int>(last_kf), 4 * (size_t)B), d_sm(as<int>(seen_mp), 4 * (size_t)B * scap),
        d_nsm(as<int>(n_seen_mp), 4 * (size_t)B);
    plvi_local_map_keyframes dk = kf;
    dk.bad = d_bad.as<uint8_t>();
    dk.order = d_order.as<int>();
    dk.covis = d_covis.as<int>();
    dk.child_off = d_coff.as<int>();
    dk.child = d_child.as<int>();
    dk.parent = d_parent.as<int>();
    dk.prev_kf = d_prev.as<int>();
    dk.mp = d_kmp.as<int>();
    dk.nmp = d_nmp.as<int>();
    dk.ml = d_kml.as<int>();
    dk.nml = d_nml.as<int>();
    plvi_local_map_pool dp = mp, dl = ml;
    dp.bad = d_pbad.as<uint8_t>();
    dp.obs_off = d_poff.as<int>();
    dp.obs_kf = d_pobs.as<int>();
    dp.pos = d_ppos.as<float>();
    dp.desc = d_pdesc.as<uint8_t>();
    dl.bad = d_lbad.as<uint8_t>();
    dl.obs_off = d_loff.as<int>();
    dl.obs_kf = d_lobs.as<int>();
    dl.sep = d_lsep.as<double>();
    plvi_local_map_frames dfr;
    memset(&dfr, 0, sizeof dfr);
    dfr.vote_mp = d_vm.as<int>();
    dfr.n_vote_mp = d_nvm.as<int>();
    dfr.vote_mp_cap = vcap;
    dfr.vote_ml = d_vl.as<int>();
    dfr.n_vote_ml = d_nvl.as<int>();
    dfr.vote_ml_cap = vlcap;
    dfr.last_kf = d_last.as<int>();
    dfr.seen_mp = d_sm.as<int>();
    dfr.n_seen_mp = d_nsm.as<int>();
    dfr.seen_mp_cap = scap;
    const size_t b = (size_t)B;
    Dev o_lkf(nullptr, 4 * b * K), o_nkf(nullptr, 4 * b), o_ref(nullptr, 4 * b), o_lmp(nullptr, 4 * b * n_mp),
        o_nmp(nullptr, 4 * b), o_lml(nullptr, 4 * b * n_ml), o_nml(nullptr, 4 * b), o_pos(nullptr, 12 * b * n_mp),
        o_fl(nullptr, b * n_mp), o_de(nullptr, 32 * b * n_mp), o_sep(nullptr, 48 * b * n_ml), o_err(nullptr, 4 * b);
    plvi_local_map_outputs dout;
    memset(&dout, 0, sizeof dout);
    dout.lkf_cap = K;
    dout.lmp_cap = n_mp;
    dout.lml_cap = n_ml;
    dout.local_kf = o_lkf.as<int>();
    dout.n_local_kf = o_nkf.as<int>();
    dout.ref_kf = o_ref.as<int>();
    dout.local_mp = o_lmp.as<int>();
    dout.n_local_mp = o_nmp.as<int>();
    dout.local_ml = o_lml.as<int>();
    dout.n_local_ml = o_nml.as<int>();
    dout.mp_pos = o_pos.as<float>();
    dout.mp_in_flags = o_fl.as<uint8_t>();
    dout.mp_desc = o_de.as<uint8_t>();
    dout.ml_sep = o_sep.as<double>();
    dout.err = o_err.as<int>();
    const size_t sb = plvi_local_map_scratch_bytes(B, K, n_mp, n_ml);
    Dev scratch(nullptr, sb);
    const int rc = plvi_local_map_batch(B, &dk, &dp, &dl, &dfr, &dout, scratch.p, sb, nullptr);
    if (rc || plvi_device_synchronize()) return 6;
    const std::vector<int> nkf = o_nkf.down<int>(b), ref = o_ref.down<int>(b), np = o_nmp.down<int>(b),
                           nl = o_nml.down<int>(b), err = o_err.down<int>(b), lkf = o_lkf.down<int>(b * K),
                           lmp = o_lmp.down<int>(b * n_mp), lml = o_lml.down<int>(b * n_ml),
                           vm = d_vm.down<int>(b * vcap), vl = d_vl.down<int>(b * vlcap);
    const std::vector<uint8_t> fl = o_fl.down<uint8_t>(b * n_mp), de = o_de.down<uint8_t>(32 * b * n_mp);
    const std::vector<float> pos = o_pos.down<float>(3 * b * n_mp);
    const std::vector<double> sep = o_sep.down<double>(6 * b * n_ml);
    for (size_t f = 0; f < b; ++f) {
        const int32_t head[6] = {rc, nkf[f], ref[f], np[f], nl[f], err[f]};
        put(head, sizeof head);
        put(lkf.data() + f * K, 4 * (size_t)nkf[f]);
        put(lmp.data() + f * n_mp, 4 * (size_t)np[f]);
        put(fl.data() + f * n_mp, (size_t)np[f]);
        put(pos.data() + 3 * f * n_mp, 12 * (size_t)np[f]);
        put(de.data() + 32 * f * n_mp, 32 * (size_t)np[f]);
        put(lml.data() + f * n_ml, 4 * (size_t)nl[f]);
        put(sep.data() + 6 * f * n_ml, 48 * (size_t)nl[f]);
        put(vm.data() + f * vcap, 4 * (size_t)vcap);
        put(vl.data() + f * vlcap, 4 * (size_t)vlcap);
    }

    // ---- refusals
    plvi_local_map_outputs neg = dout;
    neg.lmp_cap = -1;
    const int32_t st[5] = {plvi_local_map_batch(-1, &dk, &dp, &dl, &dfr, &dout, scratch.p, sb, nullptr),
                           plvi_local_map_batch(B, &dk, &dp, &dl, &dfr, &neg, scratch.p, sb, nullptr),
                           plvi_local_map_batch(B, &dk, &dp, &dl, &dfr, &dout, scratch.p, sb - 1, nullptr),
                           plvi_local_map_batch(65536, &dk, &dp, &dl, &dfr, &dout, scratch.p, sb, nullptr),
                           plvi_local_map_batch(0, &dk, &dp, &dl, &dfr, &dout, nullptr, 0, nullptr)};
    put(st, sizeof st);
    fclose(g_out);
    return 0;
}
