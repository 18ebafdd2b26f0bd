// essential_graph_capi_check.cpp — a C++11 caller of plvi_loop_correct[_device] and plvi_essential_graph[_device]
// that includes only include/plvi_frontend.h, the way a CorrectLoop shim does.
//   essential_graph_capi_check --sizes          prints the header's constants and struct sizes
//   essential_graph_capi_check in.bin out.bin   runs both forms of both calls on the tables of in.bin (blocks of
//                                               [int bytes][bytes], see tests/test_essential_graph_capi_native.py)
//                                               and writes every output, then the status of a few refused calls.
#include <cstdio>
#include <cstring>
#include <string>
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
void put(FILE* f, const std::vector<int>& v) { put(f, v.data(), 4 * v.size()); }

template <class T>
const T* ptr(const Bytes& b) { return reinterpret_cast<const T*>(b.data()); }

// a device copy of a block (a block of no bytes is one zero byte: a present, empty table)
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
    void down(void* dst, const void* d, size_t bytes) {
        if (bytes && plvi_memcpy(dst, d, bytes, 2) != 0) ok = false;
    }
    ~Dev() {
        for (size_t i = 0; i < all.size(); ++i)
            if (all[i]) plvi_device_free(all[i]);
    }
};

const int FILL = -7;

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "--sizes") {
        printf("%d %d %d %d %d %d %d %d %zu %zu %zu %zu\n", PLVI_EG_MAX_WIN, PLVI_EG_MIN_FEAT, PLVI_EG_4DOF,
               PLVI_EG_EDGE_INERTIAL, PLVI_EG_ERR_QUERY, PLVI_EG_ERR_NO_VERTEX, PLVI_EG_ERR_LC, PLVI_COVIS_MAX_CONN,
               sizeof(plvi_eg_keyframes), sizeof(plvi_eg_features), sizeof(plvi_loop_correct_outputs),
               sizeof(plvi_eg_outputs));
        return 0;
    }
    if (argc != 3) return 2;
    const std::vector<Bytes> b = read_blocks(argv[1]);
    if (b.size() != 37) return 3;
    const int* h = ptr<int>(b[0]);
    const int K = h[0], kp_cap = h[1], kl_cap = h[2], C = h[3], n_order = h[4], mp_n = h[5], ml_n = h[6], cur = h[7],
              loop = h[8], mode = h[9], n_win = h[10], lc_cap = h[11], win_cap = h[12], pt_cap = h[13], ln_cap = h[14],
              vert_cap = h[15], edge_cap = h[16];
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    int rc_all = 0;
    for (int form = 0; form < 2; ++form) {  // 0 host, 1 device
        Dev d;
        // the tables: host pointers, or device copies of the same blocks
        std::vector<const void*> t(37);
        for (int i = 1; i < 37; ++i) t[i] = form ? d.up(b[i]) : (const void*)b[i].data();
        // stamps are in/out: the host form works on copies
        Bytes by_p = b[26], ref_p = b[27], by_l = b[31], ref_l = b[32];
        if (!form) t[26] = by_p.data(), t[27] = ref_p.data(), t[31] = by_l.data(), t[32] = ref_l.data();
        plvi_cull_keyframes kf;
        memset(&kf, 0, sizeof kf);
        kf.kf_cap = K, kf.kp_cap = kp_cap, kf.kl_cap = kl_cap, kf.cand_stride = C;
        kf.bad = (const uint8_t*)t[1], kf.init_kf = (const uint8_t*)t[2], kf.mp = (const int*)t[3];
        kf.nmp = (const int*)t[4], kf.ml = (const int*)t[5], kf.nml = (const int*)t[6], kf.cand = (const int*)t[7];
        kf.n_cand = (const int*)t[8], kf.kf_id = (const unsigned*)t[9], kf.prev_kf = (const int*)t[10];
        kf.next_kf = (const int*)t[11];
        plvi_eg_keyframes eg;
        memset(&eg, 0, sizeof eg);
        eg.n_order = n_order, eg.map_stride = C, eg.order = (const int*)t[12], eg.map_id = (const int*)t[13];
        eg.parent = (const int*)t[14], eg.child_off = (const int*)t[15], eg.child = (const int*)t[16];
        eg.loop_off = (const int*)t[17], eg.loop = (const int*)t[18], eg.imu = (const uint8_t*)t[19];
        eg.cand_w = (const int*)t[20], eg.map_kf = (const int*)t[21], eg.map_w = (const int*)t[22];
        eg.map_n = (const int*)t[23];
        plvi_local_map_pool mp, ml;
        memset(&mp, 0, sizeof mp);
        memset(&ml, 0, sizeof ml);
        mp.n = mp_n, mp.bad = (const uint8_t*)t[24], ml.n = ml_n, ml.bad = (const uint8_t*)t[29];
        plvi_eg_features fmp, fml;
        fmp.ref_kf = (const int*)t[25], fmp.corr_by = (unsigned*)t[26], fmp.corr_ref = (int*)t[27];
        fmp.map_id = (const int*)t[28];
        fml.ref_kf = (const int*)t[30], fml.corr_by = (unsigned*)t[31], fml.corr_ref = (int*)t[32];
        fml.map_id = (const int*)t[33];

        // ---- A
        std::vector<int> counts(5, FILL), win(win_cap + 1, FILL), sorted(win_cap + 1, FILL), pts(pt_cap + 1, FILL),
            pts_kf(pt_cap + 1, FILL), lns(ln_cap + 1, FILL), lns_kf(ln_cap + 1, FILL);
        std::vector<std::vector<int>*> lists;
        lists.push_back(&counts), lists.push_back(&win), lists.push_back(&sorted), lists.push_back(&pts);
        lists.push_back(&pts_kf), lists.push_back(&lns), lists.push_back(&lns_kf);
        std::vector<int*> at(lists.size());
        for (size_t i = 0; i < lists.size(); ++i)
            at[i] = form ? (int*)d.up(lists[i]->data(), 4 * lists[i]->size()) : lists[i]->data();
        plvi_loop_correct_outputs oa;
        oa.win_cap = win_cap, oa.pt_cap = pt_cap, oa.ln_cap = ln_cap;
        oa.n_win = at[0], oa.n_sorted = at[0] + 1, oa.n_pts = at[0] + 2, oa.n_lns = at[0] + 3, oa.err = at[0] + 4;
        oa.win = at[1], oa.win_sorted = at[2], oa.pts = at[3], oa.pts_kf = at[4], oa.lns = at[5], oa.lns_kf = at[6];
        int rc;
        if (form) {
            const size_t sb = plvi_loop_correct_scratch_bytes(K, mp_n, ml_n);
            rc = plvi_loop_correct_device(cur, &kf, &eg, &mp, &ml, &fmp, &fml, &oa, d.up(nullptr, sb), sb, nullptr);
            if (plvi_device_synchronize() != 0) rc = -100;
            for (size_t i = 0; i < lists.size(); ++i) d.down(lists[i]->data(), at[i], 4 * lists[i]->size());
            d.down(by_p.data(), t[26], by_p.size()), d.down(ref_p.data(), t[27], ref_p.size());
            d.down(by_l.data(), t[31], by_l.size()), d.down(ref_l.data(), t[32], ref_l.size());
        } else {
            rc = plvi_loop_correct(cur, &kf, &eg, &mp, &ml, &fmp, &fml, &oa);
        }
        put(out, &rc, 4);
        for (size_t i = 0; i < lists.size(); ++i) put(out, *lists[i]);
        put(out, by_p.data(), by_p.size()), put(out, ref_p.data(), ref_p.size());
        put(out, by_l.data(), by_l.size()), put(out, ref_l.data(), ref_l.size());

        // ---- C, on the stamps A left
        std::vector<int> nv(2, FILL), ne(5, FILL), vert(vert_cap + 1, FILL), flags(vert_cap + 1, FILL),
            ea(edge_cap + 1, FILL), eb(edge_cap + 1, FILL), ek(edge_cap + 1, FILL), pref(mp_n + 1, FILL),
            lref(ml_n + 1, FILL);
        lists.clear();
        lists.push_back(&nv), lists.push_back(&ne), lists.push_back(&vert), lists.push_back(&flags);
        lists.push_back(&ea), lists.push_back(&eb), lists.push_back(&ek), lists.push_back(&pref), lists.push_back(&lref);
        at.assign(lists.size(), nullptr);
        for (size_t i = 0; i < lists.size(); ++i)
            at[i] = form ? (int*)d.up(lists[i]->data(), 4 * lists[i]->size()) : lists[i]->data();
        plvi_eg_outputs oc;
        oc.vert_cap = vert_cap, oc.edge_cap = edge_cap;
        oc.n_vert = at[0], oc.err = at[0] + 1, oc.n_edges = at[1], oc.vert = at[2], oc.vert_flags = at[3];
        oc.edge_a = at[4], oc.edge_b = at[5], oc.edge_kind = at[6], oc.pt_ref = at[7], oc.ln_ref = at[8];
        const int nw[1] = {n_win};
        if (form) {
            const size_t sb = plvi_essential_graph_scratch_bytes(K, n_order, n_win, lc_cap);
            rc = plvi_essential_graph_device(cur, loop, mode, (const int*)t[34], (const int*)d.up(nw, 4), n_win,
                                             (const int*)t[35], (const int*)t[36], lc_cap, &kf, &eg, &mp, &ml, &fmp, &fml,
                                             &oc, d.up(nullptr, sb), sb, nullptr);
            if (plvi_device_synchronize() != 0) rc = -100;
            for (size_t i = 0; i < lists.size(); ++i) d.down(lists[i]->data(), at[i], 4 * lists[i]->size());
        } else {
            rc = plvi_essential_graph(cur, loop, mode, (const int*)t[34], nw, n_win, (const int*)t[35],
                                      (const int*)t[36], lc_cap, &kf, &eg, &mp, &ml, &fmp, &fml, &oc);
        }
        put(out, &rc, 4);
        for (size_t i = 0; i < lists.size(); ++i) put(out, *lists[i]);

        if (form) {  // refusals: nothing is launched
            std::vector<int> bad;
            const size_t sb = plvi_essential_graph_scratch_bytes(K, n_order, n_win, lc_cap);
            void* scr = d.up(nullptr, sb);
            bad.push_back(plvi_essential_graph_device(cur, loop, 2, (const int*)t[34], at[0], n_win, (const int*)t[35],
                                                      (const int*)t[36], lc_cap, &kf, &eg, &mp, &ml, &fmp, &fml, &oc, scr,
                                                      sb, nullptr));  // unknown mode
            bad.push_back(plvi_essential_graph_device(cur, loop, mode, (const int*)t[34], at[0], n_win, (const int*)t[35],
                                                      (const int*)t[36], lc_cap, &kf, &eg, &mp, &ml, &fmp, &fml, &oc, scr,
                                                      sb - 1, nullptr));  // scratch too small
            plvi_eg_keyframes part = eg;
            part.loop = nullptr;
            bad.push_back(plvi_essential_graph_device(cur, loop, mode, (const int*)t[34], at[0], n_win, (const int*)t[35],
                                                      (const int*)t[36], lc_cap, &kf, &part, &mp, &ml, &fmp, &fml, &oc,
                                                      scr, sb, nullptr));  // a CSR given in part
            bad.push_back(plvi_essential_graph_device(cur, loop, mode, (const int*)t[34], at[0], PLVI_EG_MAX_WIN + 1,
                                                      (const int*)t[35], (const int*)t[36], lc_cap, &kf, &eg, &mp, &ml,
                                                      &fmp, &fml, &oc, scr, sb, nullptr));  // above the window bound
            plvi_eg_features half = fmp;
            half.corr_ref = nullptr;
            const size_t sa = plvi_loop_correct_scratch_bytes(K, mp_n, ml_n);
            bad.push_back(plvi_loop_correct_device(cur, &kf, &eg, &mp, &ml, &half, &fml, &oa, scr, sa, nullptr));
            plvi_cull_keyframes wide = kf;
            wide.cand_stride = PLVI_EG_MAX_WIN;
            bad.push_back(plvi_loop_correct_device(cur, &wide, &eg, &mp, &ml, &fmp, &fml, &oa, scr, sa, nullptr));
            bad.push_back(plvi_loop_connections_device(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                                       nullptr, nullptr, nullptr, 0, nullptr));
            bad.push_back((int)sa);
            put(out, bad);
        }
        if (!d.ok) rc_all = 5;
    }
    fclose(out);
    return rc_all;
}
