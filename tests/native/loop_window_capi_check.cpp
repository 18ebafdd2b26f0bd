// loop_window_capi_check.cpp — a C++11 caller of plvi_loop_window[_batch] and plvi_loop_bow_merge[_batch] that
// includes only include/plvi_frontend.h, the way the INTEGRATION.md shim of LoopClosing::NewDetectCommonRegions does.
//
// --sizes prints the header's constants and struct sizes (no device needed): PLVI_LOOP_COVISIBLES,
// PLVI_LOOP_BOW_WIN, PLVI_LOOP_WIN_MAX, PLVI_LOOP_WIN_LAST, PLVI_LOOP_ERR_QUERY, sizeof of the two structs.
//
// IN OUT: IN is a sequence of blocks, each an int32 byte count and the bytes --
//   ints   kf_cap kp_cap cand_stride mp_n | kind kf_slot pt_cap | bow_slot cur_slot n1 cap1
//   then   bad mp nmp cand n_cand  mp_bad mp_pos  conn  matches12
// Query A (kind, kf_slot) runs with a pos gather, query B (PLVI_LOOP_WIN_BOW, bow_slot, conn) runs and is merged
// with matches12 [6][cap1]; each once through the host forms and once through the batch forms on device copies,
// into tables filled with -7.  OUT gets, per form, the blocks
//   ints n_win abort_at n_pts err | win | pts | pts_kf | pos      (A)
//   ints n_win abort_at n_pts err num | win | matched_mp | matched_kf      (B)
// and last a block of statuses: the batch form without its scratch, with a scratch one byte short, with n_queries
// 65536, with a gather whose pool row is missing, the merge with a negative cap1, and
// plvi_loop_window_scratch_bytes(2, mp_n).
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
    template <class T>
    T* up(std::vector<T>& v) { return up<T>(v.data(), sizeof(T) * v.size()); }
    template <class T>
    void down(std::vector<T>& v, const T* d) {
        if (plvi_memcpy(v.data(), d, sizeof(T) * v.size(), 2) != PLVI_OK) exit(3);
    }
    ~Dev() {
        for (size_t i = 0; i < all.size(); ++i) plvi_device_free(all[i]);
    }
};

struct Out {  // one query's outputs on the host, pre-filled
    std::vector<int> scal, win, pts, pts_kf, mmp, mkf;
    std::vector<float> pos;
    Out(int pt_cap, int cap1)
        : scal(5, -7), win(PLVI_LOOP_WIN_MAX, -7), pts(pt_cap ? pt_cap : 1, -7), pts_kf(pts), mmp(cap1 ? cap1 : 1, -7),
          mkf(mmp), pos(3 * pts.size(), -7.f) {}
    void point(plvi_loop_outputs& o, int pt_cap, bool gather) {
        memset(&o, 0, sizeof o);
        o.pt_cap = pt_cap;
        o.win = win.data();
        o.n_win = &scal[0];
        o.abort_at = &scal[1];
        o.n_pts = &scal[2];
        o.err = &scal[3];
        o.pts = pts.data();
        o.pts_kf = pts_kf.data();
        o.pos = gather ? pos.data() : NULL;
    }
    void write_a(FILE* f) const {
        put(f, scal.data(), 16);
        put(f, win.data(), 4 * win.size());
        put(f, pts.data(), 4 * pts.size());
        put(f, pts_kf.data(), 4 * pts_kf.size());
        put(f, pos.data(), 4 * pos.size());
    }
    void write_b(FILE* f) const {
        put(f, scal.data(), 20);
        put(f, win.data(), 4 * win.size());
        put(f, mmp.data(), 4 * mmp.size());
        put(f, mkf.data(), 4 * mkf.size());
    }
};

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--sizes")) {
        printf("%d %d %d %d %d %zu %zu\n", PLVI_LOOP_COVISIBLES, PLVI_LOOP_BOW_WIN, PLVI_LOOP_WIN_MAX,
               (int)PLVI_LOOP_WIN_LAST, (int)PLVI_LOOP_ERR_QUERY, sizeof(plvi_loop_queries), sizeof(plvi_loop_outputs));
        return 0;
    }
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    Bytes ints, bad, mp, nmp, cand, n_cand, mp_bad, mp_pos, conn, m12;
    Bytes* blocks[] = {&ints, &bad, &mp, &nmp, &cand, &n_cand, &mp_bad, &mp_pos, &conn, &m12};
    for (size_t i = 0; i < sizeof blocks / sizeof *blocks; ++i)
        if (!take(in, *blocks[i])) return 2;
    fclose(in);
    if (ints.size() != 11 * 4) return 2;
    const int* I = as<int>(ints);
    const int kf_cap = I[0], kp_cap = I[1], cand_stride = I[2], mp_n = I[3], kind = I[4], kf_slot = I[5], pt_cap = I[6],
              bow_slot = I[7], cur_slot = I[8], n1 = I[9], cap1 = I[10];
    const int conn_off[2] = {0, (int)(conn.size() / 4)};
    const int bow_kind = PLVI_LOOP_WIN_BOW;

    plvi_cull_keyframes kf;
    memset(&kf, 0, sizeof kf);
    kf.kf_cap = kf_cap;
    kf.kp_cap = kp_cap;
    kf.cand_stride = cand_stride;
    kf.bad = as<uint8_t>(bad);
    kf.mp = as<int>(mp);
    kf.nmp = as<int>(nmp);
    kf.cand = as<int>(cand);
    kf.n_cand = as<int>(n_cand);
    plvi_local_map_pool pool;
    memset(&pool, 0, sizeof pool);
    pool.n = mp_n;
    pool.bad = as<uint8_t>(mp_bad);
    pool.pos = as<float>(mp_pos);
    plvi_loop_queries qa, qb;
    memset(&qa, 0, sizeof qa);
    qa.kind = &kind;
    qa.kf_slot = &kf_slot;
    memset(&qb, 0, sizeof qb);
    qb.kind = &bow_kind;
    qb.kf_slot = &bow_slot;
    qb.cur_slot = &cur_slot;
    if (!conn.empty()) {  // both or neither
        qb.conn_off = conn_off;
        qb.conn_slot = as<int>(conn);
    }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;

    {  // the host forms
        Out a(pt_cap, cap1), b(pt_cap, cap1);
        plvi_loop_outputs o;
        a.point(o, pt_cap, true);
        int rc = plvi_loop_window(&kf, &pool, &qa, &o);
        if (rc != PLVI_OK && rc != PLVI_E_CAPACITY) return 4;
        a.write_a(out);
        b.point(o, pt_cap, false);
        if (plvi_loop_window(&kf, &pool, &qb, &o) != PLVI_OK) return 4;
        if (plvi_loop_bow_merge(&kf, &pool, b.win.data(), &b.scal[0], &b.scal[1], as<int>(m12), &n1, cap1, b.mmp.data(),
                                b.mkf.data(), &b.scal[4]) != PLVI_OK)
            return 4;
        b.write_b(out);
    }
    int status[6];
    {  // the batch forms on device copies
        Dev d;
        plvi_cull_keyframes dk = kf;
        dk.bad = d.up<uint8_t>(bad);
        dk.mp = d.up<int>(mp);
        dk.nmp = d.up<int>(nmp);
        dk.cand = d.up<int>(cand);
        dk.n_cand = d.up<int>(n_cand);
        plvi_local_map_pool dp = pool;
        dp.bad = d.up<uint8_t>(mp_bad);
        dp.pos = d.up<float>(mp_pos);
        const size_t sb = plvi_loop_window_scratch_bytes(1, mp_n);
        void* scratch = d.up<unsigned char>(NULL, sb);
        Out a(pt_cap, cap1), b(pt_cap, cap1);
        for (int pass = 0; pass < 2; ++pass) {
            Out& h = pass ? b : a;
            plvi_loop_queries dq;
            memset(&dq, 0, sizeof dq);
            dq.kind = d.up<int>(pass ? &bow_kind : &kind, 4);
            dq.kf_slot = d.up<int>(pass ? &bow_slot : &kf_slot, 4);
            if (pass) {
                dq.cur_slot = d.up<int>(&cur_slot, 4);
                if (!conn.empty()) {
                    dq.conn_off = d.up<int>(conn_off, 8);
                    dq.conn_slot = d.up<int>(conn.data(), conn.size());
                }
            }
            plvi_loop_outputs o;
            memset(&o, 0, sizeof o);
            o.pt_cap = pt_cap;
            int* scal = d.up(h.scal);
            o.win = d.up(h.win);
            o.n_win = scal;
            o.abort_at = scal + 1;
            o.n_pts = scal + 2;
            o.err = scal + 3;
            o.pts = d.up(h.pts);
            o.pts_kf = d.up(h.pts_kf);
            o.pos = pass ? NULL : d.up(h.pos);
            if (plvi_loop_window_batch(1, &dk, &dp, &dq, &o, scratch, sb, NULL) != PLVI_OK) return 5;
            int *mmp = NULL, *mkf = NULL;
            if (pass) {
                mmp = d.up(h.mmp);
                mkf = d.up(h.mkf);
                if (plvi_loop_bow_merge_batch(1, &dk, &dp, o.win, o.n_win, o.abort_at, d.up<int>(m12), d.up<int>(&n1, 4),
                                              cap1, mmp, mkf, scal + 4, scratch, sb, NULL) != PLVI_OK)
                    return 5;
            }
            if (plvi_device_synchronize() != PLVI_OK) return 5;
            d.down(h.scal, scal);
            d.down(h.win, o.win);
            d.down(h.pts, o.pts);
            d.down(h.pts_kf, o.pts_kf);
            if (!pass) d.down(h.pos, o.pos);
            if (pass) {
                d.down(h.mmp, mmp);
                d.down(h.mkf, mkf);
                h.write_b(out);
            } else {
                h.write_a(out);
                // the refusals, on the arguments of a call that has just run
                status[0] = plvi_loop_window_batch(1, &dk, &dp, &dq, &o, NULL, sb, NULL);
                status[1] = plvi_loop_window_batch(1, &dk, &dp, &dq, &o, scratch, sb - 1, NULL);
                status[2] = plvi_loop_window_batch(65536, &dk, &dp, &dq, &o, scratch, sb, NULL);
                plvi_local_map_pool np = dp;
                np.pos = NULL;
                status[3] = plvi_loop_window_batch(1, &dk, &np, &dq, &o, scratch, sb, NULL);
                status[4] = plvi_loop_bow_merge_batch(1, &dk, &dp, o.win, o.n_win, o.abort_at, NULL, o.n_pts, -1, NULL,
                                                      NULL, o.err, scratch, sb, NULL);
            }
        }
    }
    status[5] = (int)plvi_loop_window_scratch_bytes(2, mp_n);
    put(out, status, sizeof status);
    fclose(out);
    return 0;
}
