// kfdb_capi_check.cpp — a C++11 caller of the plvi_kfdb_* entry points through
// include/plvi_frontend.h only, the way the INTEGRATION.md shims of
// Tracking::Relocalization and LoopClosing::NewDetectCommonRegions call them.
// Usage: kfdb_capi_check <in.bin> <out.bin>
//
// in.bin (written by tests/test_kfdb_capi_native.py): int32 n_words, slot_cap, word_cap, n_kf, n_q, n_maps;
// per keyframe int32 slot, map, n, then n uint32 words and n doubles; per query int32 map, n, n_conn,
// then the words, the values and n_conn connected slots; the covisibility table [slot_cap][10];
// map_bad [n_maps] bytes.
// The first half of the keyframes goes through plvi_kfdb_add, the second through one
// plvi_kfdb_add_batch call from device tables.
// out.bin: per query the mode 0 count and candidates (int32 n, then n slots) from plvi_kfdb_query,
// then n_loop, the loop slots, n_merge, the merge slots from the mode 1 call; then the same for all
// queries from one plvi_kfdb_query_batch call per mode (device outputs, 3 candidates a row kept);
// then int32 statuses: add to an occupied slot, add to slot_cap, create with L2_NORM, create with
// word_cap above the limit, an empty query batch.
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

struct Dev {
    void* p;
    Dev(const void* src, size_t bytes) : p(nullptr) {
        if (plvi_device_malloc(&p, bytes ? bytes : 4)) exit(4);
        if (src && bytes && plvi_memcpy(p, src, bytes, 1)) exit(4);
    }
    ~Dev() { plvi_device_free(p); }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

void put(FILE* o, const int32_t* v, size_t n) { fwrite(v, 4, n, o); }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    if (!g_in) return 3;
    const std::vector<int32_t> hd = take<int32_t>(6);
    const int n_words = hd[0], slot_cap = hd[1], word_cap = hd[2], n_kf = hd[3], n_q = hd[4], n_maps = hd[5];
    plvi_kf_database* db = nullptr;
    if (plvi_kfdb_create(n_words, slot_cap, word_cap, 0, 0, &db) || !db) return 4;

    // keyframes: the second half is packed into [row][word_cap] tables for the batched add
    const int first_batch = n_kf / 2, n_rows = n_kf - first_batch;
    std::vector<uint32_t> tw((size_t)(n_rows ? n_rows : 1) * word_cap, 0);
    std::vector<double> tv((size_t)(n_rows ? n_rows : 1) * word_cap, 0);
    std::vector<int32_t> tn(n_rows ? n_rows : 1, 0), entries;
    for (int k = 0; k < n_kf; ++k) {
        const std::vector<int32_t> h3 = take<int32_t>(3);
        const std::vector<uint32_t> w = take<uint32_t>(h3[2]);
        const std::vector<double> v = take<double>(h3[2]);
        if (k < first_batch) {
            if (plvi_kfdb_add(db, h3[0], h3[1], w.data(), v.data(), h3[2])) return 5;
        } else {
            const int r = k - first_batch;
            for (int i = 0; i < h3[2]; ++i) {
                tw[(size_t)r * word_cap + i] = w[i];
                tv[(size_t)r * word_cap + i] = v[i];
            }
            tn[r] = h3[2];
            entries.push_back(r);
            entries.push_back(h3[0]);
            entries.push_back(h3[1]);
        }
    }
    {
        const Dev dw(tw.data(), 4 * tw.size()), dv(tv.data(), 8 * tv.size()), dn(tn.data(), 4 * tn.size());
        if (plvi_kfdb_add_batch(db, n_rows, entries.data(), dw.as<unsigned>(), dv.as<double>(), dn.as<int>(), word_cap,
                                nullptr))
            return 5;
        if (plvi_kfdb_errors(db, nullptr, nullptr)) return 5;
    }

    std::vector<std::vector<uint32_t> > qw(n_q);
    std::vector<std::vector<double> > qv(n_q);
    std::vector<std::vector<int32_t> > qc(n_q);
    std::vector<int32_t> qmap(n_q ? n_q : 1), qn(n_q ? n_q : 1), conn_off(1, 0), conn_all;
    for (int q = 0; q < n_q; ++q) {
        const std::vector<int32_t> h3 = take<int32_t>(3);
        qmap[q] = h3[0];
        qn[q] = h3[1];
        qw[q] = take<uint32_t>(h3[1]);
        qv[q] = take<double>(h3[1]);
        qc[q] = take<int32_t>(h3[2]);
        qc[q].resize(h3[2]);
        conn_all.insert(conn_all.end(), qc[q].begin(), qc[q].end());
        conn_off.push_back((int32_t)conn_all.size());
    }
    const std::vector<int32_t> covis = take<int32_t>((size_t)slot_cap * PLVI_KFDB_NEIGHBOURS);
    const std::vector<uint8_t> bad = take<uint8_t>(n_maps);
    fclose(g_in);

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 6;
    const int n_best = 3;
    // one query at a time from host memory: each keyframe's members carry over to the next call
    for (int q = 0; q < n_q; ++q) {
        std::vector<int32_t> cand(slot_cap, -7), loop(n_best, -7), merge(n_best, -7);
        const int32_t n = plvi_kfdb_query(db, qw[q].data(), qv[q].data(), qn[q], qmap[q], 0, 0, nullptr, 0, covis.data(),
                                          nullptr, 0, cand.data(), slot_cap, nullptr, nullptr, nullptr, nullptr);
        put(o, &n, 1);
        if (n > 0) put(o, cand.data(), n);
        int32_t nl = -7, nm = -7;
        if (plvi_kfdb_query(db, qw[q].data(), qv[q].data(), qn[q], qmap[q], 1, n_best, qc[q].data(), (int)qc[q].size(),
                            covis.data(), bad.data(), n_maps, nullptr, 0, loop.data(), &nl, merge.data(), &nm) < 0)
            return 7;
        put(o, &nl, 1);
        put(o, loop.data(), nl);
        put(o, &nm, 1);
        put(o, merge.data(), nm);
    }
    // all queries in one call per mode, device tables in and out
    {
        std::vector<uint32_t> w((size_t)(n_q ? n_q : 1) * word_cap, 0);
        std::vector<double> v((size_t)(n_q ? n_q : 1) * word_cap, 0);
        for (int q = 0; q < n_q; ++q)
            for (int i = 0; i < qn[q]; ++i) {
                w[(size_t)q * word_cap + i] = qw[q][i];
                v[(size_t)q * word_cap + i] = qv[q][i];
            }
        conn_all.push_back(0);
        const Dev dw(w.data(), 4 * w.size()), dv(v.data(), 8 * v.size()), dn(qn.data(), 4 * qn.size()),
            dm(qmap.data(), 4 * qmap.size()), dco(conn_off.data(), 4 * conn_off.size()),
            dcs(conn_all.data(), 4 * conn_all.size()), dcv(covis.data(), 4 * covis.size()), db_(bad.data(), bad.size());
        const size_t rows = n_q ? n_q : 1;
        std::vector<int32_t> fill(rows * 3, -7);
        const Dev oc(fill.data(), 12 * rows), onc(fill.data(), 4 * rows), ol(fill.data(), 12 * rows),
            onl(fill.data(), 4 * rows), om(fill.data(), 12 * rows), onm(fill.data(), 4 * rows);
        if (plvi_kfdb_query_batch(db, n_q, dw.as<unsigned>(), dv.as<double>(), dn.as<int>(), word_cap, dm.as<int>(), 0, 0,
                                  nullptr, nullptr, dcv.as<int>(), nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                  oc.as<int>(), 3, onc.as<int>(), nullptr, nullptr, nullptr, nullptr, nullptr))
            return 8;
        if (plvi_kfdb_query_batch(db, n_q, dw.as<unsigned>(), dv.as<double>(), dn.as<int>(), word_cap, dm.as<int>(), 1,
                                  n_best, dco.as<int>(), dcs.as<int>(), dcv.as<int>(), db_.as<uint8_t>(), n_maps, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, 0, nullptr, ol.as<int>(), onl.as<int>(),
                                  om.as<int>(), onm.as<int>(), nullptr))
            return 8;
        if (plvi_device_synchronize()) return 8;
        const Dev* outs[6] = {&onc, &oc, &onl, &ol, &onm, &om};
        for (int k = 0; k < 6; ++k) {
            std::vector<int32_t> h(rows * (k % 2 ? 3 : 1));
            if (plvi_memcpy(h.data(), outs[k]->p, 4 * h.size(), 2)) return 8;
            put(o, h.data(), (size_t)n_q * (k % 2 ? 3 : 1));
        }
    }
    // refusals
    const uint32_t one_word[1] = {0};
    const double one_value[1] = {1.0};
    int32_t rc[5];
    rc[0] = n_kf ? plvi_kfdb_add(db, entries.empty() ? 0 : entries[1], 0, one_word, one_value, 1) : PLVI_E_BADARG;
    rc[1] = plvi_kfdb_add(db, slot_cap, 0, one_word, one_value, 1);
    plvi_kf_database* other = nullptr;
    rc[2] = plvi_kfdb_create(n_words, slot_cap, word_cap, 1, 0, &other);
    rc[3] = plvi_kfdb_create(n_words, slot_cap, PLVI_KFDB_MAX_WORDS + 1, 0, 0, &other);
    rc[4] = plvi_kfdb_query_batch(db, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr,
                                  0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr);
    put(o, rc, 5);
    fclose(o);
    return plvi_kfdb_destroy(db);
}
