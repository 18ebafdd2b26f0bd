// triangulation_capi_check.cpp — a C++11 caller of the triangulation section
// of the C-ABI through include/plvi_frontend.h only, the way the
// INTEGRATION.md shims of LocalMapping::CreateNewMapPoints /
// CreateNewMapLines call it.  Usage: triangulation_capi_check <in.bin> <out.bin>
//
// in.bin (written by tests/test_triangulation_capi_native.py): int32 n1, n2,
// nnodes1, nnodes2, nl1, nl2; the plvi_triangulation_pair; then per keyframe
// keypoints, descriptors, node ids, offsets (nnodes + 1), the index list
// (off[nnodes] entries), has_point, uright; then the LBD rows of both
// keyframes and the two has_line masks.
// out.bin: int32 nmatches (or error), matches12 [n1]; int32 status of the
// line call, npairs, pairs [nl1][2]; double nn_mad, nn12_mad.
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

struct KeyFrameSide {
    std::vector<plvi_keypoint> kps;
    std::vector<uint8_t> desc, has_point;
    std::vector<int32_t> node, off, idx;
    std::vector<float> uright;
    void read(int n, int nnodes) {
        kps = take<plvi_keypoint>(n);
        desc = take<uint8_t>((size_t)n * 32);
        node = take<int32_t>(nnodes);
        off = take<int32_t>(nnodes + 1);
        idx = take<int32_t>(off[nnodes]);
        has_point = take<uint8_t>(n);
        uright = take<float>(n);
    }
};

struct DeviceMem {
    void* p;
    DeviceMem(const void* src, size_t bytes) : p(nullptr) {
        if (plvi_device_malloc(&p, bytes ? bytes : 1) != PLVI_OK) exit(4);
        if (src && bytes && plvi_memcpy(p, src, bytes, 1) != PLVI_OK) exit(4);
    }
    ~DeviceMem() { plvi_device_free(p); }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    if (!g_in) return 3;
    const std::vector<int32_t> hd = take<int32_t>(6);
    const int n1 = hd[0], n2 = hd[1], nn1 = hd[2], nn2 = hd[3], nl1 = hd[4], nl2 = hd[5];
    const std::vector<plvi_triangulation_pair> pair = take<plvi_triangulation_pair>(1);
    KeyFrameSide a, b;
    a.read(n1, nn1);
    b.read(n2, nn2);
    const std::vector<uint8_t> l1 = take<uint8_t>((size_t)nl1 * 32), l2 = take<uint8_t>((size_t)nl2 * 32);
    const std::vector<uint8_t> hl1 = take<uint8_t>(nl1), hl2 = take<uint8_t>(nl2);
    fclose(g_in);

    // ORBmatcher::SearchForTriangulation: vMatches12, then vMatchedPairs by compaction
    std::vector<int32_t> m12(n1 ? n1 : 1, -7);
    const int nmatches = plvi_search_for_triangulation(
        &pair[0], a.kps.data(), a.desc.data(), n1, a.node.data(), a.off.data(), nn1, a.idx.data(),
        a.has_point.data(), a.uright.data(), b.kps.data(), b.desc.data(), n2, b.node.data(), b.off.data(), nn2,
        b.idx.data(), b.has_point.data(), b.uright.data(), m12.data());

    // LineMatcher::SearchForTriangulation, one pair through the batched entry point
    const int32_t counts[3] = {nl1, nl2, -7};
    int lrc;
    std::vector<int32_t> lpairs((size_t)(nl1 ? nl1 : 1) * 2, -7);
    int32_t npairs = -7;
    double mad[2] = {-7.0, -7.0};
    {
        const int cap1 = nl1 ? nl1 : 1, cap2 = nl2 ? nl2 : 1;
        DeviceMem d1(l1.data(), (size_t)nl1 * 32), d2(l2.data(), (size_t)nl2 * 32), dh1(hl1.data(), nl1),
            dh2(hl2.data(), nl2), dcnt(counts, sizeof(counts)), dscr(nullptr, (size_t)16 * cap1),
            dout(nullptr, (size_t)8 * cap1), dmad(nullptr, 16);
        int32_t* cnt = static_cast<int32_t*>(dcnt.p);
        lrc = plvi_line_search_triangulation_batch(
            static_cast<const uint8_t*>(d1.p), cnt, cap1, static_cast<const uint8_t*>(d2.p), cnt + 1, cap2, 1,
            static_cast<const uint8_t*>(dh1.p), static_cast<const uint8_t*>(dh2.p), static_cast<int*>(dscr.p),
            static_cast<int*>(dout.p), cnt + 2, static_cast<double*>(dmad.p), nullptr);
        if (lrc == PLVI_OK) lrc = plvi_device_synchronize();
        if (lrc == PLVI_OK) lrc = plvi_memcpy(&npairs, cnt + 2, 4, 2);
        if (lrc == PLVI_OK && npairs > 0 && npairs <= nl1)
            lrc = plvi_memcpy(lpairs.data(), dout.p, (size_t)8 * npairs, 2);
        if (lrc == PLVI_OK) lrc = plvi_memcpy(mad, dmad.p, 16, 2);
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    const int32_t nm = nmatches, lr = lrc;
    fwrite(&nm, 4, 1, o);
    fwrite(m12.data(), 4, n1, o);
    fwrite(&lr, 4, 1, o);
    fwrite(&npairs, 4, 1, o);
    fwrite(lpairs.data(), 8, nl1, o);
    fwrite(mad, 8, 2, o);
    fclose(o);
    return 0;
}
