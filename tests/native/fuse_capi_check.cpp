// fuse_capi_check.cpp — a C++11 caller of the Fuse searches of the C-ABI
// through include/plvi_frontend.h only, the way the INTEGRATION.md shims of
// LocalMapping::SearchInNeighbors / LoopClosing::SearchAndFuse call them.
// Usage: fuse_capi_check <in.bin> <out.bin>
//
// in.bin (written by tests/test_fuse_capi_native.py): int32 n_kp, n_pt,
// has_uright, n_kl, n_ml; the plvi_fuse_params; keypoints, descriptors,
// mvuRight; per point flags, x3dc, dist, dot, level, descriptors; the
// plvi_fuse_line_params; keylines, descriptors; per MapLine flags, spc, epc,
// dist, dot, level, descriptors.
// out.bin: per mode 0 / 1 int32 nfused (or error), fuse_idx [n_pt], fuse_dist
// [n_pt]; for the lines int32 nfused, fuse_idx [n_ml], fuse_dist [n_ml];
// int32 status of the two empty batch calls.
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

void put(FILE* o, int32_t n, const std::vector<int32_t>& idx, const std::vector<int32_t>& dist, int rows) {
    fwrite(&n, 4, 1, o);
    fwrite(idx.data(), 4, rows, o);
    fwrite(dist.data(), 4, rows, o);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    if (!g_in) return 3;
    const std::vector<int32_t> hd = take<int32_t>(5);
    const int n_kp = hd[0], n_pt = hd[1], n_kl = hd[3], n_ml = hd[4];
    const bool has_uright = hd[2] != 0;
    std::vector<plvi_fuse_params> prm = take<plvi_fuse_params>(1);
    const std::vector<plvi_keypoint> kps = take<plvi_keypoint>(n_kp);
    const std::vector<uint8_t> desc = take<uint8_t>((size_t)n_kp * 32);
    const std::vector<float> uright = take<float>(n_kp);
    const std::vector<uint8_t> flags = take<uint8_t>(n_pt);
    const std::vector<float> x3dc = take<float>((size_t)n_pt * 3), dist = take<float>((size_t)n_pt * 3);
    const std::vector<double> dot = take<double>(n_pt);
    const std::vector<int32_t> level = take<int32_t>(n_pt);
    const std::vector<uint8_t> mp_desc = take<uint8_t>((size_t)n_pt * 32);
    const std::vector<plvi_fuse_line_params> lprm = take<plvi_fuse_line_params>(1);
    const std::vector<plvi_keyline> kl = take<plvi_keyline>(n_kl);
    const std::vector<uint8_t> kl_desc = take<uint8_t>((size_t)n_kl * 32);
    const std::vector<uint8_t> lflags = take<uint8_t>(n_ml);
    const std::vector<float> spc = take<float>((size_t)n_ml * 3), epc = take<float>((size_t)n_ml * 3);
    const std::vector<float> ldist = take<float>((size_t)n_ml * 3);
    const std::vector<double> ldot = take<double>(n_ml);
    const std::vector<int32_t> llevel = take<int32_t>(n_ml);
    const std::vector<uint8_t> ml_desc = take<uint8_t>((size_t)n_ml * 32);
    fclose(g_in);

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    // ORBmatcher::Fuse(pKF, vpMapPoints, th) and Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): the search;
    // the caller then walks fuse_idx in list order (GetMapPoint(bestIdx), Replace / AddObservation)
    for (int mode = 0; mode < 2; ++mode) {
        prm[0].mode = mode;
        std::vector<int32_t> fuse_idx(n_pt ? n_pt : 1, -7), fuse_dist(n_pt ? n_pt : 1, -7);
        const int n = plvi_fuse_points(&prm[0], kps.data(), desc.data(), n_kp,
                                       mode == 0 && has_uright ? uright.data() : nullptr, flags.data(), x3dc.data(),
                                       dist.data(), dot.data(), level.data(), mp_desc.data(), n_pt, fuse_idx.data(),
                                       fuse_dist.data());
        put(o, n, fuse_idx, fuse_dist, n_pt);
    }
    // LineMatcher::Fuse(pKF, vpMapLines, th)
    std::vector<int32_t> line_idx(n_ml ? n_ml : 1, -7), line_dist(n_ml ? n_ml : 1, -7);
    const int nl = plvi_fuse_lines(&lprm[0], kl.data(), kl_desc.data(), n_kl, lflags.data(), spc.data(), epc.data(),
                                   ldist.data(), ldot.data(), llevel.data(), ml_desc.data(), n_ml, line_idx.data(),
                                   line_dist.data());
    put(o, nl, line_idx, line_dist, n_ml);

    // the batched entry points: an empty batch is valid and launches nothing
    const int32_t rc_pts = plvi_fuse_points_batch(0, &prm[0], nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1,
                                                  nullptr, nullptr, nullptr, nullptr);
    const int32_t rc_lines = plvi_fuse_lines_batch(0, &lprm[0], nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr,
                                                   nullptr, nullptr);
    fwrite(&rc_pts, 4, 1, o);
    fwrite(&rc_lines, 4, 1, o);
    fclose(o);
    return 0;
}
