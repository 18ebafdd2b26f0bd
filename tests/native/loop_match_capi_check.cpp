// loop_match_capi_check.cpp — a C++11 caller of the loop-closing matchers of
// the C-ABI through include/plvi_frontend.h only, the way the INTEGRATION.md
// shims of LoopClosing::DetectCommonRegionsFromBoW / FindMatchesByProjection
// call them.  Usage: loop_match_capi_check <in.bin> <out.bin>
//
// in.bin (written by tests/test_loop_match_capi_native.py): int32 n1, n2,
// nnodes1, nnodes2, check_orientation, n_kp, n_pt, has_matched; float
// nnratio; per keyframe of the BoW pair descriptors, angles, live bytes, node
// ids, offsets (nnodes + 1), the index list (off[nnodes] entries); the
// plvi_sim3_proj_params; keypoints, descriptors, matched bytes; per point
// flags, x3dc, dist, dot, level, descriptors.
// out.bin: int32 nmatches (or error) of SearchByBoW, matches12 [n1]; int32
// nmatches (or error) of SearchByProjection, match [n_kp]; int32 status of
// the two empty batch calls.
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
    std::vector<uint8_t> desc, live;
    std::vector<float> angle;
    std::vector<int32_t> node, off, idx;
    void read(int n, int nnodes) {
        desc = take<uint8_t>((size_t)n * 32);
        angle = take<float>(n);
        live = take<uint8_t>(n);
        node = take<int32_t>(nnodes);
        off = take<int32_t>(nnodes + 1);
        idx = take<int32_t>(off[nnodes]);
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    g_in = fopen(argv[1], "rb");
    if (!g_in) return 3;
    const std::vector<int32_t> hd = take<int32_t>(8);
    const int n1 = hd[0], n2 = hd[1], nn1 = hd[2], nn2 = hd[3], ori = hd[4], n_kp = hd[5], n_pt = hd[6];
    const bool has_matched = hd[7] != 0;
    const float nnratio = take<float>(1)[0];
    KeyFrameSide a, b;
    a.read(n1, nn1);
    b.read(n2, nn2);
    const std::vector<plvi_sim3_proj_params> prm = take<plvi_sim3_proj_params>(1);
    const std::vector<plvi_keypoint> kps = take<plvi_keypoint>(n_kp);
    const std::vector<uint8_t> desc = take<uint8_t>((size_t)n_kp * 32), matched = take<uint8_t>(n_kp);
    const std::vector<uint8_t> flags = take<uint8_t>(n_pt);
    const std::vector<float> x3dc = take<float>((size_t)n_pt * 3), dist = take<float>((size_t)n_pt * 3);
    const std::vector<double> dot = take<double>(n_pt);
    const std::vector<int32_t> level = take<int32_t>(n_pt);
    const std::vector<uint8_t> mp_desc = take<uint8_t>((size_t)n_pt * 32);
    fclose(g_in);

    // ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12): vpMatches12[i] = vpMapPoints2[m12[i]]
    std::vector<int32_t> m12(n1 ? n1 : 1, -7);
    const int nbow = plvi_search_by_bow_kf(nnratio, ori, a.desc.data(), a.angle.data(), a.live.data(), n1,
                                           a.node.data(), a.off.data(), nn1, a.idx.data(), b.desc.data(),
                                           b.angle.data(), b.live.data(), n2, b.node.data(), b.off.data(), nn2,
                                           b.idx.data(), m12.data());

    // ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, [vpPointsKFs,] vpMatched, [vpMatchedKF,] th, ratio)
    std::vector<int32_t> match(n_kp ? n_kp : 1, -7);
    const int nproj = plvi_search_sim3_projection(&prm[0], kps.data(), desc.data(), n_kp,
                                                  has_matched ? matched.data() : nullptr, flags.data(), x3dc.data(),
                                                  dist.data(), dot.data(), level.data(), mp_desc.data(), n_pt,
                                                  match.data());

    // the batched entry points: an empty batch is valid and launches nothing
    const int32_t rc_bow = plvi_search_by_bow_kf_batch(0, nnratio, ori, 1, 1, 1, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr);
    const int32_t rc_proj = plvi_search_sim3_projection_batch(0, &prm[0], nullptr, nullptr, nullptr, 1, nullptr,
                                                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                              nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr);

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 5;
    const int32_t nb = nbow, np = nproj;
    fwrite(&nb, 4, 1, o);
    fwrite(m12.data(), 4, n1, o);
    fwrite(&np, 4, 1, o);
    fwrite(match.data(), 4, n_kp, o);
    fwrite(&rc_bow, 4, 1, o);
    fwrite(&rc_proj, 4, 1, o);
    fclose(o);
    return 0;
}
