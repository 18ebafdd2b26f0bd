// gba_propagate_ref.cpp — a sequential host restatement of the second half of
// LoopClosing::RunGlobalBundleAdjustment[WithLines] (src/LoopClosing.cc:3727-3843 the spanning-tree walk,
// :3847-3884 the MapPoint loop, :3887-3930 the MapLine loop) in the reference's own shape: KeyFrame objects in one
// array at ascending addresses given by `order`, mspChildrens a std::set<KeyFrame*>, lpKFtoCheck a std::list, the
// stamps members of the objects; the feature loops over cv::Mat expressions, Rcw * X + tcw through cv_gemm_pose.
//
// Parity unpinned: what cv::gemm does inside.  cv_gemm_pose is gemm_pose of oracle/frustum_oracle.cpp: float
// products summed in row order, plain or contracted (PLVI_COMPAT_GEMM_FMA), then (float)(t0 * alpha + c * beta) in
// double.  Built on demand by tests/test_gba_propagate.py with -ffp-contract=off.
//
// Where the reference would not return (a cycle) or would dereference NULL (a feature without a reference
// keyframe) the restatement raises the bit the library raises: the queue is cut at kf_cap entries.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <list>
#include <set>
#include <vector>

#include "../../include/plvi_frontend.h"
#include "../../oracle/ref_fma.h"

namespace {

struct Mat31 {  // a 3x1 CV_32F cv::Mat
    float v[3];
};

struct Pose {  // the rowRange(0,3) of a 4x4 CV_32F pose: R row-major, then t
    float R[9], t[3];
    bool empty = true;
};

// R * P + t: MatExpr -> cv::gemm(R, P, 1, t, 1), the small-matrix path
Mat31 cv_gemm_pose(const Pose& T, const Mat31& P, bool fma_form) {
    Mat31 r;
    for (int i = 0; i < 3; i++) {
        const float* a = T.R + 3 * i;
        float s;
        if (fma_form) s = ref_fmaf(a[2], P.v[2], ref_fmaf(a[0], P.v[0], a[1] * P.v[1]));
        else s = a[0] * P.v[0] + a[1] * P.v[1] + a[2] * P.v[2];
        const double t0 = s;
        r.v[i] = (float)(t0 * 1.0 + (double)T.t[i] * 1.0);
    }
    return r;
}

struct KeyFrame {
    int slot = -1;
    bool mbBad = false;
    unsigned long mnBAGlobalForKF = 0;
    std::set<KeyFrame*> mspChildrens;
    Pose mTcwBefGBA, Twc;
    bool isBad() const { return mbBad; }
    std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
    Pose GetPoseInverse() const { return Twc; }
};

}  // namespace

extern "C" {

struct GbaWalkRefArgs {
    int kf_cap, n_order, n_origins, walk_cap;
    unsigned loop_kf;
    const uint8_t* bad;
    const int *order, *child_off, *child, *origins;
    unsigned* kf_ba_for;
    int *walk, *walk_parent;
    uint8_t* walk_new;
    int *n_walk, *n_new, *err;
    uint8_t* visited;
    double* seconds;
};

struct GbaCorrectRefArgs {
    int n, kf_cap, kind, fma_form, map;
    unsigned loop_kf;
    const uint8_t* bad;
    const int *map_id, *ref_kf;
    const unsigned *feat_ba_for, *kf_ba_for;
    const uint8_t* has_bef;
    const float *tcw_bef, *twc;
    const void* pos_gba;
    void* col;  // in place: pos [n][3] float or sep [n][6] double
    uint8_t* state;
    int *counts, *err;
    double* seconds;
};

void gba_walk_ref_run(const GbaWalkRefArgs* t) {
    const int K = t->kf_cap;
    // address order: the slots `order` names at their first position, then the others by slot
    std::vector<KeyFrame> kfs(K);
    std::vector<int> at(K, -1);
    int next = 0;
    for (int i = 0; i < t->n_order; ++i)
        if (t->order[i] >= 0 && t->order[i] < K && at[t->order[i]] < 0) at[t->order[i]] = next++;
    for (int s = 0; s < K; ++s)
        if (at[s] < 0) at[s] = next++;
    auto kf = [&](int s) { return s >= 0 && s < K ? &kfs[at[s]] : (KeyFrame*)nullptr; };
    for (int s = 0; s < K; ++s) {
        KeyFrame& k = *kf(s);
        k.slot = s;
        k.mbBad = t->bad[s] != 0;
        k.mnBAGlobalForKF = t->kf_ba_for[s];
        if (t->child_off)
            for (int e = t->child_off[s]; e < t->child_off[s + 1]; ++e) k.mspChildrens.insert(kf(t->child[e]));
    }
    const unsigned long nLoopKF = t->loop_kf;
    int err = 0, n_new = 0;
    std::vector<KeyFrame*> mvpKeyFrameOrigins;
    for (int i = 0; i < t->n_origins; ++i) {
        if (KeyFrame* o = kf(t->origins[i])) mvpKeyFrameOrigins.push_back(o);
        else err |= PLVI_GBA_ERR_ORIGIN;  // the vector holds keyframes only
    }

    const auto t0 = std::chrono::steady_clock::now();
    // what the caller's shim records per queue entry, in order
    struct Entry {
        KeyFrame *kf, *parent;
        bool is_new;
    };
    std::vector<Entry> out;
    std::list<Entry> lpKFtoCheck;
    for (KeyFrame* o : mvpKeyFrameOrigins) lpKFtoCheck.push_back({o, nullptr, false});
    size_t queued = lpKFtoCheck.size();
    bool cycle = queued > (size_t)K;
    while (!lpKFtoCheck.empty() && !cycle) {
        KeyFrame* pKF = lpKFtoCheck.front().kf;
        const std::set<KeyFrame*> sChilds = pKF->GetChilds();
        for (std::set<KeyFrame*>::const_iterator sit = sChilds.begin(); sit != sChilds.end(); sit++) {
            KeyFrame* pChild = *sit;
            if (!pChild || pChild->isBad()) continue;
            bool is_new = false;
            if (pChild->mnBAGlobalForKF != nLoopKF) {
                // mTcwGBA, mVwbGBA, mBiasGBA: the caller's
                pChild->mnBAGlobalForKF = nLoopKF;
                is_new = true;
                n_new++;
            }
            if (++queued > (size_t)K) {  // more entries than keyframes: the reference does not return
                cycle = true;
                break;
            }
            lpKFtoCheck.push_back({pChild, pKF, is_new});
        }
        // mTcwBefGBA = GetPose(); SetPose(mTcwGBA): the caller's, per entry of the list
        out.push_back(lpKFtoCheck.front());
        lpKFtoCheck.pop_front();
    }
    if (t->seconds) *t->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (cycle) {
        err |= PLVI_GBA_ERR_CYCLE;  // the lists are unspecified from here on
        *t->n_walk = *t->n_new = 0;
        *t->err = err;
        return;
    }
    for (size_t i = 0; i < out.size(); ++i) {
        if ((int)i < t->walk_cap) {
            t->walk[i] = out[i].kf->slot;
            t->walk_parent[i] = out[i].parent ? out[i].parent->slot : -1;
            t->walk_new[i] = out[i].is_new;
        }
        if (t->visited) t->visited[out[i].kf->slot] = 1;
    }
    if ((int)out.size() > t->walk_cap) err |= PLVI_GBA_ERR_WALK;
    for (int s = 0; s < K; ++s) t->kf_ba_for[s] = (unsigned)kf(s)->mnBAGlobalForKF;
    *t->n_walk = (int)out.size();
    *t->n_new = n_new;
    *t->err = err;
}

void gba_correct_ref_run(const GbaCorrectRefArgs* t) {
    const int K = t->kf_cap;
    const bool fma_form = t->fma_form != 0;
    std::vector<KeyFrame> kfs(K);
    for (int s = 0; s < K; ++s) {
        kfs[s].slot = s;
        kfs[s].mnBAGlobalForKF = t->kf_ba_for[s];
        kfs[s].mTcwBefGBA.empty = !t->has_bef[s];
        memcpy(kfs[s].mTcwBefGBA.R, t->tcw_bef + 12 * (size_t)s, 12 * sizeof(float));
        memcpy(kfs[s].Twc.R, t->twc + 12 * (size_t)s, 12 * sizeof(float));
    }
    const unsigned long nLoopKF = t->loop_kf;
    int counts[3] = {0, 0, 0}, err = 0;
    float* pos = static_cast<float*>(t->col);
    double* sep = static_cast<double*>(t->col);
    const float* pos_gba = static_cast<const float*>(t->pos_gba);
    const double* sep_gba = static_cast<const double*>(t->pos_gba);
    const bool lines = t->kind == PLVI_GBA_LINES;

    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < t->n; i++) {
        int st = 0;
        do {
            // GetAllMapPoints() / GetAllMapLines() of the active map
            if (t->map_id && t->map_id[i] != t->map) break;
            if (t->bad[i]) break;  // isBad()
            if (t->feat_ba_for[i] == nLoopKF) {
                // SetWorldPos(mPosGBA): a copy of the matrix data
                if (lines) memcpy(sep + 6 * (size_t)i, sep_gba + 6 * (size_t)i, 6 * sizeof(double));
                else memcpy(pos + 3 * (size_t)i, pos_gba + 3 * (size_t)i, 3 * sizeof(float));
                st = 1;
                break;
            }
            const int r = t->ref_kf[i];
            if (r < 0 || r >= K) {  // GetReferenceKeyFrame() == NULL
                err |= PLVI_GBA_ERR_REF;
                break;
            }
            KeyFrame* pRefKF = &kfs[r];
            if (pRefKF->mnBAGlobalForKF != nLoopKF) break;
            if (pRefKF->mTcwBefGBA.empty) break;
            const Pose Twc = pRefKF->GetPoseInverse();
            if (!lines) {
                Mat31 X;
                memcpy(X.v, pos + 3 * (size_t)i, sizeof X.v);
                const Mat31 Xc = cv_gemm_pose(pRefKF->mTcwBefGBA, X, fma_form);
                const Mat31 Xw = cv_gemm_pose(Twc, Xc, fma_form);
                memcpy(pos + 3 * (size_t)i, Xw.v, sizeof Xw.v);
            } else {
                for (int e = 0; e < 2; e++) {
                    double* p = sep + 6 * (size_t)i + 3 * e;
                    const Mat31 X = {{(float)p[0], (float)p[1], (float)p[2]}};  // Converter::toCvMat(Vector3d)
                    const Mat31 Xc = cv_gemm_pose(pRefKF->mTcwBefGBA, X, fma_form);
                    const Mat31 Xw = cv_gemm_pose(Twc, Xc, fma_form);
                    for (int c = 0; c < 3; c++) p[c] = Xw.v[c];  // Converter::toVector3d
                }
            }
            st = 2;
        } while (false);
        t->state[i] = (uint8_t)st;
        counts[st]++;
    }
    if (t->seconds) *t->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    memcpy(t->counts, counts, sizeof counts);
    *t->err = err;
}
}
