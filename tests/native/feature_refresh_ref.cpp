// feature_refresh_ref.cpp — a sequential host restatement of MapPoint::UpdateNormalAndDepth
// (src/MapPoint.cc:427-494, NLeft == -1) and MapLine::UpdateNormalAndDepth (src/MapLine.cc:339-382) in the
// reference's own shape -- KeyFrame objects in one array, std::map<KeyFrame*, tuple<int,int>> /
// std::map<KeyFrame*, size_t> observations iterated in address order, observations[pRefKF] indexed as the
// reference indexes it -- followed by ComputeDistinctiveDescriptors through distinctive_ref.cpp, for a list of
// pool ids over the tables of plvi_feature_refresh[_batch].
//
// The OpenCV calls are the helpers cv_sub, cv_norm, cv_scale_add and cv_div_scalar.  Parity unpinned: what
// they do inside.  cv_norm and cv_sub as oracle/frustum_oracle.cpp takes them; normal + normali / s as
// scaleAdd(normali, (float)(1 / s), normal) with the scalar tail either plain or contracted
// (PLVI_COMPAT_SCALEADD_FMA); normal / n as a multiply by (float)(1.0 / (double)n).
// Built on demand by tests/test_feature_refresh.py with -ffp-contract=off.
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "../../include/plvi_frontend.h"
#include "../../oracle/ref_fma.h"
#include "distinctive_ref.cpp"

namespace {

struct Mat3 {  // a 3x1 CV_32F cv::Mat
    float v[3];
};

Mat3 cv_sub(const Mat3& a, const Mat3& b) { return {{a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]}}; }

double cv_norm(const Mat3& m) {  // normL2Sqr<float, double> + std::sqrt
    double s = 0;
    for (int i = 0; i < 3; i++) {
        double t = m.v[i];
        s += t * t;
    }
    return std::sqrt(s);
}

// acc + src / s: MatOp_AddEx -> scaleAdd(src, 1 / s, acc)
Mat3 cv_scale_add(const Mat3& acc, const Mat3& src, double s, bool fma_form) {
    const float alpha = (float)(1.0 / s);
    Mat3 r;
    for (int i = 0; i < 3; i++) r.v[i] = fma_form ? ref_fmaf(src.v[i], alpha, acc.v[i]) : src.v[i] * alpha + acc.v[i];
    return r;
}

// m / d: convertTo(CV_32F, 1 / d, 0)
Mat3 cv_div_scalar(const Mat3& m, double d) {
    const float a = (float)(1.0 / d);
    return {{m.v[0] * a, m.v[1] * a, m.v[2] * a}};
}

struct KeyPoint {
    int octave;
};

struct KeyFrame {
    Mat3 Ow;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvScaleFactors;
    int mnScaleLevels;
    bool mbBad;
    Mat3 GetCameraCenter() const { return Ow; }
    bool isBad() const { return mbBad; }
};

struct Result {
    bool written = false;
    int err = 0;
    Mat3 mNormalVector = {{0.f, 0.f, 0.f}};
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
};

// The part both functions share once Pos and `level` are settled differently.
template <class Observations, class LevelOf>
Result update_normal_and_depth(bool mbBad, const Observations& mObservations, KeyFrame* mpRefKF, const Mat3& mWorldPos,
                               bool ref_in_table, bool fma_form, LevelOf level_of) {
    Result res;
    Observations observations;
    KeyFrame* pRefKF;
    Mat3 Pos;
    {
        if (mbBad) return res;
        observations = mObservations;
        pRefKF = mpRefKF;
        Pos = mWorldPos;
    }
    if (observations.empty()) return res;

    Mat3 normal = {{0.f, 0.f, 0.f}};
    int n = 0;
    for (typename Observations::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;
        Mat3 Owi = pKF->GetCameraCenter();
        Mat3 normali = cv_sub(mWorldPos, Owi);
        normal = cv_scale_add(normal, normali, cv_norm(normali), fma_form);
        n++;
    }
    if (!ref_in_table) {  // precondition: pRefKF is a keyframe of the table
        res.err = PLVI_REFRESH_ERR_REF;
        return res;
    }
    Mat3 PC = cv_sub(Pos, pRefKF->GetCameraCenter());
    const float dist = cv_norm(PC);

    int level;
    if (int e = level_of(observations, pRefKF, &level)) {
        res.err = e;
        return res;
    }
    const int nLevels = pRefKF->mnScaleLevels;
    if (level >= nLevels) {  // precondition: mvScaleFactors[level] exists
        res.err = PLVI_REFRESH_ERR_LEVEL;
        return res;
    }
    const float levelScaleFactor = pRefKF->mvScaleFactors[level];
    {
        res.mfMaxDistance = dist * levelScaleFactor;
        res.mfMinDistance = res.mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
        res.mNormalVector = cv_div_scalar(normal, n);
    }
    res.written = true;
    return res;
}

}  // namespace

struct feature_refresh_ref_args {
    int kind, what, fma_form, n_levels, max_obs, row_cap;
    const float* scale;
    int kf_cap, cap;
    const uint8_t* kf_bad;
    const float* ow;
    const int* cnt;
    const uint8_t* info;
    const uint8_t* kf_desc;
    int n;
    const uint8_t* bad;
    const int* obs_off;
    const int* obs_kf;
    const int* obs_idx;
    const float* pos;
    const double* sep;
    const int* ref_kf;
    const int* ids;
    int n_ids;
    float* normal;
    float* dist;
    uint8_t* desc;
    uint8_t* state;
    int* best_pos;
    int* best_median;
    int* n_rows;
    int* err;
    double* seconds;
};

extern "C" void feature_refresh_ref_run(const feature_refresh_ref_args* a) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool lines = a->kind == PLVI_REFRESH_LINES;
    const bool fma_form = a->fma_form != 0;
    std::vector<KeyFrame> kfs(a->kf_cap);
    for (int k = 0; k < a->kf_cap; ++k) {
        KeyFrame& K = kfs[k];
        if (a->ow) K.Ow = {{a->ow[3 * k], a->ow[3 * k + 1], a->ow[3 * k + 2]}};
        const int N = a->cnt ? std::max(0, std::min(a->cnt[k], a->cap)) : 0;
        K.mvKeysUn.resize(N);
        for (int i = 0; i < N && a->info; ++i) K.mvKeysUn[i].octave = a->info[(size_t)k * a->cap + i] & 63;
        K.mvScaleFactors.assign(a->scale, a->scale + a->n_levels);
        K.mnScaleLevels = a->n_levels;
        K.mbBad = a->kf_bad && a->kf_bad[k];
    }
    auto in_table = [&](int k) { return k >= 0 && k < a->kf_cap; };
    auto list_len = [&](int id) {
        if (id < 0 || id >= a->n || a->bad[id]) return 0;
        return std::max(0, std::min(a->obs_off[id + 1] - a->obs_off[id], a->max_obs));
    };
    *a->err = 0;
    *a->n_rows = 0;

    for (int i = 0; i < a->n_ids; ++i) {
        const int id = a->ids[i];
        a->state[i] = 0;
        if (!(a->what & PLVI_REFRESH_NORMAL) || id < 0 || id >= a->n) continue;
        const int len = list_len(id), o0 = a->obs_off[id];
        const int ref = a->ref_kf[id];
        KeyFrame* mpRefKF = in_table(ref) ? &kfs[ref] : nullptr;
        Result r;
        if (!lines) {
            std::map<KeyFrame*, std::tuple<int, int>> mObservations;
            for (int t = 0; t < len; ++t)
                if (in_table(a->obs_kf[o0 + t]))
                    mObservations.insert({&kfs[a->obs_kf[o0 + t]], std::make_tuple(a->obs_idx[o0 + t], -1)});
            const Mat3 mWorldPos = {{a->pos[3 * id], a->pos[3 * id + 1], a->pos[3 * id + 2]}};
            r = update_normal_and_depth(
                a->bad[id] != 0, mObservations, mpRefKF, mWorldPos, mpRefKF != nullptr, fma_form,
                [](std::map<KeyFrame*, std::tuple<int, int>>& observations, KeyFrame* pRefKF, int* level) {
                    std::tuple<int, int> indexes = observations[pRefKF];
                    int leftIndex = std::get<0>(indexes);
                    // precondition: mvKeysUn[leftIndex] exists
                    if (leftIndex < 0 || leftIndex >= (int)pRefKF->mvKeysUn.size()) return (int)PLVI_REFRESH_ERR_KEYPOINT;
                    *level = pRefKF->mvKeysUn[leftIndex].octave;
                    return 0;
                });
        } else {
            std::map<KeyFrame*, size_t> mObservations;
            for (int t = 0; t < len; ++t)
                if (in_table(a->obs_kf[o0 + t]))
                    mObservations.insert({&kfs[a->obs_kf[o0 + t]], (size_t)(a->obs_idx ? a->obs_idx[o0 + t] : 0)});
            // Eigen::Vector3d MidPoint = (mWorldPos_sP + mWorldPos_eP) / 2; Pos = Converter::toCvMat(MidPoint)
            Mat3 Pos;
            for (int c = 0; c < 3; ++c) {
                const double MidPoint = (a->sep[6 * id + c] + a->sep[6 * id + 3 + c]) * 0.5;
                Pos.v[c] = (float)MidPoint;
            }
            r = update_normal_and_depth(a->bad[id] != 0, mObservations, mpRefKF, Pos, mpRefKF != nullptr, fma_form,
                                        [](std::map<KeyFrame*, size_t>&, KeyFrame*, int* level) {
                                            *level = 0;
                                            return 0;
                                        });
        }
        *a->err |= r.err;
        if (!r.written) continue;
        for (int c = 0; c < 3; ++c) a->normal[3 * id + c] = r.mNormalVector.v[c];
        a->dist[2 * id] = r.mfMinDistance;
        a->dist[2 * id + 1] = r.mfMaxDistance;
        a->state[i] |= PLVI_REFRESH_NORMAL;
    }

    if (a->what & PLVI_REFRESH_DESC) {
        // the CSR plvi_distinctive_descriptors_batch takes: a bad keyframe is skipped (MapPoint.cc:349)
        std::vector<int> off(a->n_ids + 1, 0), row;
        for (int i = 0; i < a->n_ids; ++i) {
            const int id = a->ids[i], len = list_len(id);
            for (int t = 0; t < len; ++t) {
                const int k = a->obs_kf[a->obs_off[id] + t], idx = a->obs_idx[a->obs_off[id] + t];
                const bool ok = in_table(k) && !kfs[k].isBad() && idx >= 0 && idx < (int)kfs[k].mvKeysUn.size();
                row.push_back(ok ? k * a->cap + idx : -1);
            }
            off[i + 1] = (int)row.size();
        }
        *a->n_rows = (int)row.size();
        if (*a->n_rows > a->row_cap) {
            *a->err |= PLVI_REFRESH_ERR_ROWS;
            for (int i = 0; i < a->n_ids; ++i) {
                if (a->best_pos) a->best_pos[i] = -1;
                if (a->best_median) a->best_median[i] = -1;
            }
        } else if (a->n_ids > 0) {
            std::vector<int> bp(a->n_ids), bm(a->n_ids);
            std::vector<uint8_t> chosen(32 * (size_t)a->n_ids);
            row.push_back(-1);  // never empty
            distinctive_ref(a->n_ids, a->kf_desc, a->kf_cap * a->cap, off.data(), row.data(), a->max_obs, bp.data(),
                            bm.data(), chosen.data());
            for (int i = 0; i < a->n_ids; ++i) {
                if (a->best_pos) a->best_pos[i] = bp[i];
                if (a->best_median) a->best_median[i] = bm[i];
                if (bp[i] < 0) continue;
                memcpy(a->desc + 32 * (size_t)a->ids[i], chosen.data() + 32 * (size_t)i, 32);
                a->state[i] |= PLVI_REFRESH_DESC;
            }
        }
    }
    if (a->seconds) *a->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
