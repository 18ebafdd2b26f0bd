// cull_ref.cpp — a sequential host restatement of LocalMapping::KeyFrameCulling() /
// KeyFrameCullingWithLines() (src/LocalMapping.cc:1566-1718 / :1720-1964) in the reference's own
// shape: KeyFrame / MapPoint / MapLine objects, std::map observations copied per feature
// (GetObservations() returns by value), an nObs member kept apart from the map, EraseObservation
// and SetBadFlag with their cascade (a feature that dies is taken out of every observer's table),
// the mPrevKF / mNextKF pointers.  cv::norm is a table of verdicts by keyframe slot (-1 = the
// walk stops there).  It is the expected value of tests/test_cull.py and the one-thread context
// figure of tools/cull_bench.py; it shares no code with csrc/cull.hip.
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

namespace {

enum { END = 0, BREAK_ABORT = 1, BREAK_100 = 2, STOP_NEEDS_NORM = 3 };
enum {
    SKIP_INIT = 1, SKIP_BAD = 2, KEEP = 3, KEEP_FEW_KF = 4, KEEP_RECENT = 5, KEEP_NO_CHAIN = 6, KEEP_TIME = 7,
    KEEP_NORM = 8, CULLED = 9, CULLED_TIME = 10, CULLED_NORM = 11, NEEDS_NORM = 12, DEFERRED = 0x80
};
enum { KIND_POINTS = 1, KIND_LINES = 2, KIND_RELINKED = 4, KIND_DEFERRED = 8 };
enum { ERR_OUT = 1, ERR_CHANGED = 2 };

struct KeyFrame;
struct Map {
    int nKeyFrames = 0;
    int KeyFramesInMap() const { return nKeyFrames; }
};

struct MapPoint {
    bool mbBad = false;
    int nObs = 0;
    std::map<KeyFrame*, std::tuple<int, int>> mObservations;
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    std::map<KeyFrame*, std::tuple<int, int>> GetObservations() const { return mObservations; }
    void EraseObservation(KeyFrame* pKF);
    void SetBadFlag();
};

struct MapLine {
    bool mbBad = false;
    int nObs = 0;
    std::map<KeyFrame*, size_t> mObservations;
    bool isBad() const { return mbBad; }
    int Observations() const { return nObs; }
    std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
    void EraseObservation(KeyFrame* pKF);
    void SetBadFlag();
};

struct KeyFrame {
    int slot = 0;
    unsigned long mnId = 0;
    bool mbBad = false, init = false, mbNotErase = false, mbToBeErased = false;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapLine*> mvpMapLines;
    std::vector<uint8_t> kp_info, kl_info;  // octave, bit 6 left out by depth, bit 7 the erase takes 2
    KeyFrame *mPrevKF = nullptr, *mNextKF = nullptr;
    double mTimeStamp = 0;
    Map* mpMap = nullptr;
    bool isBad() const { return mbBad; }
    std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
    std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
    void EraseMapPointMatch(size_t idx) {
        if (idx < mvpMapPoints.size()) mvpMapPoints[idx] = nullptr;
    }
    void EraseMapLineMatch(size_t idx) {
        if (idx < mvpMapLines.size()) mvpMapLines[idx] = nullptr;
    }
    // KeyFrame.cc:870-: the connection and spanning-tree parts are not the walk's business
    bool SetBadFlag(bool with_lines) {
        if (init) return false;
        if (mbNotErase) {
            mbToBeErased = true;
            return false;
        }
        for (size_t i = 0; i < mvpMapPoints.size(); i++)
            if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
        if (with_lines)
            for (size_t i = 0; i < mvpMapLines.size(); i++)
                if (mvpMapLines[i]) mvpMapLines[i]->EraseObservation(this);
        mbBad = true;
        mpMap->nKeyFrames--;
        return true;
    }
};

void MapPoint::EraseObservation(KeyFrame* pKF) {
    bool bBad = false;
    if (mObservations.count(pKF)) {
        const int leftIndex = std::get<0>(mObservations[pKF]);
        if (leftIndex != -1) {
            if (pKF->kp_info[leftIndex] & 0x80)  // !mpCamera2 && mvuRight[leftIndex] >= 0
                nObs -= 2;
            else
                nObs--;
        }
        mObservations.erase(pKF);
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}

void MapPoint::SetBadFlag() {
    std::map<KeyFrame*, std::tuple<int, int>> obs;
    mbBad = true;
    obs = mObservations;
    mObservations.clear();
    for (auto mit = obs.begin(); mit != obs.end(); mit++) mit->first->EraseMapPointMatch(std::get<0>(mit->second));
}

void MapLine::EraseObservation(KeyFrame* pKF) {
    bool bBad = false;
    if (mObservations.count(pKF)) {
        const size_t idx = mObservations[pKF];
        if (pKF->kl_info[idx] & 0x80)  // both mvDepth_l >= 0
            nObs -= 2;
        else
            nObs--;
        mObservations.erase(pKF);
        if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
}

void MapLine::SetBadFlag() {
    std::map<KeyFrame*, size_t> obs;
    mbBad = true;
    obs = mObservations;
    mObservations.clear();
    for (auto mit = obs.begin(); mit != obs.end(); mit++) mit->first->EraseMapLineMatch(mit->second);
}

int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

struct cull_ref_tables {
    int kf_cap, kp_cap, kl_cap, cand_stride;
    const uint8_t *bad, *init_kf, *not_erase;
    const int *mp, *nmp, *ml, *nml;  // ml NULL = KeyFrameCulling()
    const uint8_t *kp_info, *kl_info;
    const int *cand, *n_cand;
    const unsigned* kf_id;
    const double* timestamp;
    const int *prev_kf, *next_kf;
    int mp_n;
    const uint8_t* mp_bad;
    const int *mp_obs_off, *mp_obs_kf, *mp_obs_idx, *mp_nobs;
    int ml_n;
    const uint8_t* ml_bad;
    const int *ml_obs_off, *ml_obs_kf, *ml_obs_idx, *ml_nobs;
    float redundant_th;
    int monocular, inertial, slam_mode;
};

struct cull_ref_query {
    int q_slot, abort_ba, n_kf_in_map, imu_init, inertial_ba2;
    const int* norm_verdict;  // [kf_cap] -1 = stop, 0 / 1 = norm < 0.02; NULL = all -1
    int out_cap, changed_cap;
    int *n_visited, *stop, *n_kf_out, *err;
    uint8_t* outcome;
    int *n_mps, *n_mls, *n_redundant;
    int *n_changed, *changed_slot, *changed_kind;
    int* n_dead;      // features that died during the walk (points + lines)
    double* seconds;  // of the walk alone
};

extern "C" void cull_ref_run(const cull_ref_tables* T, const cull_ref_query* Q) {
    const int K = T->kf_cap;
    const bool with_lines = T->ml != nullptr;
    Map map;
    map.nKeyFrames = Q->n_kf_in_map;
    std::vector<KeyFrame> kfs(K);
    std::vector<MapPoint> mps(T->mp_n > 0 ? T->mp_n : 0);
    std::vector<MapLine> mls(with_lines && T->ml_n > 0 ? T->ml_n : 0);
    for (int s = 0; s < K; ++s) {
        KeyFrame& kf = kfs[s];
        kf.slot = s;
        kf.mpMap = &map;
        kf.mbBad = T->bad[s];
        kf.init = T->init_kf && T->init_kf[s];
        kf.mbNotErase = T->not_erase && T->not_erase[s];
        if (T->inertial) {
            kf.mnId = T->kf_id[s];
            kf.mTimeStamp = T->timestamp[s];
            const int p = T->prev_kf[s], n = T->next_kf[s];
            kf.mPrevKF = p >= 0 && p < K ? &kfs[p] : nullptr;
            kf.mNextKF = n >= 0 && n < K ? &kfs[n] : nullptr;
        }
        if (T->kp_cap > 0 && !mps.empty()) {
            const int n = clampi(T->nmp[s], 0, T->kp_cap);
            kf.mvpMapPoints.resize(n, nullptr);
            for (int i = 0; i < n; ++i) {
                const int id = T->mp[(size_t)s * T->kp_cap + i];
                if (id >= 0 && id < (int)mps.size()) kf.mvpMapPoints[i] = &mps[id];
            }
            kf.kp_info.assign(T->kp_info + (size_t)s * T->kp_cap, T->kp_info + (size_t)(s + 1) * T->kp_cap);
        }
        if (with_lines && T->kl_cap > 0 && !mls.empty()) {
            const int n = clampi(T->nml[s], 0, T->kl_cap);
            kf.mvpMapLines.resize(n, nullptr);
            for (int i = 0; i < n; ++i) {
                const int id = T->ml[(size_t)s * T->kl_cap + i];
                if (id >= 0 && id < (int)mls.size()) kf.mvpMapLines[i] = &mls[id];
            }
            kf.kl_info.assign(T->kl_info + (size_t)s * T->kl_cap, T->kl_info + (size_t)(s + 1) * T->kl_cap);
        }
    }
    for (size_t id = 0; id < mps.size(); ++id) {
        MapPoint& p = mps[id];
        p.mbBad = T->mp_bad[id];
        for (int o = T->mp_obs_off[id]; o < T->mp_obs_off[id + 1]; ++o) {
            const int kf = T->mp_obs_kf[o], idx = T->mp_obs_idx[o];
            if (kf < 0 || kf >= K || idx < 0 || idx >= T->kp_cap) continue;
            p.mObservations[&kfs[kf]] = std::make_tuple(idx, -1);
        }
        p.nObs = T->mp_nobs ? T->mp_nobs[id] : T->mp_obs_off[id + 1] - T->mp_obs_off[id];
    }
    for (size_t id = 0; id < mls.size(); ++id) {
        MapLine& l = mls[id];
        l.mbBad = T->ml_bad[id];
        for (int o = T->ml_obs_off[id]; o < T->ml_obs_off[id + 1]; ++o) {
            const int kf = T->ml_obs_kf[o], idx = T->ml_obs_idx[o];
            if (kf < 0 || kf >= K || idx < 0 || idx >= T->kl_cap) continue;
            l.mObservations[&kfs[kf]] = (size_t)idx;
        }
        l.nObs = T->ml_nobs ? T->ml_nobs[id] : T->ml_obs_off[id + 1] - T->ml_obs_off[id];
    }
    int n_bad0 = 0;
    for (const MapPoint& p : mps) n_bad0 += p.mbBad;
    for (const MapLine& l : mls) n_bad0 += l.mbBad;

    int err = 0, n_changed = 0, stop = END;
    auto changed = [&](int slot, int kind) {
        if (n_changed < Q->changed_cap) {
            Q->changed_slot[n_changed] = slot;
            Q->changed_kind[n_changed] = kind;
        } else {
            err |= ERR_CHANGED;
        }
        ++n_changed;
    };
    auto record = [&](int pos, int code, int nMPs, int nMLs, int nRed) {
        if (pos < Q->out_cap) {
            Q->outcome[pos] = (uint8_t)code;
            Q->n_mps[pos] = nMPs;
            Q->n_mls[pos] = nMLs;
            Q->n_redundant[pos] = nRed;
        } else {
            err |= ERR_OUT;
        }
    };

    const auto t0 = std::chrono::steady_clock::now();
    // ---- the walk, as written in LocalMapping.cc
    const int Nd = 21;
    KeyFrame* mpCurrentKeyFrame = &kfs[Q->q_slot];
    std::vector<int> vpLocalKeyFrames(T->cand + (size_t)Q->q_slot * T->cand_stride,
                                      T->cand + (size_t)Q->q_slot * T->cand_stride +
                                          clampi(T->n_cand[Q->q_slot], 0, T->cand_stride));
    const float redundant_th = T->redundant_th;
    const bool mbMonocular = T->monocular, mbInertial = T->inertial;
    const bool bInitImu = Q->imu_init;
    int count = 0;
    unsigned int last_ID = 0;
    if (mbInertial) {
        int count = 0;
        KeyFrame* aux_KF = mpCurrentKeyFrame;
        while (count < Nd && aux_KF->mPrevKF) {
            aux_KF = aux_KF->mPrevKF;
            count++;
        }
        last_ID = aux_KF->mnId;
    }
    for (size_t v = 0; v < vpLocalKeyFrames.size(); v++) {
        count++;
        const int pos = count - 1, slot = vpLocalKeyFrames[v];
        if (slot < 0 || slot >= K) {
            record(pos, SKIP_BAD, 0, 0, 0);
            continue;
        }
        KeyFrame* pKF = &kfs[slot];
        if (pKF->init || pKF->isBad()) {
            record(pos, pKF->init ? SKIP_INIT : SKIP_BAD, 0, 0, 0);
            continue;
        }
        const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
        int nObs = 3;
        const int thObs = nObs;
        int nRedundantObservations = 0;
        int nMPs = 0;
        for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
            MapPoint* pMP = vpMapPoints[i];
            if (pMP) {
                if (!pMP->isBad()) {
                    if (!mbMonocular) {
                        if (pKF->kp_info[i] & 0x40) continue;
                    }
                    nMPs++;
                    if (pMP->Observations() > thObs) {
                        const int scaleLevel = pKF->kp_info[i] & 63;
                        const std::map<KeyFrame*, std::tuple<int, int>> observations = pMP->GetObservations();
                        int nObs = 0;
                        for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                            KeyFrame* pKFi = mit->first;
                            if (pKFi == pKF) continue;
                            const int scaleLeveli = pKFi->kp_info[std::get<0>(mit->second)] & 63;
                            if (scaleLeveli <= scaleLevel + 1) {
                                nObs++;
                                if (nObs > thObs) break;
                            }
                        }
                        if (!with_lines || T->slam_mode == 0) {
                            if (nObs > thObs) nRedundantObservations++;
                        }
                    }
                }
            }
        }
        int nMLs = 0;
        if (with_lines) {
            const std::vector<MapLine*> vpMapLines = pKF->GetMapLineMatches();
            for (size_t i = 0, iend = vpMapLines.size(); i < iend; i++) {
                MapLine* pML = vpMapLines[i];
                if (pML) {
                    if (!pML->isBad()) {
                        if (!mbMonocular) {
                            if (pKF->kl_info[i] & 0x40) continue;
                        }
                        nMLs++;
                        if (pML->Observations() > thObs) {
                            const int scaleLevel = pKF->kl_info[i] & 63;
                            const std::map<KeyFrame*, size_t> observations = pML->GetObservations();
                            int nObs = 0;
                            for (auto mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                                KeyFrame* pKFi = mit->first;
                                if (pKFi == pKF) continue;
                                const int scaleLeveli = pKFi->kl_info[mit->second] & 63;
                                if (scaleLeveli <= scaleLevel + 1) {
                                    nObs++;
                                    if (nObs >= thObs) break;
                                }
                            }
                            if (nObs >= thObs) nRedundantObservations++;
                        }
                    }
                }
            }
        }
        const int n = !with_lines ? nMPs : T->slam_mode == 0 ? nMPs + nMLs : nMLs;
        int code = KEEP;
        // volatile: the product is rounded to float before the compare, as vmulss / vcomiss do
        volatile float rhs = redundant_th * (float)n;
        if ((float)nRedundantObservations > rhs) {
            if (mbInertial) {
                if (map.KeyFramesInMap() <= Nd) {
                    record(pos, KEEP_FEW_KF, nMPs, nMLs, nRedundantObservations);
                    continue;
                }
                if (pKF->mnId > (mpCurrentKeyFrame->mnId - 2)) {
                    record(pos, KEEP_RECENT, nMPs, nMLs, nRedundantObservations);
                    continue;
                }
                code = KEEP_NO_CHAIN;
                if (pKF->mPrevKF && pKF->mNextKF) {
                    const float t = pKF->mNextKF->mTimeStamp - pKF->mPrevKF->mTimeStamp;
                    bool cull = false;
                    if ((bInitImu && (pKF->mnId < last_ID) && t < 3.) || (t < 0.5)) {
                        code = CULLED_TIME;
                        cull = true;
                    } else if (!Q->inertial_ba2 && t < 3) {
                        // cv::norm(...) < 0.02 stands between the two tests; it has no side effect
                        const int verdict = Q->norm_verdict ? Q->norm_verdict[slot] : -1;
                        if (verdict < 0) {
                            record(pos, NEEDS_NORM, nMPs, nMLs, nRedundantObservations);
                            stop = STOP_NEEDS_NORM;
                            break;
                        }
                        code = verdict ? CULLED_NORM : KEEP_NORM;
                        cull = verdict != 0;
                    } else {
                        code = KEEP_TIME;
                    }
                    if (cull) {
                        pKF->mNextKF->mPrevKF = pKF->mPrevKF;
                        pKF->mPrevKF->mNextKF = pKF->mNextKF;
                        pKF->mNextKF = nullptr;
                        pKF->mPrevKF = nullptr;
                        const bool gone = pKF->SetBadFlag(false);
                        changed(slot, KIND_RELINKED | (gone ? KIND_POINTS : KIND_DEFERRED));
                        if (!gone) code |= DEFERRED;
                    }
                }
            } else {
                code = CULLED;
                const bool gone = pKF->SetBadFlag(with_lines);
                changed(slot, gone ? KIND_POINTS | (with_lines ? KIND_LINES : 0) : KIND_DEFERRED);
                if (!gone) code |= DEFERRED;
            }
        }
        record(pos, code, nMPs, nMLs, nRedundantObservations);
        if ((count > 20 && Q->abort_ba) || count > 100) {
            stop = count > 20 && Q->abort_ba ? BREAK_ABORT : BREAK_100;
            break;
        }
    }
    const auto t1 = std::chrono::steady_clock::now();
    *Q->n_visited = count;
    *Q->stop = stop;
    *Q->n_kf_out = map.KeyFramesInMap();
    *Q->err = err;
    *Q->n_changed = n_changed;
    int n_bad1 = 0;
    for (const MapPoint& p : mps) n_bad1 += p.mbBad;
    for (const MapLine& l : mls) n_bad1 += l.mbBad;
    if (Q->n_dead) *Q->n_dead = n_bad1 - n_bad0;
    if (Q->seconds) *Q->seconds = std::chrono::duration<double>(t1 - t0).count();
}
