// ba_window_ref.cpp — the expected values of tests/test_ba_window.py: a sequential host restatement of the set-up
// and the edge loops of Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, num_fixedKF)
// (src/Optimizer.cc:4851-4960, :5048-5168), LocalBundleAdjustmentOnlyLines (:6181-6233, :6291-6337; its two Angle
// variants repeat the text) and LocalInertialBA (:9185-9307, :9521-9640) in the reference's own shape: KeyFrame /
// MapPoint / MapLine objects with mnBALocalForKF / mnBAFixedForKF members, std::list and list::remove, std::map
// observations keyed by KeyFrame* (the objects lie in one array, so a map iterates in slot order; the tables give
// every observation list in slot order), and the loop bodies as the reference's text.  What is not modelled is not
// here either: g2o, the two-camera branches, the covisible loop of :9255 (maxCovKF is 0: it leaves at its first
// test).  A pointer the reference would push uninitialised is a null pointer here and is not pushed.
#include <chrono>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <tuple>
#include <unordered_map>
#include <vector>

using namespace std;

extern "C" {
struct BaRefTables {
    int kf_cap, kp_cap, kl_cap, cand_stride;
    const uint8_t *bad, *init_kf;
    const int *mp, *nmp, *ml, *nml;
    const uint8_t* kp_info;
    const int *cand, *n_cand;
    const unsigned* kf_id;
    const int *prev_kf, *kf_map_id;
    int mp_n;
    const uint8_t* mp_bad;
    const int *mp_obs_off, *mp_obs_kf, *mp_obs_idx, *mp_map_id;
    int ml_n;
    const uint8_t* ml_bad;
    const int *ml_obs_off, *ml_obs_kf, *ml_obs_idx, *ml_map_id;
    int mode, max_opt;
};
struct BaRefQuery {
    int q_slot, n_kf_in_map;
    int lkf_cap, fkf_cap, feat_cap, edge_cap;
    int *local_kf, *n_local_kf, *fixed_kf, *n_fixed_kf, *num_fixed, *init_in_local, *non_fixed, *local_feat,
        *n_local_feat, *edge_feat, *edge_kf, *edge_idx, *edge_cam;
    uint8_t* edge_kind;
    int *n_mono, *n_stereo, *n_line, *err;
    double* seconds;  // of the walk alone, the objects built before
};
}

namespace {

enum { POINTS = 0, LINES = 1, INERTIAL = 2 };
enum { MONO = 0, STEREO = 1, LINE = 2 };
enum { ERR_LOCAL_KF = 1, ERR_FIXED_KF = 2, ERR_FEAT = 4, ERR_EDGE = 8, ERR_UNDEFINED = 16, ERR_QUERY = 32 };

struct Map {
    unsigned long initKFid;
    long nKFs;
    unsigned long GetInitKFid() { return initKFid; }
    long KeyFramesInMap() { return nKFs; }
};
struct MapPoint;
struct MapLine;
struct KeyFrame {
    unsigned long mnId = 0, mnBALocalForKF = 0, mnBAFixedForKF = 0;
    int slot = 0;
    bool mbBad = false;
    Map* mpMap = nullptr;
    KeyFrame* mPrevKF = nullptr;
    vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    vector<MapPoint*> mvpMapPoints;
    vector<MapLine*> mvpMapLines;
    vector<float> mvuRight;
    bool isBad() { return mbBad; }
    Map* GetMap() { return mpMap; }
    vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    vector<MapLine*> GetMapLineMatches() { return mvpMapLines; }
};
struct MapPoint {
    int id = 0;
    unsigned long mnBALocalForKF = 0;
    bool mbBad = false;
    Map* mpMap = nullptr;
    map<KeyFrame*, tuple<int, int>> mObservations;
    bool isBad() { return mbBad; }
    Map* GetMap() { return mpMap; }
    map<KeyFrame*, tuple<int, int>> GetObservations() { return mObservations; }
};
struct MapLine {
    int id = 0;
    unsigned long mnBALocalForKF = 0;
    bool mbBad = false;
    Map* mpMap = nullptr;
    map<KeyFrame*, size_t> mObservations;
    bool isBad() { return mbBad; }
    Map* GetMap() { return mpMap; }
    map<KeyFrame*, size_t> GetObservations() { return mObservations; }
};

struct Edge {
    int feat, kf, idx, kind;
};

struct World {
    vector<KeyFrame> kfs;
    vector<MapPoint> mps;
    vector<MapLine> mls;
    map<int, Map> maps;
    Map* map_of(int id) { return &maps[id]; }
};

int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

void build(World& w, const BaRefTables& t, int q_slot, int n_kf_in_map) {
    const int K = t.kf_cap;
    w.kfs.resize(K);
    for (int s = 0; s < K; ++s) {
        KeyFrame& k = w.kfs[s];
        k.slot = s;
        k.mnId = t.kf_id ? t.kf_id[s] : (unsigned long)s + 1;
        k.mbBad = t.bad[s];
        k.mpMap = w.map_of(t.kf_map_id ? t.kf_map_id[s] : 0);
    }
    for (auto& m : w.maps) {
        m.second.initKFid = ~0ul;  // a map's initial keyframe is the one init_kf names, if any
        m.second.nKFs = n_kf_in_map;
    }
    for (int s = 0; s < K; ++s) {
        KeyFrame& k = w.kfs[s];
        if (t.init_kf && t.init_kf[s]) k.mpMap->initKFid = k.mnId;
        if (t.prev_kf && (unsigned)t.prev_kf[s] < (unsigned)K) k.mPrevKF = &w.kfs[t.prev_kf[s]];
        if (t.cand && t.n_cand)
            for (int p = 0, n = clampi(t.n_cand[s], 0, t.cand_stride); p < n; ++p) {
                const int c = t.cand[(size_t)s * t.cand_stride + p];
                if ((unsigned)c < (unsigned)K) k.mvpOrderedConnectedKeyFrames.push_back(&w.kfs[c]);
            }
    }
    w.mps.resize(t.mode == LINES ? 0 : t.mp_n);
    for (size_t i = 0; i < w.mps.size(); ++i) {
        MapPoint& p = w.mps[i];
        p.id = (int)i;
        p.mbBad = t.mp_bad[i];
        p.mpMap = w.map_of(t.mp_map_id ? t.mp_map_id[i] : 0);
        for (int o = t.mp_obs_off[i]; o < t.mp_obs_off[i + 1]; ++o)
            if ((unsigned)t.mp_obs_kf[o] < (unsigned)K)
                p.mObservations[&w.kfs[t.mp_obs_kf[o]]] = make_tuple(t.mp_obs_idx[o], -1);
    }
    w.mls.resize(t.mode == LINES ? t.ml_n : 0);
    for (size_t i = 0; i < w.mls.size(); ++i) {
        MapLine& l = w.mls[i];
        l.id = (int)i;
        l.mbBad = t.ml_bad[i];
        l.mpMap = w.map_of(t.ml_map_id ? t.ml_map_id[i] : 0);
        for (int o = t.ml_obs_off[i]; o < t.ml_obs_off[i + 1]; ++o)
            if ((unsigned)t.ml_obs_kf[o] < (unsigned)K) l.mObservations[&w.kfs[t.ml_obs_kf[o]]] = (size_t)(long)t.ml_obs_idx[o];
    }
    for (int s = 0; s < K; ++s) {
        KeyFrame& k = w.kfs[s];
        if (t.mode != LINES && t.kp_cap > 0) {
            const int n = clampi(t.nmp[s], 0, t.kp_cap);
            k.mvuRight.assign(t.kp_cap, -1.f);
            for (int i = 0; i < t.kp_cap; ++i)
                if (t.kp_info && (t.kp_info[(size_t)s * t.kp_cap + i] & 0x80)) k.mvuRight[i] = 1.f;
            for (int i = 0; i < n; ++i) {
                const int id = t.mp[(size_t)s * t.kp_cap + i];
                k.mvpMapPoints.push_back((unsigned)id < (unsigned)t.mp_n ? &w.mps[id] : nullptr);
            }
        }
        if (t.mode == LINES && t.kl_cap > 0) {
            const int n = clampi(t.nml[s], 0, t.kl_cap);
            for (int i = 0; i < n; ++i) {
                const int id = t.ml[(size_t)s * t.kl_cap + i];
                k.mvpMapLines.push_back((unsigned)id < (unsigned)t.ml_n ? &w.mls[id] : nullptr);
            }
        }
    }
    // the same initial keyframe for every map: pMap of the call is the current keyframe's map
    (void)q_slot;
}

struct Result {
    list<KeyFrame*> local, fixed;
    vector<KeyFrame*> optimizable;
    vector<int> feats;
    vector<Edge> edges;
    int num_fixedKF = 0, init_in_local = 0, err = 0;
    bool bNonFixed = false;
};

// ---- Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, int&)
void LocalBundleAdjustment(KeyFrame* pKF, Map* pMap, int& num_fixedKF, int kp_cap, Result& r) {
    list<KeyFrame*>& lLocalKeyFrames = r.local;

    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    Map* pCurrentMap = pKF->GetMap();

    const vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame* pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lLocalKeyFrames.push_back(pKFi);
    }

    num_fixedKF = 0;
    list<MapPoint*> lLocalMapPoints;
    for (list<KeyFrame*>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        KeyFrame* pKFi = *lit;
        if (pKFi->mnId == pMap->GetInitKFid()) {
            num_fixedKF = 1;
        }
        vector<MapPoint*> vpMPs = pKFi->GetMapPointMatches();
        for (vector<MapPoint*>::iterator vit = vpMPs.begin(), vend = vpMPs.end(); vit != vend; vit++) {
            MapPoint* pMP = *vit;
            if (pMP)
                if (!pMP->isBad() && pMP->GetMap() == pCurrentMap) {
                    if (pMP->mnBALocalForKF != pKF->mnId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = pKF->mnId;
                    }
                }
        }
    }
    r.init_in_local = num_fixedKF;

    list<KeyFrame*>& lFixedCameras = r.fixed;
    for (list<MapPoint*>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        map<KeyFrame*, tuple<int, int>> observations = (*lit)->GetObservations();
        for (map<KeyFrame*, tuple<int, int>>::iterator mit = observations.begin(), mend = observations.end();
             mit != mend; mit++) {
            KeyFrame* pKFi = mit->first;

            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
            }
        }
    }
    num_fixedKF = lFixedCameras.size() + num_fixedKF;
    if (num_fixedKF < 2) {
        list<KeyFrame*>::iterator lit = lLocalKeyFrames.begin();
        int lowerId = pKF->mnId;
        KeyFrame* pLowerKf = nullptr;  // uninitialised in the reference
        int secondLowerId = pKF->mnId;
        KeyFrame* pSecondLowerKF = nullptr;  // uninitialised in the reference

        for (; lit != lLocalKeyFrames.end(); lit++) {
            KeyFrame* pKFi = *lit;
            if (pKFi == pKF || pKFi->mnId == pMap->GetInitKFid()) {
                continue;
            }

            if (pKFi->mnId < lowerId) {  // unsigned long against int: the int is converted (sign-extended)
                lowerId = pKFi->mnId;
                pLowerKf = pKFi;
            } else if (pKFi->mnId < secondLowerId) {
                secondLowerId = pKFi->mnId;
                pSecondLowerKF = pKFi;
            }
        }
        if (pLowerKf) {
            lFixedCameras.push_back(pLowerKf);
            lLocalKeyFrames.remove(pLowerKf);
        } else {
            r.err |= ERR_UNDEFINED;
        }
        num_fixedKF++;
        if (num_fixedKF < 2) {
            if (pSecondLowerKF) {
                lFixedCameras.push_back(pSecondLowerKF);
                lLocalKeyFrames.remove(pSecondLowerKF);
            } else {
                r.err |= ERR_UNDEFINED;
            }
            num_fixedKF++;
        }
    }

    // :5048-5168
    int j = 0;
    for (list<MapPoint*>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend;
         lit++, j++) {
        MapPoint* pMP = *lit;
        r.feats.push_back(pMP->id);
        const map<KeyFrame*, tuple<int, int>> observations = pMP->GetObservations();
        for (map<KeyFrame*, tuple<int, int>>::const_iterator mit = observations.begin(), mend = observations.end();
             mit != mend; mit++) {
            KeyFrame* pKFi = mit->first;

            if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) {
                const int leftIndex = get<0>(mit->second);
                if ((unsigned)leftIndex >= (unsigned)kp_cap) continue;  // outside the keyframe's row: no edge

                if (leftIndex != -1 && pKFi->mvuRight[get<0>(mit->second)] < 0) {
                    r.edges.push_back({j, pKFi->slot, leftIndex, MONO});
                } else if (leftIndex != -1 && pKFi->mvuRight[get<0>(mit->second)] >= 0) {
                    r.edges.push_back({j, pKFi->slot, leftIndex, STEREO});
                }
            }
        }
    }
}

// ---- Optimizer::LocalBundleAdjustmentOnlyLines(KeyFrame*, bool*, Map*)
void LocalBundleAdjustmentOnlyLines(KeyFrame* pKF, Map* pMap, int kl_cap, Result& r) {
    list<KeyFrame*>& lLocalKeyFrames = r.local;

    lLocalKeyFrames.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    Map* pCurrentMap = pKF->GetMap();

    const vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
    for (int i = 0, iend = vNeighKFs.size(); i < iend; i++) {
        KeyFrame* pKFi = vNeighKFs[i];
        pKFi->mnBALocalForKF = pKF->mnId;
        if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
    }

    list<MapLine*> lLocalMapLines;
    for (list<KeyFrame*>::iterator lit = lLocalKeyFrames.begin(), lend = lLocalKeyFrames.end(); lit != lend; lit++) {
        if ((*lit)->mnId == (*lit)->GetMap()->GetInitKFid()) r.init_in_local = 1;  // not in the reference: an output of ours
        vector<MapLine*> vpMLs = (*lit)->GetMapLineMatches();
        for (vector<MapLine*>::iterator vit = vpMLs.begin(), vend = vpMLs.end(); vit != vend; vit++) {
            MapLine* pML = *vit;
            if (pML)
                if (!pML->isBad() && pML->GetMap() == pCurrentMap)
                    if (pML->mnBALocalForKF != pKF->mnId) {
                        lLocalMapLines.push_back(pML);
                        pML->mnBALocalForKF = pKF->mnId;
                    }
        }
    }

    list<KeyFrame*>& lFixedCameras = r.fixed;
    for (list<MapLine*>::iterator lit = lLocalMapLines.begin(), lend = lLocalMapLines.end(); lit != lend; lit++) {
        map<KeyFrame*, size_t> observations_l = (*lit)->GetObservations();
        for (map<KeyFrame*, size_t>::iterator mit = observations_l.begin(), mend = observations_l.end(); mit != mend;
             mit++) {
            KeyFrame* pKFi = mit->first;

            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) lFixedCameras.push_back(pKFi);
            }
        }
    }
    r.num_fixedKF = lFixedCameras.size();

    // :6291-6337
    int j = 0;
    for (list<MapLine*>::iterator lit = lLocalMapLines.begin(), lend = lLocalMapLines.end(); lit != lend; lit++, j++) {
        MapLine* pML = *lit;
        r.feats.push_back(pML->id);
        const map<KeyFrame*, size_t> observations = pML->GetObservations();
        for (map<KeyFrame*, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend;
             mit++) {
            KeyFrame* pKFi = mit->first;

            if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) {
                if (mit->second >= (size_t)kl_cap) continue;  // outside the keyframe's row: no edge
                r.edges.push_back({j, pKFi->slot, (int)mit->second, LINE});
            }
        }
    }
}

// ---- Optimizer::LocalInertialBA(KeyFrame*, bool*, Map*, bool bLarge, bool bRecInit)
void LocalInertialBA(KeyFrame* pKF, Map* pMap, int maxOpt, int kp_cap, Result& r) {
    Map* pCurrentMap = pKF->GetMap();
    (void)pMap;

    const int Nd = std::min((int)pCurrentMap->KeyFramesInMap() - 2, maxOpt);

    vector<KeyFrame*>& vpOptimizableKFs = r.optimizable;
    const vector<KeyFrame*> vpNeighsKFs = pKF->GetVectorCovisibleKeyFrames();
    list<KeyFrame*> lpOptVisKFs;

    vpOptimizableKFs.reserve(Nd > 0 ? Nd : 0);
    vpOptimizableKFs.push_back(pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    for (int i = 1; i < Nd; i++) {
        if (vpOptimizableKFs.back()->mPrevKF) {
            vpOptimizableKFs.push_back(vpOptimizableKFs.back()->mPrevKF);
            vpOptimizableKFs.back()->mnBALocalForKF = pKF->mnId;
        } else
            break;
    }

    int N = vpOptimizableKFs.size();

    list<MapPoint*> lLocalMapPoints;
    for (int i = 0; i < N; i++) {
        if (vpOptimizableKFs[i]->mnId == vpOptimizableKFs[i]->GetMap()->GetInitKFid())
            r.init_in_local = 1;  // not in the reference: an output of ours
        vector<MapPoint*> vpMPs = vpOptimizableKFs[i]->GetMapPointMatches();
        for (vector<MapPoint*>::iterator vit = vpMPs.begin(), vend = vpMPs.end(); vit != vend; vit++) {
            MapPoint* pMP = *vit;
            if (pMP)
                if (!pMP->isBad())
                    if (pMP->mnBALocalForKF != pKF->mnId) {
                        lLocalMapPoints.push_back(pMP);
                        pMP->mnBALocalForKF = pKF->mnId;
                    }
        }
    }

    list<KeyFrame*>& lFixedKeyFrames = r.fixed;
    if (vpOptimizableKFs.back()->mPrevKF) {
        lFixedKeyFrames.push_back(vpOptimizableKFs.back()->mPrevKF);
        vpOptimizableKFs.back()->mPrevKF->mnBAFixedForKF = pKF->mnId;
    } else {
        vpOptimizableKFs.back()->mnBALocalForKF = 0;
        vpOptimizableKFs.back()->mnBAFixedForKF = pKF->mnId;
        lFixedKeyFrames.push_back(vpOptimizableKFs.back());
        vpOptimizableKFs.pop_back();
    }

    const int maxCovKF = 0;
    for (int i = 0, iend = vpNeighsKFs.size(); i < iend; i++) {
        if ((int)lpOptVisKFs.size() >= maxCovKF) break;
    }

    const int maxFixKF = 200;

    for (list<MapPoint*>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend; lit++) {
        map<KeyFrame*, tuple<int, int>> observations = (*lit)->GetObservations();
        for (map<KeyFrame*, tuple<int, int>>::iterator mit = observations.begin(), mend = observations.end();
             mit != mend; mit++) {
            KeyFrame* pKFi = mit->first;

            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) {
                    lFixedKeyFrames.push_back(pKFi);
                    break;
                }
            }
        }
        if (lFixedKeyFrames.size() >= (size_t)maxFixKF) break;
    }

    r.bNonFixed = (lFixedKeyFrames.size() == 0);
    r.num_fixedKF = lFixedKeyFrames.size();

    // :9521-9640
    int j = 0;
    for (list<MapPoint*>::iterator lit = lLocalMapPoints.begin(), lend = lLocalMapPoints.end(); lit != lend;
         lit++, j++) {
        MapPoint* pMP = *lit;
        r.feats.push_back(pMP->id);
        const map<KeyFrame*, tuple<int, int>> observations = pMP->GetObservations();
        for (map<KeyFrame*, tuple<int, int>>::const_iterator mit = observations.begin(), mend = observations.end();
             mit != mend; mit++) {
            KeyFrame* pKFi = mit->first;

            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) continue;

            if (!pKFi->isBad() && pKFi->GetMap() == pCurrentMap) {
                const int leftIndex = get<0>(mit->second);
                if ((unsigned)leftIndex >= (unsigned)kp_cap) continue;  // outside the keyframe's row: no edge

                if (leftIndex != -1 && pKFi->mvuRight[leftIndex] < 0) {
                    r.edges.push_back({j, pKFi->slot, leftIndex, MONO});
                } else if (leftIndex != -1) {
                    r.edges.push_back({j, pKFi->slot, leftIndex, STEREO});
                }
            }
        }
    }
}

template <class L>
void put_list(const L& l, int* dst, int cap, int* n, int bit, int& err) {
    int i = 0;
    for (KeyFrame* k : l) {
        if (i < cap) dst[i] = k->slot;
        ++i;
    }
    *n = i;
    if (i > cap) err |= bit;
}

}  // namespace

extern "C" void ba_window_ref_run(const BaRefTables* t, BaRefQuery* q) {
    if ((unsigned)q->q_slot >= (unsigned)t->kf_cap) {
        *q->n_local_kf = *q->n_fixed_kf = *q->num_fixed = *q->init_in_local = *q->n_local_feat = 0;
        *q->n_mono = *q->n_stereo = *q->n_line = 0;
        *q->non_fixed = 1;
        *q->err = ERR_QUERY;
        if (q->seconds) *q->seconds = 0;
        return;
    }
    World w;
    build(w, *t, q->q_slot, q->n_kf_in_map);
    KeyFrame* pKF = &w.kfs[q->q_slot];
    Result r;
    const auto t0 = chrono::steady_clock::now();
    if (t->mode == POINTS)
        LocalBundleAdjustment(pKF, pKF->GetMap(), r.num_fixedKF, t->kp_cap, r);
    else if (t->mode == LINES)
        LocalBundleAdjustmentOnlyLines(pKF, pKF->GetMap(), t->kl_cap, r);
    else
        LocalInertialBA(pKF, pKF->GetMap(), t->max_opt, t->kp_cap, r);
    if (q->seconds) *q->seconds = chrono::duration<double>(chrono::steady_clock::now() - t0).count();

    int err = r.err;
    if (t->mode == INERTIAL)
        put_list(r.optimizable, q->local_kf, q->lkf_cap, q->n_local_kf, ERR_LOCAL_KF, err);
    else
        put_list(r.local, q->local_kf, q->lkf_cap, q->n_local_kf, ERR_LOCAL_KF, err);
    put_list(r.fixed, q->fixed_kf, q->fkf_cap, q->n_fixed_kf, ERR_FIXED_KF, err);
    *q->num_fixed = r.num_fixedKF;
    *q->init_in_local = r.init_in_local;
    *q->non_fixed = r.fixed.empty();
    for (size_t i = 0; i < r.feats.size() && (int)i < q->feat_cap; ++i) q->local_feat[i] = r.feats[i];
    *q->n_local_feat = (int)r.feats.size();
    if ((int)r.feats.size() > q->feat_cap) err |= ERR_FEAT;
    // the vertex order: local (optimizable) then fixed; a keyframe's first position
    unordered_map<int, int> cam;
    int pos = 0;
    if (t->mode == INERTIAL)
        for (KeyFrame* k : r.optimizable) cam.emplace(k->slot, pos++);
    else
        for (KeyFrame* k : r.local) cam.emplace(k->slot, pos++);
    for (KeyFrame* k : r.fixed) cam.emplace(k->slot, pos++);
    int n_kind[3] = {0, 0, 0};
    for (size_t e = 0; e < r.edges.size(); ++e) {
        const Edge& ed = r.edges[e];
        ++n_kind[ed.kind];
        if ((int)e >= q->edge_cap) continue;
        q->edge_feat[e] = ed.feat;
        q->edge_kf[e] = ed.kf;
        q->edge_idx[e] = ed.idx;
        const auto it = cam.find(ed.kf);
        q->edge_cam[e] = it == cam.end() ? -1 : it->second;
        q->edge_kind[e] = (uint8_t)ed.kind;
    }
    if ((int)r.edges.size() > q->edge_cap) err |= ERR_EDGE;
    *q->n_mono = n_kind[MONO];
    *q->n_stereo = n_kind[STEREO];
    *q->n_line = n_kind[LINE];
    *q->err = err;
}
