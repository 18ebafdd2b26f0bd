// loop_window_ref.cpp — a sequential host restatement of the integer work of
// LoopClosing::NewDetectCommonRegions between its matcher calls, in the reference's own shape:
// keyframe objects with an ordered covisible vector, the current keyframe's connected std::set,
// std::set<MapPoint*> membership, the push_back / [0] = window construction, whole vectors appended
// unconditionally, and the proximity break inside the j loop.  The expected values of
// tests/test_loop_window.py come from here; the test pins this file against an independent numpy
// restatement in the kernel's formulation.
//
//   DetectCommonRegionsFromBoW   src/LoopClosing.cc:794-858 (one candidate) and :893-915
//   FindMatchesByProjection      src/LoopClosing.cc:1157-1199
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <vector>

namespace {

struct MapPoint {
    int id;
    bool bad;
    bool isBad() const { return bad; }
};

struct KeyFrame {
    int slot;
    bool bad = false;
    bool ghost = false;  // a stored covisible that names no slot: listed, no table, no covisibles
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<MapPoint*> mvpMapPoints;
    bool isBad() const { return bad; }
    // KeyFrame.cc:255-263
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    const std::vector<MapPoint*>& GetMapPointMatches() const { return mvpMapPoints; }
};

struct Tables {
    int kf_cap, kp_cap, cand_stride;
    const uint8_t* bad;
    const int *mp, *nmp, *cand, *n_cand;
    int mp_n;
    const uint8_t* mp_bad;
};

struct Query {
    int kind, kf_slot, cur_slot, n_conn;
    const int* conn;
    int pt_cap;
    // BOW only: the six SearchByBoW results as indices into the member's table, NULL = windows only
    const int* matches12;  // [6][cap1]
    int n1, cap1;
    int *win, *n_win, *abort_at, *pts, *pts_kf, *n_pts, *err;
    int *matched_mp, *matched_kf, *num;
    double* seconds;
};

enum { BOW = 0, PROJ = 1, LAST = 2 };
enum { ERR_PTS = 1, ERR_UNDEFINED = 2, ERR_QUERY = 4 };

struct Map {
    std::vector<MapPoint> points;
    std::vector<KeyFrame> kfs;
    std::map<int, std::unique_ptr<KeyFrame>> ghosts;

    explicit Map(const Tables& t) : points(t.mp_n), kfs(t.kf_cap) {
        for (int i = 0; i < t.mp_n; ++i) points[i] = {i, t.mp_bad[i] != 0};
        for (int s = 0; s < t.kf_cap; ++s) {
            KeyFrame& k = kfs[s];
            k.slot = s;
            k.bad = t.bad[s] != 0;
            const int n = std::min(std::max(t.nmp[s], 0), t.kp_cap);
            for (int i = 0; i < n; ++i) {
                const int id = t.mp[(size_t)s * t.kp_cap + i];
                k.mvpMapPoints.push_back(id >= 0 && id < t.mp_n ? &points[id] : nullptr);
            }
        }
        for (int s = 0; s < t.kf_cap; ++s) {
            const int n = std::min(std::max(t.n_cand[s], 0), t.cand_stride);
            for (int i = 0; i < n; ++i) kfs[s].mvpOrderedConnectedKeyFrames.push_back(at(t.cand[(size_t)s * t.cand_stride + i]));
        }
    }
    KeyFrame* at(int slot) {
        if (slot >= 0 && slot < (int)kfs.size()) return &kfs[slot];
        std::unique_ptr<KeyFrame>& g = ghosts[slot];
        if (!g) {
            g.reset(new KeyFrame);
            g->slot = slot;
            g->ghost = true;
        }
        return g.get();
    }
};

void put_window(const std::vector<KeyFrame*>& w, const Query& q) {
    *q.n_win = (int)w.size();
    for (size_t i = 0; i < w.size(); ++i) q.win[i] = w[i]->slot;
}

void put_points(const std::vector<MapPoint*>& pts, const std::vector<KeyFrame*>* kfs, const Query& q, int* err) {
    *q.n_pts = (int)pts.size();
    for (int i = 0; i < (int)pts.size() && i < q.pt_cap; ++i) {
        q.pts[i] = pts[i]->id;
        if (kfs && q.pts_kf) q.pts_kf[i] = (*kfs)[i]->slot;
    }
    if ((int)pts.size() > q.pt_cap) *err |= ERR_PTS;
}

// :794-858 for one candidate pKFi
void bow(Map& map, const Query& q, int* err) {
    KeyFrame* pKFi = map.at(q.kf_slot);
    std::set<KeyFrame*> spConnectedKeyFrames;
    for (int i = 0; i < q.n_conn; ++i)
        if (q.conn[i] >= 0 && q.conn[i] < (int)map.kfs.size()) spConnectedKeyFrames.insert(&map.kfs[q.conn[i]]);
    const int nNumCovisibles = 5;
    if (!pKFi || pKFi->isBad()) return;

    std::vector<KeyFrame*> vpCovKFi = pKFi->GetBestCovisibilityKeyFrames(nNumCovisibles);
    if (vpCovKFi.empty()) {  // the reference reads vpCovKFi[0] of an empty vector
        *err |= ERR_UNDEFINED;
        vpCovKFi.push_back(pKFi);
    } else {
        vpCovKFi.push_back(vpCovKFi[0]);
        vpCovKFi[0] = pKFi;
    }
    put_window(vpCovKFi, q);

    std::vector<std::vector<MapPoint*>> vvpMatchedMPs;
    vvpMatchedMPs.resize(vpCovKFi.size());
    std::set<MapPoint*> spMatchedMPi;
    int numBoWMatches = 0;
    std::vector<MapPoint*> vpMatchedPoints(q.matches12 ? q.n1 : 0, static_cast<MapPoint*>(NULL));
    std::vector<KeyFrame*> vpKeyFrameMatchedMP(q.matches12 ? q.n1 : 0, static_cast<KeyFrame*>(NULL));

    for (int j = 0; j < (int)vpCovKFi.size(); ++j) {
        if (!vpCovKFi[j] || vpCovKFi[j]->isBad()) continue;
        if (!q.matches12 || vpCovKFi[j]->ghost) continue;
        // matcherBoW.SearchByBoW(mpCurrentKF, vpCovKFi[j], vvpMatchedMPs[j]): the matcher's index table
        // turned into the MapPoint vector it stands for
        const std::vector<MapPoint*>& vpMapPoints2 = vpCovKFi[j]->GetMapPointMatches();
        vvpMatchedMPs[j].assign(q.n1, static_cast<MapPoint*>(NULL));
        for (int k = 0; k < q.n1; ++k) {
            const int idx2 = q.matches12[(size_t)j * q.cap1 + k];
            if (idx2 >= 0 && idx2 < (int)vpMapPoints2.size()) vvpMatchedMPs[j][k] = vpMapPoints2[idx2];
        }
    }

    for (int j = 0; j < (int)vpCovKFi.size(); ++j) {
        if (spConnectedKeyFrames.find(vpCovKFi[j]) != spConnectedKeyFrames.end()) {
            *q.abort_at = j;  // bAbortByNearKF = true
            break;
        }
        for (int k = 0; k < (int)vvpMatchedMPs[j].size(); ++k) {
            MapPoint* pMPi_j = vvpMatchedMPs[j][k];
            if (!pMPi_j || pMPi_j->isBad()) continue;
            if (spMatchedMPi.find(pMPi_j) == spMatchedMPi.end()) {
                spMatchedMPi.insert(pMPi_j);
                numBoWMatches++;
                vpMatchedPoints[k] = pMPi_j;
                vpKeyFrameMatchedMP[k] = vpCovKFi[j];
            }
        }
    }
    if (q.matches12) {
        *q.num = numBoWMatches;
        for (int k = 0; k < q.n1; ++k) {
            q.matched_mp[k] = vpMatchedPoints[k] ? vpMatchedPoints[k]->id : -1;
            q.matched_kf[k] = vpKeyFrameMatchedMP[k] ? vpKeyFrameMatchedMP[k]->slot : -1;
        }
    }
}

// :893-915 around pMostBoWMatchesKF
void proj(Map& map, const Query& q, int* err) {
    KeyFrame* pMostBoWMatchesKF = map.at(q.kf_slot);
    const int nNumCovisibles = 5;
    std::vector<KeyFrame*> vpCovKFi = pMostBoWMatchesKF->GetBestCovisibilityKeyFrames(nNumCovisibles);
    vpCovKFi.push_back(pMostBoWMatchesKF);
    std::set<MapPoint*> spMapPoints;
    std::vector<MapPoint*> vpMapPoints;
    std::vector<KeyFrame*> vpKeyFrames;
    for (KeyFrame* pCovKFi : vpCovKFi) {
        for (MapPoint* pCovMPij : pCovKFi->GetMapPointMatches()) {
            if (!pCovMPij || pCovMPij->isBad()) continue;
            if (spMapPoints.find(pCovMPij) == spMapPoints.end()) {
                spMapPoints.insert(pCovMPij);
                vpMapPoints.push_back(pCovMPij);
                vpKeyFrames.push_back(pCovKFi);
            }
        }
    }
    put_window(vpCovKFi, q);
    put_points(vpMapPoints, &vpKeyFrames, q, err);
}

// :1161-1199 around pMatchedKFw; spCurrentCovisbles is the current keyframe's connected set
void last(Map& map, const Query& q, int* err) {
    KeyFrame* pMatchedKFw = map.at(q.kf_slot);
    int nNumCovisibles = 5;
    std::vector<KeyFrame*> vpCovKFm = pMatchedKFw->GetBestCovisibilityKeyFrames(nNumCovisibles);
    int nInitialCov = vpCovKFm.size();
    vpCovKFm.push_back(pMatchedKFw);
    std::set<KeyFrame*> spCheckKFs(vpCovKFm.begin(), vpCovKFm.end());
    std::set<KeyFrame*> spCurrentCovisbles;
    for (int i = 0; i < q.n_conn; ++i)
        if (q.conn[i] >= 0 && q.conn[i] < (int)map.kfs.size()) spCurrentCovisbles.insert(&map.kfs[q.conn[i]]);
    for (int i = 0; i < nInitialCov; ++i) {
        std::vector<KeyFrame*> vpKFs = vpCovKFm[i]->GetBestCovisibilityKeyFrames(nNumCovisibles);
        int nInserted = 0;
        int j = 0;
        while (j < (int)vpKFs.size() && nInserted < nNumCovisibles) {
            if (spCheckKFs.find(vpKFs[j]) == spCheckKFs.end() &&
                spCurrentCovisbles.find(vpKFs[j]) == spCurrentCovisbles.end()) {
                spCheckKFs.insert(vpKFs[j]);
                ++nInserted;
            }
            ++j;
        }
        vpCovKFm.insert(vpCovKFm.end(), vpKFs.begin(), vpKFs.end());
    }
    std::set<MapPoint*> spMapPoints;
    std::vector<MapPoint*> vpMapPoints;
    for (KeyFrame* pKFi : vpCovKFm) {
        for (MapPoint* pMPij : pKFi->GetMapPointMatches()) {
            if (!pMPij || pMPij->isBad()) continue;
            if (spMapPoints.find(pMPij) == spMapPoints.end()) {
                spMapPoints.insert(pMPij);
                vpMapPoints.push_back(pMPij);
            }
        }
    }
    put_window(vpCovKFm, q);
    put_points(vpMapPoints, nullptr, q, err);
}

}  // namespace

extern "C" void loop_window_ref_run(const Tables* t, int n_queries, const Query* qs) {
    Map map(*t);  // the objects are built once; the queries are timed without them
    for (int i = 0; i < n_queries; ++i) {
        Query q = qs[i];
        q.n1 = std::min(std::max(q.n1, 0), q.cap1);  // the count contract
        const auto t0 = std::chrono::steady_clock::now();
        int err = 0;
        const bool known = q.kind == BOW || q.kind == PROJ || q.kind == LAST;
        const bool slots = q.kf_slot >= 0 && q.kf_slot < t->kf_cap &&
                           (q.kind != BOW || (q.cur_slot >= 0 && q.cur_slot < t->kf_cap));
        *q.n_win = *q.n_pts = 0;
        *q.abort_at = -1;
        if (q.kind == BOW && q.matches12) {  // vpMatchedPoints / vpKeyFrameMatchedMP start as N NULLs
            *q.num = 0;
            std::fill(q.matched_mp, q.matched_mp + q.n1, -1);
            std::fill(q.matched_kf, q.matched_kf + q.n1, -1);
        }
        if (!known || !slots) {
            err = ERR_QUERY;
        } else if (q.kind == BOW) {
            bow(map, q, &err);
        } else if (q.kind == PROJ) {
            proj(map, q, &err);
        } else {
            last(map, q, &err);
        }
        *q.err = err;
        if (q.seconds) *q.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
}
