// essential_graph_ref.cpp — a sequential host restatement of the integer work of LoopClosing::CorrectLoop
// [WithLines] (src/LoopClosing.cc:1252-1253, :1294-1345, :1406-1424) and Optimizer::OptimizeEssentialGraph /
// OptimizeEssentialGraph4DoF (src/Optimizer.cc:6985-7021, :7030-7058, :7062-7190, :7235-7301; :14442-14660) in the
// reference's own shape: KeyFrame objects at ascending addresses given by `order`, std::map<KeyFrame*, ...> and
// std::set<KeyFrame*> iterated by address, map<KeyFrame*, set<KeyFrame*> > LoopConnections, set<pair<id, id> >
// sInsertedEdges, mspChildrens, mspLoopEdges, the stamp members on the feature objects.  UpdateConnections is the
// one of covis_ref.cpp, included unmodified.  The expected values of tests/test_essential_graph.py; compiled at
// test time.
#include "covis_ref.cpp"

#include <set>

namespace {

typedef unsigned long idt;  // long unsigned int mnId

struct EKeyFrame;

struct EFeature {  // MapPoint or MapLine
    int id = -1;
    bool bad = false;
    int mpMap = 0;
    EKeyFrame* mpRefKF = nullptr;
    idt mnCorrectedByKF = ~idt(0);     // no keyframe has this id: nothing stamped
    EKeyFrame* corrected = nullptr;    // mnCorrectedReference, kept as the keyframe
    int corr_ref_slot = -1;
    bool isBad() const { return bad; }
    EKeyFrame* GetReferenceKeyFrame() const { return mpRefKF; }
};

struct EKeyFrame {
    int slot = -1;
    idt mnId = 0;
    bool mbBad = true, named = false, init = false, bImu = false;
    int mpMap = 0;
    std::vector<EFeature*> mvpMapPoints, mvpMapLines;
    std::map<EKeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<EKeyFrame*> mvpOrderedConnectedKeyFrames;  // a NULL entry names no slot
    std::vector<int> mvOrderedWeights;
    EKeyFrame* mpParent = nullptr;
    std::set<EKeyFrame*> mspChildrens, mspLoopEdges;
    EKeyFrame *mPrevKF = nullptr, *mNextKF = nullptr;

    bool isBad() const { return mbBad; }
    EKeyFrame* GetParent() const { return mpParent; }
    bool hasChild(EKeyFrame* p) const { return mspChildrens.count(p); }
    std::set<EKeyFrame*> GetLoopEdges() const { return mspLoopEdges; }
    int GetWeight(EKeyFrame* pKF) {
        if (mConnectedKeyFrameWeights.count(pKF)) return mConnectedKeyFrameWeights[pKF];
        return 0;
    }
    static bool weightComp(int a, int b) { return a > b; }
    std::vector<EKeyFrame*> GetCovisiblesByWeight(const int& w) {
        if (mvpOrderedConnectedKeyFrames.empty()) return std::vector<EKeyFrame*>();
        std::vector<int>::iterator it = std::upper_bound(mvOrderedWeights.begin(), mvOrderedWeights.end(), w, weightComp);
        if (it == mvOrderedWeights.end() && mvOrderedWeights.back() < w) return std::vector<EKeyFrame*>();
        const int n = (int)(it - mvOrderedWeights.begin());
        return std::vector<EKeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
    }
};

}  // namespace

extern "C" {

struct EgRefTables {
    int kf_cap, kp_cap, kl_cap, cand_stride, n_order, map_stride, mp_n, ml_n;
    const uint8_t *bad, *init_kf;
    const int *mp, *nmp, *ml, *nml, *cand, *n_cand;
    const unsigned* kf_id;
    const int *prev_kf, *next_kf, *order, *map_id, *parent, *child_off, *child, *loop_off, *loop;
    const uint8_t* imu;
    const int *cand_w, *map_kf, *map_w, *map_n;
    const uint8_t* mp_bad;
    const int* mp_ref;
    unsigned* mp_by;
    int* mp_cref;
    const int* mp_map;
    const uint8_t* ml_bad;
    const int* ml_ref;
    unsigned* ml_by;
    int* ml_cref;
    const int* ml_map;
};
}

namespace {

int clampc(int v, int cap) { return v < 0 ? 0 : v > cap ? cap : v; }

struct EWorld {
    std::vector<EKeyFrame> kfs;
    std::vector<int> at;
    std::vector<EFeature> mps, mls;
    bool lines;
    EKeyFrame* kf(int s) { return s >= 0 && s < (int)at.size() ? &kfs[at[s]] : nullptr; }

    void pool(std::vector<EFeature>& v, int n, const uint8_t* bad, const int* ref, const unsigned* by, const int* cref,
              const int* map) {
        v.resize(n);
        for (int i = 0; i < n; ++i) {
            v[i].id = i;
            v[i].bad = bad[i] != 0;
            v[i].mpMap = map ? map[i] : 0;
            v[i].mpRefKF = ref ? kf(ref[i]) : nullptr;
            if (by) {
                v[i].mnCorrectedByKF = by[i];
                v[i].corr_ref_slot = cref[i];
            }
        }
    }

    explicit EWorld(const EgRefTables& t) : kfs(t.kf_cap), at(t.kf_cap, -1) {
        const int K = t.kf_cap;
        int next = 0;
        for (int i = 0; i < t.n_order; ++i)
            if (t.order[i] >= 0 && t.order[i] < K && at[t.order[i]] < 0) {
                at[t.order[i]] = next++;
                kfs[at[t.order[i]]].named = true;
            }
        for (int s = 0; s < K; ++s)
            if (at[s] < 0) at[s] = next++;
        lines = t.ml && t.ml_bad;
        pool(mps, t.mp_n, t.mp_bad, t.mp_ref, t.mp_by, t.mp_cref, t.mp_map);
        if (t.ml_bad) pool(mls, t.ml_n, t.ml_bad, t.ml_ref, t.ml_by, t.ml_cref, t.ml_map);
        for (int s = 0; s < K; ++s) {
            EKeyFrame& k = *kf(s);
            k.slot = s;
            k.mnId = t.kf_id[s];
            k.mbBad = t.bad[s] != 0;
            k.init = t.init_kf && t.init_kf[s];
            k.bImu = t.imu && t.imu[s];
            k.mpMap = t.map_id ? t.map_id[s] : 0;
            if (t.mp)
                for (int i = 0; i < clampc(t.nmp[s], t.kp_cap); ++i) {
                    const int id = t.mp[(size_t)s * t.kp_cap + i];
                    k.mvpMapPoints.push_back(id >= 0 && id < t.mp_n ? &mps[id] : nullptr);
                }
            if (lines)
                for (int i = 0; i < clampc(t.nml[s], t.kl_cap); ++i) {
                    const int id = t.ml[(size_t)s * t.kl_cap + i];
                    k.mvpMapLines.push_back(id >= 0 && id < t.ml_n ? &mls[id] : nullptr);
                }
            for (int i = 0; i < clampc(t.n_cand[s], t.cand_stride); ++i) {
                k.mvpOrderedConnectedKeyFrames.push_back(kf(t.cand[(size_t)s * t.cand_stride + i]));
                k.mvOrderedWeights.push_back(t.cand_w ? t.cand_w[(size_t)s * t.cand_stride + i] : 0);
            }
            if (t.map_n)
                for (int i = 0; i < clampc(t.map_n[s], t.map_stride); ++i)
                    if (kf(t.map_kf[(size_t)s * t.map_stride + i]))
                        k.mConnectedKeyFrameWeights[kf(t.map_kf[(size_t)s * t.map_stride + i])] =
                            t.map_w[(size_t)s * t.map_stride + i];
            k.mpParent = t.parent ? kf(t.parent[s]) : nullptr;
            if (t.child_off)
                for (int c = t.child_off[s]; c < t.child_off[s + 1]; ++c)
                    if (kf(t.child[c])) k.mspChildrens.insert(kf(t.child[c]));
            if (t.loop_off)
                for (int c = t.loop_off[s]; c < t.loop_off[s + 1]; ++c)
                    if (kf(t.loop[c])) k.mspLoopEdges.insert(kf(t.loop[c]));
            k.mPrevKF = t.prev_kf ? kf(t.prev_kf[s]) : nullptr;
            k.mNextKF = t.next_kf ? kf(t.next_kf[s]) : nullptr;
        }
    }
};

void put_list(const std::vector<int>& v, int cap, int* out) {
    for (size_t i = 0; i < v.size() && (int)i < cap; ++i) out[i] = v[i];
}

// :1294-1345 for one pool; against = the listed features whose owner is not the first member in WINDOW order
// that holds them
void correct_pool(std::map<EKeyFrame*, int>& CorrectedSim3, const std::vector<EKeyFrame*>& window, bool lns,
                  EKeyFrame* mpCurrentKF, bool stamp, std::vector<int>& ids, std::vector<int>& owners, int* against) {
    std::set<EFeature*> seen;  // with the stamps absent: met earlier in the walk
    for (std::map<EKeyFrame*, int>::iterator mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++) {
        EKeyFrame* pKFi = mit->first;
        std::vector<EFeature*> vpMPsi = lns ? pKFi->mvpMapLines : pKFi->mvpMapPoints;
        for (size_t iMP = 0, endMPi = vpMPsi.size(); iMP < endMPi; iMP++) {
            EFeature* pMPi = vpMPsi[iMP];
            if (!pMPi) continue;
            if (pMPi->isBad()) continue;
            if (pMPi->mnCorrectedByKF == mpCurrentKF->mnId) continue;
            if (!stamp && !seen.insert(pMPi).second) continue;
            EKeyFrame* first = nullptr;
            for (size_t w = 0; w < window.size() && !first; ++w) {
                if (!window[w]) continue;
                const std::vector<EFeature*>& v = lns ? window[w]->mvpMapLines : window[w]->mvpMapPoints;
                if (std::find(v.begin(), v.end(), pMPi) != v.end()) first = window[w];
            }
            if (first != pKFi) ++*against;
            ids.push_back(pMPi->id);
            owners.push_back(pKFi->slot);
            if (stamp) {
                pMPi->mnCorrectedByKF = mpCurrentKF->mnId;
                pMPi->corr_ref_slot = pKFi->slot;  // mnCorrectedReference = pKFi->mnId
            }
        }
    }
}

}  // namespace

// plvi_loop_correct.  against [1]: see correct_pool (points and lines together).
extern "C" void eg_ref_correct(const EgRefTables* tp, int cur, int win_cap, int pt_cap, int ln_cap, int* win, int* n_win,
                               int* win_sorted, int* n_sorted, int* pts, int* pts_kf, int* n_pts, int* lns, int* lns_kf,
                               int* n_lns, int* err, int* against, double* seconds) {
    const EgRefTables& t = *tp;
    *against = 0;
    if (cur < 0 || cur >= t.kf_cap) {
        *n_win = *n_sorted = *n_pts = *n_lns = 0;
        *err = 8;
        return;
    }
    EWorld w(t);
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    EKeyFrame* mpCurrentKF = w.kf(cur);
    std::vector<EKeyFrame*> mvpCurrentConnectedKFs = mpCurrentKF->mvpOrderedConnectedKeyFrames;  // :1252
    mvpCurrentConnectedKFs.push_back(mpCurrentKF);
    std::vector<int> v_win;
    for (int i = 0; i < clampc(t.n_cand[cur], t.cand_stride); ++i) v_win.push_back(t.cand[(size_t)cur * t.cand_stride + i]);
    v_win.push_back(cur);
    std::map<EKeyFrame*, int> CorrectedSim3;  // KeyFrameAndPose
    for (size_t i = 0; i < mvpCurrentConnectedKFs.size(); ++i)
        if (mvpCurrentConnectedKFs[i]) CorrectedSim3[mvpCurrentConnectedKFs[i]] = 1;
    std::vector<int> v_sorted, v_pts, v_pts_kf, v_lns, v_lns_kf;
    for (std::map<EKeyFrame*, int>::iterator mit = CorrectedSim3.begin(); mit != CorrectedSim3.end(); ++mit)
        v_sorted.push_back(mit->first->slot);
    correct_pool(CorrectedSim3, mvpCurrentConnectedKFs, false, mpCurrentKF, t.mp_by != nullptr, v_pts, v_pts_kf, against);
    if (w.lines)
        correct_pool(CorrectedSim3, mvpCurrentConnectedKFs, true, mpCurrentKF, t.ml_by != nullptr, v_lns, v_lns_kf, against);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    put_list(v_win, win_cap, win);
    put_list(v_sorted, win_cap, win_sorted);
    put_list(v_pts, pt_cap, pts);
    put_list(v_pts_kf, pt_cap, pts_kf);
    put_list(v_lns, ln_cap, lns);
    put_list(v_lns_kf, ln_cap, lns_kf);
    *n_win = (int)v_win.size();
    *n_sorted = (int)v_sorted.size();
    *n_pts = (int)v_pts.size();
    *n_lns = (int)v_lns.size();
    *err = ((int)v_win.size() > win_cap ? 1 : 0) | ((int)v_pts.size() > pt_cap ? 2 : 0) | ((int)v_lns.size() > ln_cap ? 4 : 0);
    if (t.mp_by)
        for (int i = 0; i < t.mp_n; ++i) {
            t.mp_by[i] = (unsigned)w.mps[i].mnCorrectedByKF;
            t.mp_cref[i] = w.mps[i].corr_ref_slot;
        }
    if (t.ml_by && w.lines)
        for (int i = 0; i < t.ml_n; ++i) {
            t.ml_by[i] = (unsigned)w.mls[i].mnCorrectedByKF;
            t.ml_cref[i] = w.mls[i].corr_ref_slot;
        }
}

namespace {

struct EdgeList {
    std::vector<int> a, b, kind;
    int n_kind[5] = {0, 0, 0, 0, 0};
    bool no_vertex = false;
    std::map<idt, EKeyFrame*>* vertices;
    // optimizer.vertex(id) of both ends; addEdge
    void add(EKeyFrame* i, EKeyFrame* j, int k) {
        if (!vertices->count(i->mnId) || !vertices->count(j->mnId)) no_vertex = true;
        a.push_back(i->slot);
        b.push_back(j->slot);
        kind.push_back(k);
        ++n_kind[k];
    }
};

}  // namespace

// plvi_essential_graph.  win [n_win] / lc_kf [n_win][lc_cap] / n_lc [n_win]: LoopConnections[win[p]] = row p, in
// window order (a later position overwrites).  suppressed [1] = the covisibility edges left out because the
// pair is in sInsertedEdges.
extern "C" void eg_ref_graph(const EgRefTables* tp, int cur, int loop, int mode, const int* win, int n_win,
                             const int* lc_kf, const int* n_lc, int lc_cap, int vert_cap, int edge_cap, int* vert,
                             int* vert_flags, int* n_vert, int* edge_a, int* edge_b, int* edge_kind, int* n_edges,
                             int* pt_ref, int* ln_ref, int* err, int* suppressed, double* seconds) {
    const EgRefTables& t = *tp;
    *suppressed = 0;
    if (cur < 0 || cur >= t.kf_cap || loop < 0 || loop >= t.kf_cap) {
        *n_vert = 0;
        for (int k = 0; k < 5; ++k) n_edges[k] = 0;
        *err = 8;
        return;
    }
    EWorld w(t);
    EKeyFrame *pCurKF = w.kf(cur), *pLoopKF = w.kf(loop);
    const int pMap = pCurKF->mpMap;
    std::set<EKeyFrame*> mspKeyFrames;  // Map::mspKeyFrames
    for (int s = 0; s < t.kf_cap; ++s)
        if (w.kf(s)->named && w.kf(s)->mpMap == pMap) mspKeyFrames.insert(w.kf(s));
    std::map<EKeyFrame*, std::set<EKeyFrame*> > LoopConnections;
    std::map<EKeyFrame*, int> CorrectedSim3;
    for (int p = 0; p < n_win; ++p) {
        EKeyFrame* pKFi = w.kf(win[p]);
        if (!pKFi) continue;
        CorrectedSim3[pKFi] = 1;
        std::set<EKeyFrame*> row;
        for (int e = 0; e < clampc(n_lc[p], lc_cap); ++e)
            if (w.kf(lc_kf[(size_t)p * lc_cap + e])) row.insert(w.kf(lc_kf[(size_t)p * lc_cap + e]));
        LoopConnections[pKFi] = row;
    }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    const std::vector<EKeyFrame*> vpKFs(mspKeyFrames.begin(), mspKeyFrames.end());  // GetAllKeyFrames()
    const int minFeat = 100;
    const bool four = mode == 1;
    std::vector<int> v_vert, v_flags;
    std::map<idt, EKeyFrame*> vpVertices;
    // Set KeyFrame vertices
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        EKeyFrame* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const bool corrected = CorrectedSim3.find(pKF) != CorrectedSim3.end();
        const bool fixed = four ? pKF == pLoopKF : pKF->init;  // mnId == pMap->GetInitKFid()
        v_vert.push_back(pKF->slot);
        v_flags.push_back((fixed ? 1 : 0) | (corrected ? 2 : 0));
        vpVertices[pKF->mnId] = pKF;
    }
    EdgeList E;
    E.vertices = &vpVertices;
    std::set<std::pair<idt, idt> > sInsertedEdges;
    // Set Loop edges
    for (std::map<EKeyFrame*, std::set<EKeyFrame*> >::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        EKeyFrame* pKF = mit->first;
        const idt nIDi = pKF->mnId;
        const std::set<EKeyFrame*>& spConnections = mit->second;
        for (std::set<EKeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const idt nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            E.add(pKF, *sit, 0);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    // Set normal edges
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {
        EKeyFrame* pKF = vpKFs[i];
        EKeyFrame* pParentKF = four ? static_cast<EKeyFrame*>(NULL) : pKF->GetParent();
        // Spanning tree edge
        if (pParentKF) E.add(pKF, pParentKF, 1);
        if (four) {
            EKeyFrame* prevKF = pKF->mPrevKF;
            if (prevKF) E.add(pKF, prevKF, 4);
        }
        // Loop edges
        const std::set<EKeyFrame*> sLoopEdges = pKF->GetLoopEdges();
        for (std::set<EKeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            EKeyFrame* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) E.add(pKF, pLKF, 2);
        }
        // Covisibility graph edges
        const std::vector<EKeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (std::vector<EKeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            EKeyFrame* pKFn = *vit;
            const bool chain = four && (pKFn == pKF->mPrevKF || pKFn == pKF->mNextKF);
            if (pKFn && pKFn != pParentKF && !chain && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) {
                        ++*suppressed;
                        continue;
                    }
                    E.add(pKF, pKFn, 3);
                }
            }
        }
        // Inertial edges if inertial
        if (!four && pKF->bImu && pKF->mPrevKF) E.add(pKF, pKF->mPrevKF, 4);
    }
    // Correct points: the keyframe each is mapped through
    for (int p = 0; p < 2; ++p) {
        int* out = p ? ln_ref : pt_ref;
        std::vector<EFeature>& v = p ? w.mls : w.mps;
        if (!out) continue;
        for (size_t i = 0; i < v.size(); ++i) {
            EFeature* pMP = &v[i];
            out[i] = -1;
            if (pMP->mpMap != pMap) continue;  // not in vpMPs = pMap->GetAllMapPoints()
            if (pMP->isBad()) continue;
            if (!four && pMP->mnCorrectedByKF == pCurKF->mnId)
                out[i] = pMP->corr_ref_slot;
            else
                out[i] = pMP->GetReferenceKeyFrame() ? pMP->GetReferenceKeyFrame()->slot : (p ? t.ml_ref[i] : t.mp_ref[i]);
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    put_list(v_vert, vert_cap, vert);
    put_list(v_flags, vert_cap, vert_flags);
    put_list(E.a, edge_cap, edge_a);
    put_list(E.b, edge_cap, edge_b);
    put_list(E.kind, edge_cap, edge_kind);
    *n_vert = (int)v_vert.size();
    for (int k = 0; k < 5; ++k) n_edges[k] = E.n_kind[k];
    *err = ((int)v_vert.size() > vert_cap ? 16 : 0) | ((int)E.a.size() > edge_cap ? 32 : 0) | (E.no_vertex ? 64 : 0);
}

// plvi_loop_connections on a covis_ref graph `h`: the arguments of covis_ref_update with the window for the
// queries; the outputs of the updates by window position.  one_shot [n_win][lc_cap] / n_one_shot: the rows a
// snapshot of every member taken before the first update would give.
extern "C" void eg_ref_connections(void* h, const uint8_t* kf_bad, const int* order, int n_order, const int* kf_mp,
                                   const int* kf_nmp, int kp_cap, const int* kf_ml, const int* kf_nml, int kl_cap,
                                   const int* map_id, const uint8_t* init_kf, uint8_t* first_conn, int* parent, int mp_n,
                                   const uint8_t* mp_bad, const int* mp_obs_off, const int* mp_obs_kf, int ml_n,
                                   const uint8_t* ml_bad, const int* ml_obs_off, const int* ml_obs_kf, int n_win,
                                   const int* win, int* n_counted, int* n_conn, int* kf_max, int* w_max, int* new_parent,
                                   int lc_cap, int* lc_kf, int* n_lc, int* err, int* one_shot, int* n_one_shot,
                                   double* seconds) {
    Graph& g = *static_cast<Graph*>(h);
    const bool with_lines = kf_ml != nullptr;
    World w(g, kf_bad, order, n_order);
    std::vector<Feature> mps, mls;
    build_pool(mps, mp_n, mp_bad, mp_obs_off, mp_obs_kf, w);
    if (with_lines) build_pool(mls, ml_n, ml_bad, ml_obs_off, ml_obs_kf, w);
    for (int s = 0; s < g.K; ++s) {
        KeyFrame& k = *w.kf(s);
        k.mpMap = map_id ? map_id[s] : 0;
        k.init = init_kf && init_kf[s];
        k.mbFirstConnection = first_conn && first_conn[s];
        k.mpParent = parent ? w.kf(parent[s]) : nullptr;
        for (int i = 0; i < clampc(kf_nmp[s], kp_cap); ++i) {
            const int id = kf_mp[(size_t)s * kp_cap + i];
            k.mvpMapPoints.push_back(id >= 0 && id < mp_n ? &mps[id] : nullptr);
        }
        if (with_lines)
            for (int i = 0; i < clampc(kf_nml[s], kl_cap); ++i) {
                const int id = kf_ml[(size_t)s * kl_cap + i];
                k.mvpMapLines.push_back(id >= 0 && id < ml_n ? &mls[id] : nullptr);
            }
    }
    std::vector<KeyFrame*> mvpCurrentConnectedKFs;
    for (int p = 0; p < n_win; ++p) mvpCurrentConnectedKFs.push_back(w.kf(win[p]));
    std::vector<std::vector<KeyFrame*> > before(n_win);
    for (int p = 0; p < n_win; ++p)
        if (mvpCurrentConnectedKFs[p]) before[p] = mvpCurrentConnectedKFs[p]->mvpOrderedConnectedKeyFrames;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::map<KeyFrame*, std::set<KeyFrame*> > LoopConnections;
    *err = 0;
    int p = 0;
    for (std::vector<KeyFrame*>::iterator vit = mvpCurrentConnectedKFs.begin(), vend = mvpCurrentConnectedKFs.end(); vit != vend; vit++, p++) {
        KeyFrame* pKFi = *vit;
        n_lc[p] = 0;
        if (one_shot) n_one_shot[p] = 0;
        if (!pKFi) continue;
        std::vector<KeyFrame*> vpPreviousNeighbors = pKFi->mvpOrderedConnectedKeyFrames;  // GetVectorCovisibleKeyFrames()
        // Update connections. Detect new links.
        pKFi->parentSet = false;
        KeyFrame* pmax = nullptr;
        int wmax = 0;
        n_counted[p] = pKFi->UpdateConnections(with_lines, &pmax, &wmax);
        n_conn[p] = n_counted[p] ? (int)pKFi->mvpOrderedConnectedKeyFrames.size() : 0;
        kf_max[p] = pmax ? pmax->slot : -1;
        w_max[p] = wmax;
        new_parent[p] = pKFi->parentSet ? pKFi->mpParent->slot : -1;
        std::set<KeyFrame*> connected;  // GetConnectedKeyFrames()
        for (std::map<KeyFrame*, int>::iterator mit = pKFi->mConnectedKeyFrameWeights.begin(); mit != pKFi->mConnectedKeyFrameWeights.end(); mit++)
            connected.insert(mit->first);
        LoopConnections[pKFi] = connected;
        for (std::vector<KeyFrame*>::iterator vit_prev = vpPreviousNeighbors.begin(), vend_prev = vpPreviousNeighbors.end(); vit_prev != vend_prev; vit_prev++)
            LoopConnections[pKFi].erase(*vit_prev);
        for (std::vector<KeyFrame*>::iterator vit2 = mvpCurrentConnectedKFs.begin(), vend2 = mvpCurrentConnectedKFs.end(); vit2 != vend2; vit2++)
            LoopConnections[pKFi].erase(*vit2);
        int e = 0;
        for (std::set<KeyFrame*>::iterator sit = LoopConnections[pKFi].begin(); sit != LoopConnections[pKFi].end(); ++sit, ++e)
            if (e < lc_cap) lc_kf[(size_t)p * lc_cap + e] = (*sit)->slot;
        n_lc[p] = e;
        if (e > lc_cap) *err = 128;
        if (one_shot) {
            std::set<KeyFrame*> s = connected;
            for (size_t i = 0; i < before[p].size(); ++i) s.erase(before[p][i]);
            for (size_t i = 0; i < mvpCurrentConnectedKFs.size(); ++i) s.erase(mvpCurrentConnectedKFs[i]);
            int o = 0;
            for (std::set<KeyFrame*>::iterator sit = s.begin(); sit != s.end(); ++sit, ++o)
                if (o < lc_cap) one_shot[(size_t)p * lc_cap + o] = (*sit)->slot;
            n_one_shot[p] = o;
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int s = 0; s < g.K; ++s) {
        KeyFrame& k = *w.kf(s);
        if (first_conn) first_conn[s] = k.mbFirstConnection ? 1 : 0;
        if (parent) parent[s] = k.mpParent ? k.mpParent->slot : -1;
    }
    w.store(g, nullptr);
}
