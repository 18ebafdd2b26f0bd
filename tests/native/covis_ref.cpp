// covis_ref.cpp — a sequential host restatement of KeyFrame::UpdateConnections[WithLines]
// (src/KeyFrame.cc:499-622 / :624-769), AddConnection (:201-214), UpdateBestCovisibles (:216-238),
// EraseConnection (:1154-1168), the connection part of SetBadFlag (:894-897, :915-916),
// GetCovisiblesByWeight (:265-286) and GetWeight (:288-295) in the reference's own shape: KeyFrame
// objects and pointers, std::map<KeyFrame*, int> iterated by address, vector<pair<int, KeyFrame*>>
// + std::sort + push_front, AddConnection with its early return, and the queries of a batch
// applied one by one.  The expected values of tests/test_covis.py; compiled at test time.
//
// Addresses: the keyframe objects live in one array, placed so that ascending address is the
// caller's `order` (slots it does not name follow, by slot, and are not part of the map: they are
// never counted).  The graph is kept between calls by slot and turned into objects for each call,
// so `order` and the bad flags may change from call to call.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <list>
#include <map>
#include <utility>
#include <vector>

namespace {

struct KeyFrame;

struct Feature {  // MapPoint or MapLine
    bool bad = false;
    std::map<KeyFrame*, int> mObservations;
    bool isBad() const { return bad; }
    std::map<KeyFrame*, int> GetObservations() const { return mObservations; }
};

struct KeyFrame {
    int slot = -1;
    bool mbBad = true, named = false, init = false;
    int mpMap = 0;
    std::vector<Feature*> mvpMapPoints, mvpMapLines;
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;
    bool mbFirstConnection = false;
    KeyFrame* mpParent = nullptr;
    bool touched = false, parentSet = false;

    bool isBad() const { return mbBad; }

    void UpdateBestCovisibles() {
        std::vector<std::pair<int, KeyFrame*> > vPairs;
        vPairs.reserve(mConnectedKeyFrameWeights.size());
        for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(), mend = mConnectedKeyFrameWeights.end(); mit != mend; mit++)
            vPairs.push_back(std::make_pair(mit->second, mit->first));
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KeyFrame*> lKFs;
        std::list<int> lWs;
        for (size_t i = 0, iend = vPairs.size(); i < iend; i++) {
            if (!vPairs[i].second->isBad()) {
                lKFs.push_front(vPairs[i].second);
                lWs.push_front(vPairs[i].first);
            }
        }
        mvpOrderedConnectedKeyFrames = std::vector<KeyFrame*>(lKFs.begin(), lKFs.end());
        mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
        touched = true;
    }

    void AddConnection(KeyFrame* pKF, const int& weight) {
        if (!mConnectedKeyFrameWeights.count(pKF))
            mConnectedKeyFrameWeights[pKF] = weight;
        else if (mConnectedKeyFrameWeights[pKF] != weight)
            mConnectedKeyFrameWeights[pKF] = weight;
        else
            return;
        UpdateBestCovisibles();
    }

    void EraseConnection(KeyFrame* pKF) {
        bool bUpdate = false;
        if (mConnectedKeyFrameWeights.count(pKF)) {
            mConnectedKeyFrameWeights.erase(pKF);
            bUpdate = true;
        }
        if (bUpdate) UpdateBestCovisibles();
    }

    void count(const std::vector<Feature*>& v, std::map<KeyFrame*, int>& KFcounter) {
        for (std::vector<Feature*>::const_iterator vit = v.begin(), vend = v.end(); vit != vend; vit++) {
            Feature* pMP = *vit;
            if (!pMP) continue;
            if (pMP->isBad()) continue;
            std::map<KeyFrame*, int> observations = pMP->GetObservations();
            for (std::map<KeyFrame*, int>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
                if (mit->first == this || mit->first->isBad() || mit->first->mpMap != mpMap) continue;
                if (!mit->first->named) continue;  // not a keyframe of the map walk
                KFcounter[mit->first]++;
            }
        }
    }

    // returns KFcounter.size(); *pmax / *wmax = pKFmax / nmax
    int UpdateConnections(bool withLines, KeyFrame** pmax, int* wmax) {
        std::map<KeyFrame*, int> KFcounter;
        count(mvpMapPoints, KFcounter);
        if (withLines) count(mvpMapLines, KFcounter);
        *pmax = nullptr;
        *wmax = 0;
        if (KFcounter.empty()) return 0;
        int nmax = 0;
        KeyFrame* pKFmax = nullptr;
        int th = 15;
        std::vector<std::pair<int, KeyFrame*> > vPairs;
        vPairs.reserve(KFcounter.size());
        for (std::map<KeyFrame*, int>::iterator mit = KFcounter.begin(), mend = KFcounter.end(); mit != mend; mit++) {
            if (mit->second > nmax) {
                nmax = mit->second;
                pKFmax = mit->first;
            }
            if (mit->second >= th) {
                vPairs.push_back(std::make_pair(mit->second, mit->first));
                (mit->first)->AddConnection(this, mit->second);
            }
        }
        if (vPairs.empty()) {
            vPairs.push_back(std::make_pair(nmax, pKFmax));
            pKFmax->AddConnection(this, nmax);
        }
        std::sort(vPairs.begin(), vPairs.end());
        std::list<KeyFrame*> lKFs;
        std::list<int> lWs;
        for (size_t i = 0; i < vPairs.size(); i++) {
            lKFs.push_front(vPairs[i].second);
            lWs.push_front(vPairs[i].first);
        }
        mConnectedKeyFrameWeights = KFcounter;
        mvpOrderedConnectedKeyFrames = std::vector<KeyFrame*>(lKFs.begin(), lKFs.end());
        mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
        touched = true;
        if (mbFirstConnection && !init) {
            mpParent = mvpOrderedConnectedKeyFrames.front();
            parentSet = true;  // mpParent->AddChild(this) is the caller's
            mbFirstConnection = false;
        }
        *pmax = pKFmax;
        *wmax = nmax;
        return (int)KFcounter.size();
    }

    static bool weightComp(int a, int b) { return a > b; }

    int GetCovisiblesByWeight(const int& w) {
        if (mvpOrderedConnectedKeyFrames.empty()) return 0;
        std::vector<int>::iterator it = std::upper_bound(mvOrderedWeights.begin(), mvOrderedWeights.end(), w, KeyFrame::weightComp);
        if (it == mvOrderedWeights.end() && mvOrderedWeights.back() < w) return 0;
        return (int)(it - mvOrderedWeights.begin());
    }

    int GetWeight(KeyFrame* pKF) {
        if (mConnectedKeyFrameWeights.count(pKF)) return mConnectedKeyFrameWeights[pKF];
        return 0;
    }
};

// the graph between calls, by slot
struct Graph {
    int K;
    std::vector<std::map<int, int> > weights;                // slot -> (slot -> weight)
    std::vector<std::vector<std::pair<int, int> > > ordered;  // slot -> (slot, weight) as stored
};

// the objects of one call
struct World {
    std::vector<KeyFrame> kfs;
    std::vector<int> at;  // slot -> index = address rank
    KeyFrame* kf(int s) { return s >= 0 && s < (int)at.size() ? &kfs[at[s]] : nullptr; }

    World(const Graph& g, const uint8_t* bad, const int* order, int n_order) : kfs(g.K), at(g.K, -1) {
        int next = 0;
        for (int i = 0; i < n_order; ++i)
            if (order[i] >= 0 && order[i] < g.K && at[order[i]] < 0) {
                at[order[i]] = next++;
                kfs[at[order[i]]].named = true;
            }
        for (int s = 0; s < g.K; ++s)
            if (at[s] < 0) at[s] = next++;
        for (int s = 0; s < g.K; ++s) {
            KeyFrame& k = *kf(s);
            k.slot = s;
            k.mbBad = bad[s] != 0;
            for (std::map<int, int>::const_iterator it = g.weights[s].begin(); it != g.weights[s].end(); ++it)
                k.mConnectedKeyFrameWeights[kf(it->first)] = it->second;
            for (size_t i = 0; i < g.ordered[s].size(); ++i) {
                k.mvpOrderedConnectedKeyFrames.push_back(kf(g.ordered[s][i].first));
                k.mvOrderedWeights.push_back(g.ordered[s][i].second);
            }
        }
    }

    void store(Graph& g, int* touched) {
        for (int s = 0; s < g.K; ++s) {
            KeyFrame& k = *kf(s);
            g.weights[s].clear();
            for (std::map<KeyFrame*, int>::iterator it = k.mConnectedKeyFrameWeights.begin(); it != k.mConnectedKeyFrameWeights.end(); ++it)
                g.weights[s][it->first->slot] = it->second;
            g.ordered[s].clear();
            for (size_t i = 0; i < k.mvpOrderedConnectedKeyFrames.size(); ++i)
                g.ordered[s].push_back(std::make_pair(k.mvpOrderedConnectedKeyFrames[i]->slot, k.mvOrderedWeights[i]));
            if (touched) touched[s] = k.touched ? 1 : 0;
        }
    }
};

void build_pool(std::vector<Feature>& pool, int n, const uint8_t* bad, const int* obs_off, const int* obs_kf, World& w) {
    pool.resize(n);
    for (int i = 0; i < n; ++i) {
        pool[i].bad = bad[i] != 0;
        for (int o = obs_off[i]; o < obs_off[i + 1]; ++o)
            if (w.kf(obs_kf[o])) pool[i].mObservations[w.kf(obs_kf[o])] = o;
    }
}

double g_seconds = 0;

}  // namespace

extern "C" void* covis_ref_create(int K) {
    Graph* g = new Graph;
    g->K = K;
    g->weights.resize(K);
    g->ordered.resize(K);
    return g;
}

extern "C" void covis_ref_destroy(void* h) { delete static_cast<Graph*>(h); }

// the time the last covis_ref_update spent in the UpdateConnections calls, the object graph already built
extern "C" double covis_ref_seconds() { return g_seconds; }

// The queries q[0 .. n_q) one after another.  first_conn / parent (may be NULL) are in/out;
// touched[s] = 1 where the ordered list of slot s was assigned during the call.
extern "C" void covis_ref_update(void* h, const uint8_t* kf_bad, const int* order, int n_order, const int* kf_mp,
                                 const int* kf_nmp, int kp_cap, const int* kf_ml, const int* kf_nml, int kl_cap,
                                 const int* map_id, const uint8_t* init_kf, uint8_t* first_conn, int* parent, int mp_n,
                                 const uint8_t* mp_bad, const int* mp_obs_off, const int* mp_obs_kf, int ml_n,
                                 const uint8_t* ml_bad, const int* ml_obs_off, const int* ml_obs_kf, int n_q, const int* q,
                                 int* n_counted, int* n_conn, int* kf_max, int* w_max, int* new_parent, int* touched) {
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
        const int np = kf_nmp[s] < 0 ? 0 : kf_nmp[s] > kp_cap ? kp_cap : kf_nmp[s];
        for (int i = 0; i < np; ++i) {
            const int id = kf_mp[(size_t)s * kp_cap + i];
            k.mvpMapPoints.push_back(id >= 0 && id < mp_n ? &mps[id] : nullptr);
        }
        if (with_lines) {
            const int nl = kf_nml[s] < 0 ? 0 : kf_nml[s] > kl_cap ? kl_cap : kf_nml[s];
            for (int i = 0; i < nl; ++i) {
                const int id = kf_ml[(size_t)s * kl_cap + i];
                k.mvpMapLines.push_back(id >= 0 && id < ml_n ? &mls[id] : nullptr);
            }
        }
    }
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n_q; ++i) {
        KeyFrame& k = *w.kf(q[i]);
        k.parentSet = false;
        KeyFrame* pmax = nullptr;
        int wmax = 0;
        n_counted[i] = k.UpdateConnections(with_lines, &pmax, &wmax);
        n_conn[i] = n_counted[i] ? (int)k.mvpOrderedConnectedKeyFrames.size() : 0;
        kf_max[i] = pmax ? pmax->slot : -1;
        w_max[i] = wmax;
        new_parent[i] = k.parentSet ? k.mpParent->slot : -1;
    }
    g_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int s = 0; s < g.K; ++s) {
        KeyFrame& k = *w.kf(s);
        if (first_conn) first_conn[s] = k.mbFirstConnection ? 1 : 0;
        if (parent) parent[s] = k.mpParent ? k.mpParent->slot : -1;
    }
    w.store(g, touched);
}

// the connection part of SetBadFlag for each slot in turn
extern "C" void covis_ref_erase(void* h, int n, const int* slots, const uint8_t* kf_bad, const int* order, int n_order,
                                int* touched) {
    Graph& g = *static_cast<Graph*>(h);
    World w(g, kf_bad, order, n_order);
    for (int i = 0; i < n; ++i) {
        KeyFrame* k = w.kf(slots[i]);
        for (std::map<KeyFrame*, int>::iterator mit = k->mConnectedKeyFrameWeights.begin(), mend = k->mConnectedKeyFrameWeights.end(); mit != mend; mit++)
            mit->first->EraseConnection(k);
        k->mConnectedKeyFrameWeights.clear();
        k->mvpOrderedConnectedKeyFrames.clear();
        k->mvOrderedWeights.clear();
        k->touched = true;
    }
    w.store(g, touched);
}

extern "C" void covis_ref_resort(void* h, int n, const int* slots, const uint8_t* kf_bad, const int* order, int n_order,
                                 int* touched) {
    Graph& g = *static_cast<Graph*>(h);
    World w(g, kf_bad, order, n_order);
    for (int i = 0; i < n; ++i) w.kf(slots[i])->UpdateBestCovisibles();
    w.store(g, touched);
}

// the map in ascending slot order and the ordered list as stored; the tables hold K entries
extern "C" void covis_ref_get(void* h, int slot, int* map_kf, int* map_w, int* n_map, int* ord_kf, int* ord_w, int* n_ord) {
    Graph& g = *static_cast<Graph*>(h);
    int i = 0;
    for (std::map<int, int>::const_iterator it = g.weights[slot].begin(); it != g.weights[slot].end(); ++it, ++i) {
        map_kf[i] = it->first;
        map_w[i] = it->second;
    }
    *n_map = i;
    *n_ord = (int)g.ordered[slot].size();
    for (size_t j = 0; j < g.ordered[slot].size(); ++j) {
        ord_kf[j] = g.ordered[slot][j].first;
        ord_w[j] = g.ordered[slot][j].second;
    }
}

extern "C" int covis_ref_by_weight(void* h, int slot, int w) {
    Graph& g = *static_cast<Graph*>(h);
    KeyFrame k;
    std::vector<KeyFrame> dummy(g.ordered[slot].size());
    for (size_t j = 0; j < g.ordered[slot].size(); ++j) {
        k.mvpOrderedConnectedKeyFrames.push_back(&dummy[j]);
        k.mvOrderedWeights.push_back(g.ordered[slot][j].second);
    }
    return k.GetCovisiblesByWeight(w);
}

extern "C" int covis_ref_weight(void* h, int a, int b) {
    Graph& g = *static_cast<Graph*>(h);
    std::vector<KeyFrame> kfs(g.K);
    KeyFrame& k = kfs[a];
    for (std::map<int, int>::const_iterator it = g.weights[a].begin(); it != g.weights[a].end(); ++it)
        k.mConnectedKeyFrameWeights[&kfs[it->first]] = it->second;
    return b >= 0 && b < g.K ? k.GetWeight(&kfs[b]) : 0;
}
