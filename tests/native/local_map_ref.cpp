// local_map_ref.cpp — a sequential host restatement of Tracking::UpdateLocalKeyFrames[WithLines]
// (src/Tracking.cc:5399-5551 / :5553-5745), UpdateLocalPoints[AndLines] (:5325-5352 / :5354-5397)
// and the first loop of SearchLocalPoints[AndLines] (:5052-5069 / :5126-5161) in the reference's own
// shape: objects and pointers, a std::map<KF*, int> counter iterated by address, std::set<KF*>
// children, a std::vector with reserve(3 * size) walked by an end iterator taken before the loop,
// and the two stamps mnTrackReferenceForFrame / mnLastFrameSeen.  The expected values of
// tests/test_local_map.py; compiled at test time.
//
// Addresses: the keyframe objects live in one array, placed so that ascending address is the
// caller's `order` (slots it does not name follow, by slot).  A child list is therefore re-sorted
// here, by the std::set, into that same order -- the caller of the library must hand the children
// over already sorted this way.  The frame id is 1, so the constructors' stamp 0 never equals it.
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

namespace {

struct KF;

struct Feature {  // MapPoint or MapLine
    int id = -1;
    bool bad = false;
    std::map<KF*, int> mObservations;
    long mnTrackReferenceForFrame = 0, mnLastFrameSeen = 0;
    bool isBad() const { return bad; }
};

struct KF {
    int slot = -1;
    bool bad = true;
    std::vector<KF*> covis;  // GetBestCovisibilityKeyFrames(10)
    std::set<KF*> childs;
    KF* parent = nullptr;
    KF* mPrevKF = nullptr;
    std::vector<Feature*> mps, mls;
    long mnTrackReferenceForFrame = 0;
    bool isBad() const { return bad; }
};

void vote(std::vector<Feature>& pool, int* table, int n, std::map<KF*, int>& keyframeCounter) {
    for (int i = 0; i < n; i++) {
        if (table[i] < 0 || table[i] >= (int)pool.size()) continue;  // NULL
        Feature* p = &pool[table[i]];
        if (!p->isBad()) {
            const std::map<KF*, int> observations = p->mObservations;
            for (std::map<KF*, int>::const_iterator it = observations.begin(), itend = observations.end(); it != itend; it++)
                keyframeCounter[it->first]++;
        } else {
            table[i] = -1;
        }
    }
}

void collect(const std::vector<Feature*>& v, long id, std::vector<Feature*>& local) {
    for (std::vector<Feature*>::const_iterator it = v.begin(), end = v.end(); it != end; it++) {
        Feature* p = *it;
        if (!p) continue;
        if (p->mnTrackReferenceForFrame == id) continue;
        if (!p->isBad()) {
            local.push_back(p);
            p->mnTrackReferenceForFrame = id;
        }
    }
}

void build_pool(std::vector<Feature>& pool, int n, const uint8_t* bad, const int* obs_off, const int* obs_kf,
                std::vector<KF>& kfs, const std::vector<int>& at, int kf_cap) {
    pool.resize(n);
    for (int i = 0; i < n; ++i) {
        pool[i].id = i;
        pool[i].bad = bad[i] != 0;
        for (int o = obs_off[i]; o < obs_off[i + 1]; ++o)
            if (obs_kf[o] >= 0 && obs_kf[o] < kf_cap) pool[i].mObservations[&kfs[at[obs_kf[o]]]] = o;
    }
}

double g_seconds = 0;

}  // namespace

// the time the last call spent in the two Update functions, the object graph already built
// (tools/local_map_bench.py prints it for context)
extern "C" double local_map_ref_seconds() { return g_seconds; }

extern "C" int local_map_ref(int kf_cap, const uint8_t* kf_bad, const int* order, int n_order, const int* covis,
                             const int* child_off, const int* child, const int* parent, const int* prev_kf,
                             const int* kf_mp, const int* kf_nmp, int kp_cap, const int* kf_ml, const int* kf_nml,
                             int kl_cap, int mp_n, const uint8_t* mp_bad, const int* mp_obs_off, const int* mp_obs_kf,
                             int ml_n, const uint8_t* ml_bad, const int* ml_obs_off, const int* ml_obs_kf, int* vote_mp,
                             int n_vote_mp, int* vote_ml, int n_vote_ml, const int* seen_mp, int n_seen_mp,
                             const int* seen_ml, int n_seen_ml, int last_kf, int* local_kf, int* n_local_kf, int* ref_kf,
                             int* local_mp, int* n_local_mp, uint8_t* mp_flags, int* local_ml, int* n_local_ml,
                             uint8_t* ml_flags) {
    const bool with_lines = kf_ml != nullptr;
    const long mnId = 1;  // mCurrentFrame.mnId
    // slot -> index in the array, i.e. its address rank
    std::vector<int> at(kf_cap, -1);
    int next = 0;
    for (int i = 0; i < n_order; ++i)
        if (order[i] >= 0 && order[i] < kf_cap && at[order[i]] < 0) at[order[i]] = next++;
    for (int s = 0; s < kf_cap; ++s)
        if (at[s] < 0) at[s] = next++;
    std::vector<KF> kfs(kf_cap);
    std::vector<Feature> mps, mls;
    build_pool(mps, mp_n, mp_bad, mp_obs_off, mp_obs_kf, kfs, at, kf_cap);
    if (with_lines) build_pool(mls, ml_n, ml_bad, ml_obs_off, ml_obs_kf, kfs, at, kf_cap);
    auto kfp = [&](int s) -> KF* { return s >= 0 && s < kf_cap ? &kfs[at[s]] : nullptr; };
    for (int s = 0; s < kf_cap; ++s) {
        KF& k = *kfp(s);
        k.slot = s;
        k.bad = kf_bad[s] != 0;
        if (covis)
            for (int c = 0; c < 10 && covis[s * 10 + c] >= 0; ++c)
                if (covis[s * 10 + c] < kf_cap) k.covis.push_back(kfp(covis[s * 10 + c]));
        if (child_off)
            for (int c = child_off[s]; c < child_off[s + 1]; ++c)
                if (kfp(child[c])) k.childs.insert(kfp(child[c]));
        k.parent = parent ? kfp(parent[s]) : nullptr;
        k.mPrevKF = prev_kf ? kfp(prev_kf[s]) : nullptr;
        const int np = kf_nmp[s] < 0 ? 0 : kf_nmp[s] > kp_cap ? kp_cap : kf_nmp[s];
        for (int i = 0; i < np; ++i) {
            const int id = kf_mp[(size_t)s * kp_cap + i];
            k.mps.push_back(id >= 0 && id < mp_n ? &mps[id] : nullptr);
        }
        if (with_lines) {
            const int nl = kf_nml[s] < 0 ? 0 : kf_nml[s] > kl_cap ? kl_cap : kf_nml[s];
            for (int i = 0; i < nl; ++i) {
                const int id = kf_ml[(size_t)s * kl_cap + i];
                k.mls.push_back(id >= 0 && id < ml_n ? &mls[id] : nullptr);
            }
        }
    }

    // ---- UpdateLocalKeyFrames[WithLines]
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::map<KF*, int> keyframeCounter;
    if (vote_mp) vote(mps, vote_mp, n_vote_mp, keyframeCounter);
    if (with_lines && vote_ml) vote(mls, vote_ml, n_vote_ml, keyframeCounter);

    int max = 0;
    KF* pKFmax = nullptr;
    std::vector<KF*> mvpLocalKeyFrames;
    mvpLocalKeyFrames.reserve(3 * keyframeCounter.size());
    const size_t reserved = mvpLocalKeyFrames.capacity();
    for (std::map<KF*, int>::const_iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {
        KF* pKF = it->first;
        if (pKF->isBad()) continue;
        if (it->second > max) {
            max = it->second;
            pKFmax = pKF;
        }
        mvpLocalKeyFrames.push_back(pKF);
        pKF->mnTrackReferenceForFrame = mnId;
    }
    int reallocated = 0;
    for (std::vector<KF*>::const_iterator itKF = mvpLocalKeyFrames.begin(), itEndKF = mvpLocalKeyFrames.end(); itKF != itEndKF; itKF++) {
        if (mvpLocalKeyFrames.size() > 80) break;
        KF* pKF = *itKF;
        const std::vector<KF*> vNeighs = pKF->covis;
        for (std::vector<KF*>::const_iterator itN = vNeighs.begin(), itEndN = vNeighs.end(); itN != itEndN; itN++) {
            KF* pNeighKF = *itN;
            if (!pNeighKF->isBad()) {
                if (pNeighKF->mnTrackReferenceForFrame != mnId) {
                    mvpLocalKeyFrames.push_back(pNeighKF);
                    pNeighKF->mnTrackReferenceForFrame = mnId;
                    break;
                }
            }
        }
        const std::set<KF*> spChilds = pKF->childs;
        for (std::set<KF*>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) {
            KF* pChildKF = *sit;
            if (!pChildKF->isBad()) {
                if (pChildKF->mnTrackReferenceForFrame != mnId) {
                    mvpLocalKeyFrames.push_back(pChildKF);
                    pChildKF->mnTrackReferenceForFrame = mnId;
                    break;
                }
            }
        }
        KF* pParent = pKF->parent;
        if (pParent) {
            if (pParent->mnTrackReferenceForFrame != mnId) {
                mvpLocalKeyFrames.push_back(pParent);
                pParent->mnTrackReferenceForFrame = mnId;
                break;
            }
        }
        // the iterators stay valid only while the reserve holds (3 per K1 member at most)
        if (mvpLocalKeyFrames.capacity() != reserved) reallocated = 1;
    }
    if (last_kf >= 0 && prev_kf && mvpLocalKeyFrames.size() < 80) {
        KF* tempKeyFrame = kfp(last_kf);
        const int Nd = 20;
        for (int i = 0; i < Nd; i++) {
            if (!tempKeyFrame) break;
            if (tempKeyFrame->mnTrackReferenceForFrame != mnId) {
                mvpLocalKeyFrames.push_back(tempKeyFrame);
                tempKeyFrame->mnTrackReferenceForFrame = mnId;
                tempKeyFrame = tempKeyFrame->mPrevKF;
            }
        }
    }
    *ref_kf = pKFmax ? pKFmax->slot : -1;
    *n_local_kf = (int)mvpLocalKeyFrames.size();
    for (size_t i = 0; i < mvpLocalKeyFrames.size(); ++i) local_kf[i] = mvpLocalKeyFrames[i]->slot;

    // ---- UpdateLocalPoints[AndLines]
    std::vector<Feature*> mvpLocalMapPoints, mvpLocalMapLines;
    for (std::vector<KF*>::const_reverse_iterator itKF = mvpLocalKeyFrames.rbegin(), itEndKF = mvpLocalKeyFrames.rend(); itKF != itEndKF; ++itKF) {
        KF* pKF = *itKF;
        collect(pKF->mps, mnId, mvpLocalMapPoints);
        if (with_lines) collect(pKF->mls, mnId, mvpLocalMapLines);
    }
    g_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    // ---- the first loop of SearchLocalPoints[AndLines], then the test of the second
    const int* sp = seen_mp ? seen_mp : vote_mp;
    const int nsp = seen_mp ? n_seen_mp : n_vote_mp;
    for (int i = 0; sp && i < nsp; ++i)
        if (sp[i] >= 0 && sp[i] < mp_n && !mps[sp[i]].isBad()) mps[sp[i]].mnLastFrameSeen = mnId;
    const int* sl = seen_ml ? seen_ml : vote_ml;
    const int nsl = seen_ml ? n_seen_ml : n_vote_ml;
    for (int i = 0; with_lines && sl && i < nsl; ++i)
        if (sl[i] >= 0 && sl[i] < ml_n && !mls[sl[i]].isBad()) mls[sl[i]].mnLastFrameSeen = mnId;
    *n_local_mp = (int)mvpLocalMapPoints.size();
    for (size_t i = 0; i < mvpLocalMapPoints.size(); ++i) {
        const Feature* p = mvpLocalMapPoints[i];
        local_mp[i] = p->id;
        mp_flags[i] = (uint8_t)((p->mnLastFrameSeen != mnId ? 1 : 0) | (p->mObservations.size() > 0 ? 2 : 0));
    }
    *n_local_ml = (int)mvpLocalMapLines.size();
    for (size_t i = 0; i < mvpLocalMapLines.size(); ++i) {
        const Feature* p = mvpLocalMapLines[i];
        local_ml[i] = p->id;
        ml_flags[i] = (uint8_t)((p->mnLastFrameSeen != mnId ? 1 : 0) | (p->mObservations.size() > 0 ? 2 : 0));
    }
    return reallocated;
}
