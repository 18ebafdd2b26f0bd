// kfdb_ref.cpp — a sequential host restatement of KeyFrameDatabase (src/KeyFrameDatabase.cc) in the
// reference's own shape: a std::vector<std::list<KF*>> inverted file, per-keyframe stamp / words /
// score members that persist between calls, std::map BowVectors, L1Scoring::score as written
// (ScoringObject.cpp:23-68) and std::list::sort(compFirst).  The expected values of
// tests/test_kfdb.py; compiled at test time with -ffp-contract=off.
//
// What the restatement models and the reference leaves open: mRelocScore and
// mPlaceRecognitionScore start at 0 (the reference never initialises them), every query gets a
// fresh id >= 1 (so the stamp 0 of a new keyframe never equals it), and a slot that is erased and
// added again is a new keyframe.
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

typedef std::map<unsigned, double> BowVector;

struct KF {
    int slot = -1, map = 0;
    bool in_db = false;
    BowVector mBowVec;
    long mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
    int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
    float mRelocScore = 0, mPlaceRecognitionScore = 0;
};

struct DB {
    std::vector<std::list<KF*> > mvInvertedFile;
    std::vector<KF> kfs;
    long next_id = 1;
};

double score(const BowVector& v1, const BowVector& v2) {
    BowVector::const_iterator v1_it = v1.begin(), v2_it = v2.begin();
    const BowVector::const_iterator v1_end = v1.end(), v2_end = v2.end();
    double score = 0;
    while (v1_it != v1_end && v2_it != v2_end) {
        const double& vi = v1_it->second;
        const double& wi = v2_it->second;
        if (v1_it->first == v2_it->first) {
            score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++v1_it;
            ++v2_it;
        } else if (v1_it->first < v2_it->first) {
            v1_it = v1.lower_bound(v2_it->first);
        } else {
            v2_it = v2.lower_bound(v1_it->first);
        }
    }
    score = -score / 2.0;
    return score;
}

bool compFirst(const std::pair<float, KF*>& a, const std::pair<float, KF*>& b) { return a.first > b.first; }

}  // namespace

extern "C" {

void* kfdb_ref_create(int n_words, int slot_cap) {
    DB* db = new DB;
    db->mvInvertedFile.resize(n_words);
    db->kfs.resize(slot_cap);
    return db;
}

void kfdb_ref_destroy(void* p) { delete static_cast<DB*>(p); }

int kfdb_ref_add(void* p, int slot, int map, const unsigned* word, const double* value, int n) {
    DB* db = static_cast<DB*>(p);
    if (slot < 0 || slot >= (int)db->kfs.size() || db->kfs[slot].in_db) return -2;
    KF fresh;
    fresh.slot = slot;
    fresh.map = map;
    fresh.in_db = true;
    for (int i = 0; i < n; ++i) fresh.mBowVec[word[i]] = value[i];
    db->kfs[slot] = fresh;
    KF* pKF = &db->kfs[slot];
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++)
        db->mvInvertedFile[vit->first].push_back(pKF);
    return 0;
}

void kfdb_ref_erase(void* p, int slot) {
    DB* db = static_cast<DB*>(p);
    KF* pKF = &db->kfs[slot];
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) {
        std::list<KF*>& lKFs = db->mvInvertedFile[vit->first];
        for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++)
            if (pKF == *lit) {
                lKFs.erase(lit);
                break;
            }
    }
    pKF->in_db = false;
}

void kfdb_ref_clear_map(void* p, int map) {
    DB* db = static_cast<DB*>(p);
    for (std::vector<std::list<KF*> >::iterator vit = db->mvInvertedFile.begin(); vit != db->mvInvertedFile.end(); vit++) {
        std::list<KF*>& lKFs = *vit;
        for (std::list<KF*>::iterator lit = lKFs.begin(); lit != lKFs.end();) {
            if (map == (*lit)->map) lit = lKFs.erase(lit);
            else ++lit;
        }
    }
    for (size_t s = 0; s < db->kfs.size(); ++s)
        if (db->kfs[s].map == map) db->kfs[s].in_db = false;
}

void kfdb_ref_clear(void* p) {
    DB* db = static_cast<DB*>(p);
    const size_t n = db->mvInvertedFile.size();
    db->mvInvertedFile.clear();
    db->mvInvertedFile.resize(n);
    for (size_t s = 0; s < db->kfs.size(); ++s) db->kfs[s].in_db = false;
}

// One query.  words / sc [slot_cap] (cells of keyframes outside the list / not scored are left
// alone, words is pre-set to -1 here), order [slot_cap] + *norder, out_a / *n_a = the candidates
// (mode 0, all of them) or vpLoopCand (mode 1), out_b / *n_b = vpMergeCand.  Diagnostics per entry
// of lAccScoreAndMatch in list order: ent_slot, ent_acc, ent_best [slot_cap] + *n_ent; diag[0] =
// entries dropped as duplicates, diag[1] = accumulation steps that added a non-zero member of a
// neighbour this query did not score.
void kfdb_ref_query(void* p, const unsigned* q_word, const double* q_value, int q_n, int q_map, int mode, int n_best,
                    const int* conn, int n_conn, const int* covis, const uint8_t* map_bad, int n_maps, int* words,
                    double* sc, int* order, int* norder, int* out_a, int* n_a, int* out_b, int* n_b, int* ent_slot,
                    float* ent_acc, int* ent_best, int* n_ent, int* diag) {
    DB* db = static_cast<DB*>(p);
    const int S = (int)db->kfs.size();
    BowVector qBow;
    for (int i = 0; i < q_n; ++i) qBow[q_word[i]] = q_value[i];
    const long id = db->next_id++;
    for (int s = 0; s < S; ++s) words[s] = -1;
    *norder = *n_a = *n_b = *n_ent = 0;
    diag[0] = diag[1] = 0;
    std::set<KF*> spConnectedKF;
    if (mode == 1)
        for (int i = 0; i < n_conn; ++i)
            if (conn[i] >= 0 && conn[i] < S) spConnectedKF.insert(&db->kfs[conn[i]]);

    std::list<KF*> lKFsSharingWords;
    for (BowVector::const_iterator vit = qBow.begin(), vend = qBow.end(); vit != vend; vit++) {
        std::list<KF*>& lKFs = db->mvInvertedFile[vit->first];
        for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
            KF* pKFi = *lit;
            if (mode == 1) {
                if (pKFi->mnPlaceRecognitionQuery != id) {
                    pKFi->mnPlaceRecognitionWords = 0;
                    if (!spConnectedKF.count(pKFi)) {
                        pKFi->mnPlaceRecognitionQuery = id;
                        lKFsSharingWords.push_back(pKFi);
                    }
                }
                pKFi->mnPlaceRecognitionWords++;
            } else {
                if (pKFi->mnRelocQuery != id) {
                    pKFi->mnRelocWords = 0;
                    pKFi->mnRelocQuery = id;
                    lKFsSharingWords.push_back(pKFi);
                }
                pKFi->mnRelocWords++;
            }
        }
    }
    if (lKFsSharingWords.empty()) return;
#define WORDS(k) (mode == 1 ? (k)->mnPlaceRecognitionWords : (k)->mnRelocWords)
#define STAMP(k) (mode == 1 ? (k)->mnPlaceRecognitionQuery : (k)->mnRelocQuery)
#define MEMBER(k) (mode == 1 ? (k)->mPlaceRecognitionScore : (k)->mRelocScore)
    int maxCommonWords = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
        order[(*norder)++] = (*lit)->slot;
        words[(*lit)->slot] = WORDS(*lit);
        if (WORDS(*lit) > maxCommonWords) maxCommonWords = WORDS(*lit);
    }
    int minCommonWords = maxCommonWords * 0.8f;

    std::list<std::pair<float, KF*> > lScoreAndMatch;
    std::set<KF*> scored;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++) {
        KF* pKFi = *lit;
        if (WORDS(pKFi) > minCommonWords) {
            const double d = score(qBow, pKFi->mBowVec);
            sc[pKFi->slot] = d;
            float si = d;
            if (mode == 1) pKFi->mPlaceRecognitionScore = si;
            else pKFi->mRelocScore = si;
            lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            scored.insert(pKFi);
        }
    }
    if (lScoreAndMatch.empty()) return;

    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = 0;
    for (std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); it++) {
        KF* pKFi = it->second;
        // GetBestCovisibilityKeyFrames(10): the caller's table; an entry naming a keyframe that is
        // not in the database cannot carry this query's stamp
        std::vector<KF*> vpNeighs;
        if (covis)
            for (int k = 0; k < 10 && covis[pKFi->slot * 10 + k] >= 0; ++k)
                if (covis[pKFi->slot * 10 + k] < S && db->kfs[covis[pKFi->slot * 10 + k]].in_db)
                    vpNeighs.push_back(&db->kfs[covis[pKFi->slot * 10 + k]]);
        float bestScore = it->first;
        float accScore = bestScore;
        KF* pBestKF = pKFi;
        for (std::vector<KF*>::iterator vit = vpNeighs.begin(); vit != vpNeighs.end(); vit++) {
            KF* pKF2 = *vit;
            if (STAMP(pKF2) != id) continue;
            if (!scored.count(pKF2) && MEMBER(pKF2) != 0) diag[1]++;
            accScore += MEMBER(pKF2);
            if (MEMBER(pKF2) > bestScore) {
                pBestKF = pKF2;
                bestScore = MEMBER(pKF2);
            }
        }
        lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
        ent_slot[*n_ent] = pKFi->slot;
        ent_acc[*n_ent] = accScore;
        ent_best[(*n_ent)++] = pBestKF->slot;
        if (accScore > bestAccScore) bestAccScore = accScore;
    }

    std::set<KF*> spAlreadyAddedKF;
    if (mode == 0) {
        float minScoreToRetain = 0.75f * bestAccScore;
        for (std::list<std::pair<float, KF*> >::iterator it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end();
             it++) {
            const float& si = it->first;
            if (si > minScoreToRetain) {
                KF* pKFi = it->second;
                if (pKFi->map != q_map) continue;
                if (!spAlreadyAddedKF.count(pKFi)) {
                    out_a[(*n_a)++] = pKFi->slot;
                    spAlreadyAddedKF.insert(pKFi);
                } else {
                    diag[0]++;
                }
            }
        }
        return;
    }
    lAccScoreAndMatch.sort(compFirst);
    size_t i = 0;
    std::list<std::pair<float, KF*> >::iterator it = lAccScoreAndMatch.begin();
    while (i < lAccScoreAndMatch.size() && (*n_a < n_best || *n_b < n_best)) {
        KF* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
            const bool bad = map_bad && pKFi->map >= 0 && pKFi->map < n_maps && map_bad[pKFi->map];
            if (q_map == pKFi->map && *n_a < n_best) out_a[(*n_a)++] = pKFi->slot;
            else if (q_map != pKFi->map && *n_b < n_best && !bad) out_b[(*n_b)++] = pKFi->slot;
            spAlreadyAddedKF.insert(pKFi);
        } else {
            diag[0]++;
        }
        i++;
        it++;
    }
}

}  // extern "C"
