// match_tile_check -- the matrix-core kNN-2's arithmetic (csrc/match_tile.h) on
// the host: a replay of the kernel's tile walk against a brute-force scan with
// BFMatcher's rule (train rows ascending, strict-< insertion into two slots).
//
// The replay keeps the kernel's shape: 16 x 16 tiles with the trains as rows
// and the queries as columns; "lane" (c, g) expands bytes [8g, 8g + 8) of
// train row c and of query c with expand_train_word / expand_query_word, the
// int8 product of v_mfma_i32_16x16x64_i8 is summed over the four lane groups
// and the four K blocks, lane (c, g) gets trains 4g .. 4g + 3 of the tile,
// keys are made, masked in the tail tile and inserted with top2_update, the
// four groups merge with top2_merge and decode_key gives (index, distance).
// Tables: random, near-duplicates, duplicate-heavy, all-equal, complement.
// usage: match_tile_check nq:nt ...
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "match_tile.h"

namespace {

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

using Table = std::vector<uint32_t>;  // 8 words per row

void brute(const Table& q, int nq, const Table& t, int nt, std::vector<int>& out) {
    out.assign((size_t)nq * 4, 0);
    for (int i = 0; i < nq; ++i) {
        int b0 = 0x7fffffff, b1 = 0x7fffffff, j0 = -1, j1 = -1;
        for (int j = 0; j < nt; ++j) {
            int d = 0;
            for (int k = 0; k < 8; ++k) d += __builtin_popcount(q[(size_t)i * 8 + k] ^ t[(size_t)j * 8 + k]);
            if (d < b1) {
                if (d < b0) { b1 = b0; j1 = j0; b0 = d; j0 = j; }
                else { b1 = d; j1 = j; }
            }
        }
        int* o = &out[(size_t)i * 4];
        o[0] = j0; o[1] = b0; o[2] = j1; o[3] = b1;
    }
}

// expanded bytes of one lane: 16 registers of four int8
struct Lane { uint32_t e[16]; };

int dot_lane(const Lane& a, const Lane& b) {
    int s = 0;
    for (int k = 0; k < 16; ++k)
        for (int by = 0; by < 4; ++by)
            s += (int)(int8_t)(a.e[k] >> (8 * by)) * (int)(int8_t)(b.e[k] >> (8 * by));
    return s;
}

void tiled(const Table& q, int nq, const Table& t, int nt, std::vector<int>& out) {
    out.assign((size_t)nq * 4, 0);
    for (int qb = 0; qb < nq; qb += 16) {  // one query tile
        Lane ql[16][4];
        int popq[16];
        for (int c = 0; c < 16; ++c) {
            popq[c] = 0;
            for (int g = 0; g < 4; ++g) {
                uint32_t w0 = 0, w1 = 0;
                if (qb + c < nq) { w0 = q[(size_t)(qb + c) * 8 + 2 * g]; w1 = q[(size_t)(qb + c) * 8 + 2 * g + 1]; }
                plvi::expand_query_word(w0, ql[c][g].e);
                plvi::expand_query_word(w1, ql[c][g].e + 8);
                popq[c] += plvi::popc32(w0) + plvi::popc32(w1);
            }
        }
        int b0[16][4], b1[16][4];
        for (int c = 0; c < 16; ++c)
            for (int g = 0; g < 4; ++g) b0[c][g] = b1[c][g] = plvi::kKeySentinel;
        for (int tb = 0; tb < nt; tb += 16) {
            const bool mask = tb + 16 > nt;
            Lane tl[16][4];
            for (int r = 0; r < 16; ++r)
                for (int g = 0; g < 4; ++g) {
                    uint32_t w0 = 0, w1 = 0;  // rows past the count: zeros, not loaded
                    if (tb + r < nt) { w0 = t[(size_t)(tb + r) * 8 + 2 * g]; w1 = t[(size_t)(tb + r) * 8 + 2 * g + 1]; }
                    plvi::expand_train_word(w0, tl[r][g].e);
                    plvi::expand_train_word(w1, tl[r][g].e + 8);
                }
            for (int c = 0; c < 16; ++c)
                for (int g = 0; g < 4; ++g)
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * g + r, j = tb + row;
                        int acc = 0;
                        for (int gg = 0; gg < 4; ++gg) acc += dot_lane(tl[row][gg], ql[c][gg]);
                        int k = plvi::make_key(acc, j);
                        if (mask) k = j < nt ? k : plvi::kKeySentinel;
                        plvi::top2_update(b0[c][g], b1[c][g], k);
                    }
        }
        for (int c = 0; c < 16 && qb + c < nq; ++c) {
            // the butterfly of the kernel: groups g ^ 1 (lanes ^ 16), then g ^ 2 (lanes ^ 32)
            int m0[4], m1[4];
            for (int g = 0; g < 4; ++g) { m0[g] = b0[c][g]; m1[g] = b1[c][g]; }
            for (int x = 1; x <= 2; x <<= 1) {
                int n0[4], n1[4];
                for (int g = 0; g < 4; ++g) {
                    n0[g] = m0[g]; n1[g] = m1[g];
                    plvi::top2_merge(n0[g], n1[g], m0[g ^ x], m1[g ^ x]);
                }
                memcpy(m0, n0, sizeof m0);
                memcpy(m1, n1, sizeof m1);
            }
            int* o = &out[(size_t)(qb + c) * 4];
            plvi::decode_key(m0[0], popq[c], o[0], o[1]);
            plvi::decode_key(m1[0], popq[c], o[2], o[3]);
            for (int g = 1; g < 4; ++g)
                if (m0[g] != m0[0] || m1[g] != m1[0]) o[0] = -2;  // the groups must agree after the merge
        }
    }
}

void fill(Table& q, int nq, Table& t, int nt, int kind) {
    q.assign((size_t)nq * 8, 0);
    t.assign((size_t)nt * 8, 0);
    for (auto& w : t) w = rnd();
    for (auto& w : q) w = rnd();
    if (kind == 1 && nt) {  // near-duplicates: a query is a train row with a few bits flipped
        for (int i = 0; i < nq; ++i) {
            const int j = rnd() % nt;
            for (int k = 0; k < 8; ++k) q[(size_t)i * 8 + k] = t[(size_t)j * 8 + k] ^ (1u << (rnd() & 31)) * (rnd() & 1);
        }
    } else if (kind == 2 && nt) {  // duplicate-heavy: four distinct train rows, queries drawn from them
        for (int j = 4; j < nt; ++j) memcpy(&t[(size_t)j * 8], &t[(size_t)(rnd() & 3) * 8], 32);
        for (int i = 0; i < nq; ++i) memcpy(&q[(size_t)i * 8], &t[(size_t)(rnd() % nt) * 8], 32);
    } else if (kind == 3 && nt) {  // all-equal trains; queries: the row, its complement, one bit off
        for (int j = 1; j < nt; ++j) memcpy(&t[(size_t)j * 8], &t[0], 32);
        for (int i = 0; i < nq; ++i)
            for (int k = 0; k < 8; ++k)
                q[(size_t)i * 8 + k] = i % 3 == 0 ? t[k] : i % 3 == 1 ? ~t[k] : t[k] ^ (k == 0);
    } else if (kind == 4) {  // all-zero and all-one rows: dot products at both ends
        for (int j = 0; j < nt; ++j)
            for (int k = 0; k < 8; ++k) t[(size_t)j * 8 + k] = (j & 1) ? ~0u : 0u;
        for (int i = 0; i < nq; ++i)
            for (int k = 0; k < 8; ++k) q[(size_t)i * 8 + k] = (i & 2) ? ~0u : 0u;
    }
}

}  // namespace

int main(int argc, char** argv) {
    long checked = 0, mismatches = 0;
    // the expansion itself: every bit of a word lands in one byte of one register, as documented
    for (int bit = 0; bit < 32; ++bit) {
        uint32_t a[8], b1[8], b0[8];
        plvi::expand_train_word(1u << bit, a);
        plvi::expand_query_word(1u << bit, b1);
        plvi::expand_query_word(0, b0);
        const int j = bit & 7, by = bit >> 3;
        for (int k = 0; k < 8; ++k)
            for (int y = 0; y < 4; ++y) {
                const int av = (int8_t)(a[k] >> (8 * y)), q1 = (int8_t)(b1[k] >> (8 * y)), q0 = (int8_t)(b0[k] >> (8 * y));
                const bool here = k == j && y == by;
                if (av * q0 != (here ? 64 : 0) || av * q1 != (here ? -64 : 0) || (q0 != q1) != here) {
                    ++mismatches;
                    std::printf("expansion: bit %d register %d byte %d\n", bit, k, y);
                }
                ++checked;
            }
    }
    Table q, t;
    std::vector<int> want, got;
    for (int i = 1; i < argc; ++i) {
        int nq = 0, nt = 0;
        if (std::sscanf(argv[i], "%d:%d", &nq, &nt) != 2 || nq < 0 || nt < 0 || nt > plvi::kKeyMaxTrain) return 2;
        for (int kind = 0; kind < 5; ++kind) {
            fill(q, nq, t, nt, kind);
            brute(q, nq, t, nt, want);
            tiled(q, nq, t, nt, got);
            for (int r = 0; r < nq; ++r) {
                if (memcmp(&want[(size_t)r * 4], &got[(size_t)r * 4], 16)) {
                    ++mismatches;
                    if (mismatches < 20)
                        std::printf("%s kind %d query %d: want (%d,%d,%d,%d) got (%d,%d,%d,%d)\n", argv[i], kind, r,
                                    want[r * 4], want[r * 4 + 1], want[r * 4 + 2], want[r * 4 + 3], got[r * 4],
                                    got[r * 4 + 1], got[r * 4 + 2], got[r * 4 + 3]);
                }
                ++checked;
            }
        }
    }
    std::printf("checked=%ld mismatches=%ld\n", checked, mismatches);
    return mismatches ? 1 : 0;
}
