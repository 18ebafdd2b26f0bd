// match_tile.h — the arithmetic of the matrix-core Hamming kNN-2 (match.hip),
// as plain C++ for host and device; tests/native/match_tile_check.cpp replays
// a tile walk with it on the CPU against a brute-force scan.
//
// Distance as an int8 dot product.  For a train row t and a query row q
// (256 bits each), with the train bit kept as {0, 1} and the query bit b
// turned into 1 - 2b:
//     sum_k t_k (1 - 2 q_k) = popc(t) - 2 popc(t & q)
//     ham(q, t) = popc(q) + popc(t) - 2 popc(t & q) = popc(q) + that sum.
// popc(q) is a constant of the lane that owns the query, so it is left out of
// the running keys and added once at the end.
//
// Expansion.  Only the pairing of K slots between the two operands matters,
// so a 32-bit word goes to eight registers by bit position j inside its four
// bytes: register j holds bits {j, j + 8, j + 16, j + 24}, one per byte.
//   train:  w & (0x01010101 << j)            byte = bit * 2^j      (j < 7)
//           (w >> 7) & 0x01010101            byte = bit            (j = 7)
//   query:  byte = (1 - 2 bit) * 2^(6 - j)   (j < 7),  (1 - 2 bit) * 64 (j = 7)
// Every product is then bit_t * (1 - 2 bit_q) * 64: the accumulator is
// 64 * (ham - popc(q)), exact in int32 (|acc| <= 16384).  The train side costs
// nine VALU instructions per word; the query side is done once per sweep.
//
// Key.  key = (acc << 10) | j = ((ham - popc(q)) << 16) | j as a signed int:
// ordered by distance, then by train index, which is BFMatcher's strict-<
// insertion over ascending train rows.  Holds for train counts <= 65535.
#pragma once
#include <stdint.h>

#ifndef PLVI_HD
#ifdef __HIPCC__
#define PLVI_HD __host__ __device__ __forceinline__
#else
#define PLVI_HD static inline
#endif
#endif

namespace plvi {

constexpr int kKeySentinel = 0x7fffffff;  // no neighbour; also masks train rows at or past the count
constexpr int kKeyMaxTrain = 65535;       // the index field of a key

// train word -> eight operand registers ({0, 2^j} bytes)
PLVI_HD void expand_train_word(uint32_t w, uint32_t out[8]) {
#pragma unroll
    for (int j = 0; j < 7; ++j) out[j] = w & (0x01010101u << j);
    out[7] = (w >> 7) & 0x01010101u;
}

// query word -> eight operand registers (+-2^(6-j) bytes, two's complement per byte)
PLVI_HD void expand_query_word(uint32_t w, uint32_t out[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t mag = j < 7 ? (64u >> j) : 64u;
        // bit ? 256 - mag : mag, per byte; neither term carries into the next byte
        out[j] = mag * 0x01010101u + ((w >> j) & 0x01010101u) * (256u - 2u * mag);
    }
}

PLVI_HD int popc32(uint32_t w) { return __builtin_popcount(w); }

// acc = 64 * (ham - popc(q)); j = train row
PLVI_HD int make_key(int acc, int j) { return (int)(((uint32_t)acc << 10) | (uint32_t)j); }

PLVI_HD int imin(int a, int b) { return a < b ? a : b; }
PLVI_HD int imax(int a, int b) { return a > b ? a : b; }
PLVI_HD int imed3(int a, int b, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    return imax(imin(a, b), imin(imax(a, b), c));
#endif
}

// running two smallest keys, b0 <= b1; keys of real rows are distinct
PLVI_HD void top2_update(int& b0, int& b1, int k) {
    b1 = imed3(b0, b1, k);
    b0 = imin(b0, k);
}

// merge of two (b0, b1) lists (the cross-lane step: the partner's pair comes by shuffle)
PLVI_HD void top2_merge(int& b0, int& b1, int p0, int p1) {
    const int hi = imax(b0, p0);
    b0 = imin(b0, p0);
    b1 = imin(hi, imin(b1, p1));
}

// key -> (index, distance); the sentinel is BFMatcher's missing neighbour
PLVI_HD void decode_key(int key, int popq, int& idx, int& dist) {
    if (key == kKeySentinel) {
        idx = -1;
        dist = 0x7fffffff;
    } else {
        key += popq << 16;
        idx = key & 0xffff;
        dist = key >> 16;
    }
}

}  // namespace plvi
