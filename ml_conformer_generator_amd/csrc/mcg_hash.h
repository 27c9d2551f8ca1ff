// H of the graph keys ("Chemical fingerprints"): MurmurHash3_x86_32 over uint32 words, one 4-byte block
// at a time, and the two seeds of a 64-bit key's halves.  The fingerprint key and the canonical key are this one hash.
#pragma once
#include <stdint.h>

constexpr uint32_t MCG_HASH_SEED = 0x6d636731u;
constexpr uint32_t MCG_HASH_SEED_HI = MCG_HASH_SEED ^ 0x9e3779b9u;

__device__ __forceinline__ uint32_t mm3_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ __forceinline__ uint32_t mm3_mix(uint32_t h, uint32_t k) {
    k *= 0xcc9e2d51u;
    k = mm3_rotl32(k, 15);
    k *= 0x1b873593u;
    h ^= k;
    h = mm3_rotl32(h, 13);
    return h * 5u + 0xe6546b64u;
}

__device__ __forceinline__ uint32_t mm3_final(uint32_t h, uint32_t n_words) {
    h ^= 4u * n_words;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
