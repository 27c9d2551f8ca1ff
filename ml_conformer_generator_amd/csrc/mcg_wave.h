// The 64-lane helpers of the kernels that run one wave per molecule with lane = atom and one bit of a 64-bit mask per
// atom ("The shared prologue of the graph kernels").  A reduction is the fixed xor butterfly
// off = 32 ... 1 with v = op(v, other): every lane ends with the same bits, and a float sum keeps that one order.
#pragma once
#include <stdint.h>

template <class T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

template <class T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}

template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo |= __shfl_xor(lo, off);
        hi |= __shfl_xor(hi, off);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// the index of the lowest set bit; -1 for an empty mask
__device__ __forceinline__ int low_bit(unsigned long long m) { return __ffsll((long long)m) - 1; }

// bits 0..n-1; n = 64 has no `1ull << 64`
__device__ __forceinline__ unsigned long long low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }
