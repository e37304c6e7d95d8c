// bf16 TABLE STORAGE (include/kge_mi355.h, "bf16 table storage"): the two device-side rules every kernel of that mode shares --
// how a stored value becomes an fp32 one (exactly), and how an fp32 value is stored (stochastic rounding from a counter hash).
// Host and device: the host side is what a stand-alone check of the rule compiles.
#pragma once
#include <stdint.h>

#include "mix_dev.hpp"

namespace kge {

// a stored bf16 value is the top 16 bits of an fp32 pattern: widening is a shift, no rounding
__host__ __device__ inline float bf16_widen(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
// the two values of one 32-bit word of a row (elements 2i and 2i + 1, little endian)
__host__ __device__ inline float bf16_widen_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__host__ __device__ inline float bf16_widen_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }

// the step's key: one mix per launch, on the host
__host__ __device__ inline unsigned long long bf16_step_key(unsigned long long seed, unsigned long long step) {
    return mix64(seed + kMixGamma * (step + 1));
}

// 16 random bits of column j of the row `key` (record row space: entity e -> e, relation r -> E + r); quarter = D / 4.  One mix
// serves the four columns 4 (j >> 2) .. + 3.
__host__ __device__ inline uint32_t bf16_round_bits(unsigned long long k, unsigned long long key, unsigned long long quarter, unsigned j) {
    const unsigned long long z = mix64(k + kMixGamma * (key * quarter + (unsigned long long)(j >> 2) + 1));
    return (uint32_t)(z >> (16 * (j & 3))) & 0xFFFFu;
}

// y -> stored bits.  Adding up to 0xFFFF below the kept bits carries into them with probability (dropped bits) / 2^16: the
// expected stored value is y.  A value with no dropped bits never carries; inf and NaN (exponent all ones) are truncated, so an
// inf stays an inf and a NaN whose kept mantissa bits are set (every quiet NaN) a NaN.  The largest finite magnitudes may carry
// into inf, as any rounding up does.
__host__ __device__ inline uint16_t bf16_round_stochastic(float y, uint32_t rnd) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, y);
    if ((bits & 0x7F800000u) == 0x7F800000u) return (uint16_t)(bits >> 16);
    return (uint16_t)((bits + rnd) >> 16);
}

}  // namespace kge
