// The 64-bit finaliser behind every counter-based draw of the engine (the candidates kge_rank_candidates draws, the shared
// negatives of kge_shared_negatives_draw): splitmix64's output function.  All arithmetic is mod 2^64.  Defined once, for the host
// and the device.
#pragma once

namespace kge {

constexpr unsigned long long kMixGamma = 0x9E3779B97F4A7C15ULL;   // the counter's stride: draw c reads mix64(key + (c + 1) * kMixGamma)

__host__ __device__ inline unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}

// the high word of a mixed value scaled to [0, n): ((z >> 32) * n) >> 32, n < 2^32
__host__ __device__ inline unsigned long long mix_scale(unsigned long long z, unsigned long long n) { return ((z >> 32) * n) >> 32; }

}  // namespace kge
