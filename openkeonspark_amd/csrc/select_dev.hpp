// Device-side k-smallest selection shared by the top-k entity (topk.hip) and relation (relpred.hip) kernels: (score, id)
// packed into one orderable 64-bit key, and LDS key buffers that are sorted (bitonic) back to their k smallest keys.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kge {

constexpr uint64_t kNoKey = ~0ull;   // padding: id -1, score +inf; above every real key (a NaN key's low word is an id < 2^31)

// orderable score bits << 32 | id: ascending (score, id), NaN after every number
__device__ __forceinline__ uint64_t pack_key(float s, int id) {
    const uint32_t b = __float_as_uint(s);
    const uint32_t ord = s != s ? 0xFFFFFFFFu : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
    return ((uint64_t)ord << 32) | (uint32_t)id;
}
__device__ __forceinline__ void unpack_key(uint64_t key, int32_t &id, float &s) {
    if (key == kNoKey) { id = -1; s = __uint_as_float(0x7F800000u); return; }
    const uint32_t ord = (uint32_t)(key >> 32);
    id = (int32_t)(uint32_t)key;
    s = ord == 0xFFFFFFFFu ? __uint_as_float(0x7FC00000u) : __uint_as_float((ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord);
}

// Sorts the buffers q with bit q of `need` (ascending; `cap` keys each, a power of two) -- all threads of the block call it.
__device__ inline void sort_buffers(uint64_t *keys, int cap, int nbuf, unsigned need) {
    const int half = cap >> 1;
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int idx = threadIdx.x; idx < nbuf * half; idx += blockDim.x) {
                const int q = idx / half, i = idx - q * half;
                if (!((need >> q) & 1u)) continue;
                uint64_t *b = keys + (long long)q * cap;
                const int pos = 2 * i - (i & (stride - 1));
                const uint64_t x = b[pos], y = b[pos + stride];
                if ((x > y) == ((pos & size) == 0)) { b[pos] = y; b[pos + stride] = x; }
            }
            __syncthreads();
        }
    }
}

// Brings the buffers in `need` back to their k smallest keys and raises their thresholds.  Block-uniform call.
__device__ inline void shrink_buffers(uint64_t *keys, int cap, int nbuf, unsigned need, int k, int *cnt, uint64_t *thr) {
    for (int q = 0; q < nbuf; q++) {
        if (!((need >> q) & 1u)) continue;
        for (int i = cnt[q] + (int)threadIdx.x; i < cap; i += blockDim.x) keys[(long long)q * cap + i] = kNoKey;
    }
    __syncthreads();
    sort_buffers(keys, cap, nbuf, need);
    if ((int)threadIdx.x < nbuf && ((need >> threadIdx.x) & 1u)) {
        const int q = threadIdx.x;
        if (cnt[q] >= k) { thr[q] = keys[(long long)q * cap + k - 1]; cnt[q] = k; }
    }
    __syncthreads();
}

}  // namespace kge
