// Counter-based Philox4x32-10 (Salmon et al., SC'11), shared by the sampler (sampler.hip) and the bootstrap (bootstrap.hip).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace elimrec {

struct Philox {
    uint32_t c[4];
    uint32_t k[2];
    __device__ static inline void mulhilo(uint32_t a, uint32_t b, uint32_t &hi, uint32_t &lo) {
        const uint64_t p = (uint64_t)a * b;
        hi = (uint32_t)(p >> 32);
        lo = (uint32_t)p;
    }
    // Philox4x32-10 (Salmon et al., SC'11)
    __device__ inline void generate(uint32_t out[4]) const {
        uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], k0 = k[0], k1 = k[1];
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            uint32_t h0, l0, h1, l1;
            mulhilo(0xD2511F53u, c0, h0, l0);
            mulhilo(0xCD9E8D57u, c2, h1, l1);
            const uint32_t n0 = h1 ^ c1 ^ k0, n1 = l1, n2 = h0 ^ c3 ^ k1, n3 = l0;
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    }
};

}  // namespace elimrec
