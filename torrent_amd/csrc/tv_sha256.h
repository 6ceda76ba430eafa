// tv_sha256.h -- one SHA-256 compression (FIPS 180-4) in plain C++, for the BitTorrent v2 merkle kernels
// (tv_v2_kernels.hip).  On gfx950 each three-input boolean (the xor of three rotations in the four sigmas, Ch, Maj)
// is one v_bitop3_b32 and each rotation one v_alignbit_b32; a host compile (the CPU check of this header against
// hashlib's known answers) takes the same functions through the plain operators.
#pragma once
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define TV_SHA256_FN __device__ __forceinline__
// bitop3: result bit = imm[(a << 2) | (b << 1) | c]
#define TV_XOR3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)
#define TV_CH(e, f, g) __builtin_amdgcn_bitop3_b32((e), (f), (g), 0xCA)
#define TV_MAJ(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0xE8)
#define TV_ROR(x, n) __builtin_rotateright32((x), (n))
#else
#if defined(__HIPCC__)
#define TV_SHA256_FN __host__ __device__ inline
#else
#define TV_SHA256_FN inline
#endif
#define TV_XOR3(a, b, c) ((a) ^ (b) ^ (c))
#define TV_CH(e, f, g) (((e) & (f)) | (~(e) & (g)))
#define TV_MAJ(a, b, c) (((a) & (b)) | ((a) & (c)) | ((b) & (c)))
#define TV_ROR(x, n) (((x) >> (n)) | ((x) << (32 - (n))))
#endif

namespace tv256 {

constexpr uint32_t kK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

TV_SHA256_FN void iv(uint32_t h[8]) {
    h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

// out = the chaining value after the block w (16 big-endian message words; w is consumed as the rolling schedule).
// out may alias h.
TV_SHA256_FN void compress(const uint32_t h[8], uint32_t w[16], uint32_t out[8]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int t = 0; t < 64; t++) {
        if (t >= 16) {
            const uint32_t x = w[(t + 1) & 15], y = w[(t + 14) & 15];
            const uint32_t s0 = TV_XOR3(TV_ROR(x, 7), TV_ROR(x, 18), x >> 3);
            const uint32_t s1 = TV_XOR3(TV_ROR(y, 17), TV_ROR(y, 19), y >> 10);
            w[t & 15] = w[t & 15] + s0 + w[(t + 9) & 15] + s1;
        }
        const uint32_t S1 = TV_XOR3(TV_ROR(e, 6), TV_ROR(e, 11), TV_ROR(e, 25));
        const uint32_t S0 = TV_XOR3(TV_ROR(a, 2), TV_ROR(a, 13), TV_ROR(a, 22));
        const uint32_t t1 = hh + S1 + TV_CH(e, f, g) + kK[t] + w[t & 15];
        const uint32_t t2 = S0 + TV_MAJ(a, b, c);
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    const uint32_t r[8] = {a, b, c, d, e, f, g, hh};
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = h[i] + r[i];
}

}  // namespace tv256
