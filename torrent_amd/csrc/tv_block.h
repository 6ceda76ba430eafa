// tv_block.h -- 64-byte message blocks of a byte range in HBM, shared by the SHA-1 kernels (tv_kernels.hip) and the
// SHA-256 merkle kernels (tv_v2_kernels.hip): both hashes pad alike (0x80, zeros, the 64-bit big-endian bit length).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }
__device__ __forceinline__ uint64_t nblocks(uint64_t len) { return (len + 8) / 64 + 1; }

// Build the 16 big-endian message words of block b of a piece of length len whose byte 0 is
// at `piece` (slow path: data tail, 0x80 terminator, zero fill, bit length).  Reads at most
// 64 bytes from piece + 64*b; the buffers carry >= 64 bytes of slack past every piece.
__device__ __forceinline__ void build_tail_block(const uint8_t* piece, uint64_t len, uint64_t b,
                                                 uint32_t w[16]) {
    const int64_t rem = (int64_t)len - (int64_t)(b * 64);
    uint4 raw[4];
    if (rem > 0) {
        const uint4* src = reinterpret_cast<const uint4*>(piece + b * 64);
#pragma unroll
        for (int i = 0; i < 4; i++) raw[i] = src[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) raw[i] = make_uint4(0, 0, 0, 0);
    }
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(raw);
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int64_t v = rem - 4 * k;  // valid data bytes in word k (may be <0 or >=4)
        uint32_t x = bswap32(rw[k]);
        if (v < 4) {
            if (v < 0) {
                x = 0;
            } else {
                const uint32_t keep = v == 0 ? 0u : (0xFFFFFFFFu << (32 - 8 * (int)v));
                x = (x & keep) | (0x80u << (24 - 8 * (int)v));
            }
        }
        w[k] = x;
    }
    if (b == nblocks(len) - 1) {
        const uint64_t bits = len * 8;
        w[14] = (uint32_t)(bits >> 32);
        w[15] = (uint32_t)bits;
    }
}

__device__ __forceinline__ void load_block(const uint8_t* piece, uint32_t b, uint4 (&r)[4]) {
    const uint4* src = reinterpret_cast<const uint4*>(piece + (uint64_t)b * 64);
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = src[i];
}

}  // namespace
