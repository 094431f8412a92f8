// CRC-32 (RFC 1952 8) of a BGZF member's bytes on the device, shared by the reader (k_crc32, nc_inflate.hip: the inflated members against
// their trailers) and the writer (k_member_crc, nc_bamwrite.hip: the trailers of the members it compresses).
// One wave per member.  The member's <= 64 KB are cut from their END into 64 slices of 1024 bytes (the first non-empty slice is the short one
// and starts from the initial register 0xffffffff); a lane runs slice-by-4 over its slice (tables in LDS, dwords from 4-byte aligned
// addresses); the 64 partial registers combine in a tree whose level l multiplies by x^(8 * 1024 * 2^l) mod P -- six constants, since every
// slice but the first has the same length (an empty lane's register is 0).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace nc_crc {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
struct CrcOps { uint32_t x[6]; };                                      // x^(8 * 1024 * 2^l) mod P, reflected representation, l = 0 .. 5

__host__ __device__ inline uint32_t crc_multmodp(uint32_t a, uint32_t b)      // a * b mod P (zlib's crc32 combine arithmetic)
{
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// the kernels' argument: computed once per process on the host
inline CrcOps crc_ops()
{
    static const CrcOps ops = []() {
        CrcOps o;
        uint32_t p = 1u << 30;                                          // x^1
        for (int k = 0; k < 13; k++) p = crc_multmodp(p, p);           // x^(2^13) = x^(8 * 1024)
        for (int l = 0; l < 6; l++) { o.x[l] = p; p = crc_multmodp(p, p); }
        return o;
    }();
    return ops;
}

// the slice-by-4 tables, by a workgroup of 256 threads (two barriers)
__device__ __forceinline__ void crc_tables(uint32_t (*T)[256], int tid)
{
    {
        uint32_t c = (uint32_t)tid;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
        T[0][tid] = c;
    }
    __syncthreads();
    {
        uint32_t c = T[0][tid];
#pragma unroll
        for (int t = 1; t < 4; t++) { c = (c >> 8) ^ T[0][c & 0xffu]; T[t][tid] = c; }
    }
    __syncthreads();
}

// CRC-32 of base[0, n), n <= 65536, by the 64 lanes of one wave (every lane returns it)
__device__ __forceinline__ uint32_t crc_wave(const uint8_t *base, int n, int lane, const uint32_t (*T)[256], const CrcOps &ops)
{
    // slice `lane` covers bytes [n - (64 - lane) * 1024, n - (63 - lane) * 1024) of the member, clipped at 0
    const int hi = n - (63 - lane) * 1024, lo = max(hi - 1024, 0);
    int len = hi > 0 ? hi - lo : 0;
    uint32_t crc = (len > 0 && lo == 0) ? 0xffffffffu : 0u;            // the first non-empty slice carries the initial register
    const uint8_t *q = base + lo;
    for (; len > 0 && ((uintptr_t)q & 3); len--) crc = (crc >> 8) ^ T[0][(crc ^ *q++) & 0xffu];      // up to the next aligned dword (the short first slice only, or an unaligned member)
    const uint32_t *w = reinterpret_cast<const uint32_t *>(q);
    for (int i = 0; i + 4 <= len; i += 4) {
        const uint32_t x = crc ^ *w++;
        crc = T[3][x & 0xffu] ^ T[2][(x >> 8) & 0xffu] ^ T[1][(x >> 16) & 0xffu] ^ T[0][x >> 24];
    }
    q = reinterpret_cast<const uint8_t *>(w);
    for (int i = len & ~3; i < len; i++) crc = (crc >> 8) ^ T[0][(crc ^ *q++) & 0xffu];
    // tree: at level l the register of the left half moves 1024 * 2^l bytes forward
#pragma unroll
    for (int l = 0; l < 6; l++) {
        const uint32_t other = (uint32_t)__shfl_xor((int)crc, 1 << l);
        const bool right = (lane >> l) & 1;
        const uint32_t left_c = right ? other : crc, right_c = right ? crc : other;
        crc = crc_multmodp(ops.x[l], left_c) ^ right_c;               // (both lanes of a pair compute the same value)
    }
    return n > 0 ? crc ^ 0xffffffffu : 0u;
}

}   // namespace nc_crc
