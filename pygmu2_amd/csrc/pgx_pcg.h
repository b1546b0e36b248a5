// pgx_pcg.h -- numpy's PCG64 on the device, shared by pgx_noise.hip (NoisePE) and pgx_spectral.hip (TralfamPE).
//
// PCG64 is a 128-bit LCG  s <- M * s + inc  (stepped BEFORE the output is taken) with the XSL-RR output
// u64 = rotr64(hi ^ lo, hi >> 58).  n steps are  s -> M^n * s + inc * S_n,  S_n = 1 + M + ... + M^(n-1); the skip
// table holds (M^(2^k), S_(2^k)) for k = 0..63, made at compile time from M alone.  The library keeps ONE copy of it
// in device memory: the __constant__ table of pgx_noise.hip.  Other translation units reach it through
// pcg_skip_table_device() and hand the pointer to their kernels.
#pragma once

#include "pgx_common.h"

namespace pgx {

typedef unsigned __int128 u128;

constexpr u128 kPcgMult = ((u128)0x2360ED051FC65DA4ULL << 64) | (u128)0x4385DF649FCCF645ULL;

struct SkipTable {
    u128 a[64];     // M^(2^k)
    u128 c[64];     // S_(2^k) = 1 + M + ... + M^(2^k - 1)
};

constexpr SkipTable make_skip_table() {
    SkipTable t{};
    u128 a = kPcgMult, c = 1;
    for (int k = 0; k < 64; ++k) {
        t.a[k] = a;
        t.c[k] = c;
        c = c * (a + 1);        // S_2n = S_n + M^n * S_n
        a = a * a;
    }
    return t;
}

// device address of the library's skip table (defined in pgx_noise.hip); nullptr with the error set on failure
const SkipTable *pcg_skip_table_device();

#ifdef __HIPCC__
__device__ __forceinline__ u128 make128(uint64_t hi, uint64_t lo) { return ((u128)hi << 64) | (u128)lo; }

// `d` LCG steps from s
__device__ __forceinline__ u128 pcg_skip_with(const SkipTable &t, u128 s, u128 inc, uint64_t d) {
    for (int k = 0; d != 0; ++k, d >>= 1)
        if (d & 1) s = t.a[k] * s + t.c[k] * inc;
    return s;
}

// the 64-bit draw numpy takes from state s (already stepped)
__device__ __forceinline__ uint64_t pcg_output(u128 s) {
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    const uint64_t x = hi ^ lo;
    const unsigned rot = (unsigned)(hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}
#endif

}  // namespace pgx
