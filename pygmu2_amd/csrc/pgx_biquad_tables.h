// pgx_biquad_tables.h -- the constant BiquadPE's pieces that the oscillator-into-filter kernels of pgx_scan.hip use as well
// as pgx_biquad.hip: the frames per thread, the layout of a section's matrix-power tables (written by k_biquad_tables in
// pgx_biquad.hip) and the moves that read and fold them.  Helpers and constants only (see pgx_scan.h).
#pragma once

#include "pgx_scan.h"

namespace {

constexpr int kBqT = 16;                       // frames per thread per tile

// DPP moves of a double (two 32-bit halves).  CTRL: 0x110+n = row_shr:n (within 16-lane rows),
// 0x138 = wave_shr:1, 0x142 = row_bcast:15, 0x143 = row_bcast:31.  Lanes without a source, or outside
// ROW_MASK, receive 0.0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ V2 dpp_v2(const V2 &v) {
    return V2{dpp_f64<CTRL, ROW_MASK>(v.x), dpp_f64<CTRL, ROW_MASK>(v.y)};
}

// Matrix-power tables of one section, computed once per coefficient set (pgx_biquad_tables):
// A^(16*2^k) for k = 0..5, A^(16*64), then A^(16*j) for j = 0..63.
constexpr int kBqTableDoubles = 28 + 4 * 64 + 2 * kBqT;     // ... then the first rows of A^j, j = 0..kBqT-1 (SINE pass 2)
constexpr int kBqRowsAt = 28 + 4 * 64;

__device__ __forceinline__ M2 load_m2(const double *p) { return M2{p[0], p[1], p[2], p[3]}; }

// p*v + q with fused multiply-adds.  Used only where the result feeds a carry (zero-state responses and
// their scan), never in the output pass, whose operation order is the reference's.
__device__ __forceinline__ V2 mv_add_fma(const M2 &p, const V2 &v, const V2 &q) {
    return V2{__builtin_fma(p.a, v.x, __builtin_fma(p.b, v.y, q.x)),
              __builtin_fma(p.c, v.x, __builtin_fma(p.d, v.y, q.y))};
}

}  // namespace
