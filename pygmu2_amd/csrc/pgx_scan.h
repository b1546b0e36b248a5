// pgx_scan.h -- what the linear-recurrence PEs share: they are evaluated as parallel scans over affine state maps.
//
//   pgx_biquad.hip    BiquadPE (constant)  : 2-state constant map      z' = A z + B x      (biquad_pe.py:383-404)
//   pgx_scan.hip      BiquadPE (varying)   : 2-state time-varying map  [y;y1]' = M_n [y1;y2] + [ff_n;0] (biquad_pe.py:35-62)
//                     SVFilterPE           : 2-state map with a full 2x2 A, constant or per sample (svfilter_pe.py:41-205)
//   pgx_scan.hip      BlitSawPE            : prefix sum (phase) + 1-state constant map (leaky integrator)
//                                            (blit_saw_pe.py:150-264)
//   pgx_phase.hip     SinePE (stateful)    : prefix sum (phase)        (sine_pe.py:177-232)
//   pgx_envelope.hip  EnvelopePE           : 1-state map; with attack != release a walk over regimes (envelope_pe.py:128-271)
//
// This header holds the V2 / M2 algebra, the DPP moves, the frame loads and stores and the wave and block scans: constants,
// structs, __device__ __forceinline__ helpers and templates only, all in the including unit's anonymous namespace.  No
// kernel and no state lives here.
//
// Common structure (wave64, 256-thread workgroups = 4 waves):
//   * a tile is 256 threads x T consecutive frames; every thread folds its T frames into one
//     affine map starting from the zero state (pass 1),
//   * the 64 per-lane maps of a wave are combined with a Kogge-Stone scan over __shfl_up
//     (6 steps; for constant maps only the offset vector travels, the matrix powers
//     A^(T*2^k) are loop invariants kept in LDS),
//   * the 4 wave totals cross through LDS; the tile's carry-out feeds the next tile of the
//     same chain in registers,
//   * every thread then re-runs its T frames from its scanned carry-in in EXACTLY the
//     reference's float64 operation order (pass 2) and stores float32.
// So the only departure from the reference's sequential float64 arithmetic is the rounding
// of each chunk's carry-in (O(1e-16) relative); everything is compiled with -ffp-contract=off.
//
// Long chains are cut into segments, one workgroup each, in one of three ways:
//   * constant sections that forget (k_biquad_settled): each workgroup rebuilds its carry-in from a
//     short warm-up over the frames before its range -- one launch, no cross-workgroup traffic;
//   * constant sections that decay slowly (k_biquad_const<reduce/apply>): a reduce launch produces every
//     segment's zero-state response, the apply launch folds the preceding aggregates (binary powers of
//     A^segment) into its carry-in -- exact for any section;
//   * time-varying maps (k_biquad_varying / k_svf <reduce/apply>): the reduce launch composes each
//     segment's affine map, the apply launch folds the earlier maps onto the carried state.
// Many short chains (voices) use one workgroup per chain and no cross-workgroup traffic at all.
#pragma once

#include "pgx_common.h"

namespace {

constexpr double kPi = 3.141592653589793;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

struct V2 {
    double x, y;
};
struct M2 {
    double a, b, c, d;   // [[a b],[c d]]
};

__device__ __forceinline__ M2 mm(const M2 &p, const M2 &q) {   // p*q
    M2 r;
    r.a = p.a * q.a + p.b * q.c;
    r.b = p.a * q.b + p.b * q.d;
    r.c = p.c * q.a + p.d * q.c;
    r.d = p.c * q.b + p.d * q.d;
    return r;
}
__device__ __forceinline__ V2 mv(const M2 &p, const V2 &v) {
    V2 r;
    r.x = p.a * v.x + p.b * v.y;
    r.y = p.c * v.x + p.d * v.y;
    return r;
}
__device__ __forceinline__ V2 vadd(const V2 &p, const V2 &q) { return V2{p.x + q.x, p.y + q.y}; }
__device__ __forceinline__ M2 m_identity() { return M2{1.0, 0.0, 0.0, 1.0}; }

__device__ __forceinline__ V2 shfl_up_v2(const V2 &v, int d) {
    return V2{__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)};
}

__device__ __forceinline__ double readlane_f64(double v, int src_lane) {   // src_lane wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64_keep(double old, double v) {     // lanes without a source keep `old`
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
// DPP shifts of a 2x2 map / a 2-vector; lanes without a source see the identity map / the zero vector, so a
// scan step needs no lane test.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ M2 dpp_m2_identity(const M2 &m) {
    return M2{dpp_f64_keep<CTRL, ROW_MASK>(1.0, m.a), dpp_f64_keep<CTRL, ROW_MASK>(0.0, m.b),
              dpp_f64_keep<CTRL, ROW_MASK>(0.0, m.c), dpp_f64_keep<CTRL, ROW_MASK>(1.0, m.d)};
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ V2 dpp_v2_zero(const V2 &v) {
    return V2{dpp_f64_keep<CTRL, ROW_MASK>(0.0, v.x), dpp_f64_keep<CTRL, ROW_MASK>(0.0, v.y)};
}

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ------------------------------------------------------------------------------------------------
// Load / store T consecutive frames of one channel of a (frames, channels) float32 buffer.
template <int T>
__device__ __forceinline__ void load_frames(const float *base, int64_t f0, int64_t n, int channels, int ch,
                                            float (&x)[T]) {
    if (channels == 1 && f0 + T <= n && aligned16(base + f0)) {
#pragma unroll
        for (int j = 0; j < T; j += 4) {
            float4 t = *reinterpret_cast<const float4 *>(base + f0 + j);
            x[j] = t.x; x[j + 1] = t.y; x[j + 2] = t.z; x[j + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j) x[j] = (f0 + j < n) ? base[(f0 + j) * channels + ch] : 0.0f;
    }
}

template <int T>
__device__ __forceinline__ void store_frames(float *base, int64_t f0, int64_t n, int channels, int ch,
                                             const float (&y)[T]) {
    if (channels == 1 && f0 + T <= n && aligned16(base + f0)) {
#pragma unroll
        for (int j = 0; j < T; j += 4)
            *reinterpret_cast<float4 *>(base + f0 + j) = make_float4(y[j], y[j + 1], y[j + 2], y[j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j)
            if (f0 + j < n) base[(f0 + j) * channels + ch] = y[j];
    }
}

// Store T frames of a mono result replicated over `channels` output channels (np.tile).
template <int T>
__device__ __forceinline__ void store_frames_tiled(float *base, int64_t f0, int64_t n, int channels,
                                                   const float (&y)[T]) {
    if (channels == 1) {
        store_frames<T>(base, f0, n, 1, 0, y);
    } else {
#pragma unroll
        for (int j = 0; j < T; ++j)
            if (f0 + j < n)
                for (int c = 0; c < channels; ++c) base[(f0 + j) * channels + c] = y[j];
    }
}

// ------------------------------------------------------------------------------------------------
// Block-wide exclusive prefix sum of one double per thread: pgx::block_excl_sum (pgx_common.h; TimeWarpPE's
// position scan in pgx_lookup.hip integrates its rate with the same routine).
__device__ __forceinline__ double block_excl_sum(double v, double *lds, double &total) {
    return pgx::block_excl_sum<kWaves>(v, lds, total);
}

// Block-wide scan for the scalar constant map y' = lam^len * y + b.  On entry `e` is this thread's
// zero-state chunk response; lamp[k] = lam^(T*2^k) for k=0..5, lam_wave = lam^(T*64),
// lam_lane = lam^(T*lane).  Returns this thread's carry-in given the tile carry-in `carry`, and
// updates `carry` to the tile carry-out.  `lds` holds kWaves doubles.
__device__ __forceinline__ double block_scan_scalar_affine(double e, const double (&lamp)[6], double lam_wave,
                                                           double lam_lane, double *lds, double &carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double inc = e;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double o = __shfl_up(inc, 1 << k, 64);
        if (lane >= (1 << k)) inc = lamp[k] * o + inc;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    double cw = carry, cn = carry;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        double t = lds[w];
        if (w < wave) cw = lam_wave * cw + t;
        cn = lam_wave * cn + t;
    }
    __syncthreads();
    carry = cn;
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    return lam_lane * cw + ex;
}

// Inclusive scans over a wave on DPP moves (VALU; a `__shfl_up` step is two ds_bpermute round trips through LDS):
// Kogge-Stone inside each 16-lane row (row_shr), then row 0 -> 1 and 2 -> 3 (lane 15 of the previous row), then
// rows 0-1 -> 2, 3 (lane 31).  Lanes without a source receive the neutral element.  Every oscillator kernel scans
// with these two, so their folds -- and bits -- agree with each other.
__device__ __forceinline__ double wave_incl_sum_dpp(double v) {
    v = dpp_f64_keep<0x111, 0xf>(0.0, v) + v;
    v = dpp_f64_keep<0x112, 0xf>(0.0, v) + v;
    v = dpp_f64_keep<0x114, 0xf>(0.0, v) + v;
    v = dpp_f64_keep<0x118, 0xf>(0.0, v) + v;
    v = dpp_f64_keep<0x142, 0xa>(0.0, v) + v;
    v = dpp_f64_keep<0x143, 0xc>(0.0, v) + v;
    return v;
}
// y' = lam^len * y + b: lamp[k] = lam^(T*2^k); lam16 / lam32 = lam^(T*((lane & 15) + 1)) / lam^(T*((lane & 31) + 1))
__device__ __forceinline__ double wave_incl_affine_dpp(double e, const double (&lamp)[6], double lam16, double lam32) {
    // (fused multiply-adds: these numbers only feed carries -- the samples themselves are re-run from the scanned
    // carry-in in the reference's operation order; k_blitsaw_chain folds with the same fused step)
    e = __builtin_fma(lamp[0], dpp_f64_keep<0x111, 0xf>(0.0, e), e);
    e = __builtin_fma(lamp[1], dpp_f64_keep<0x112, 0xf>(0.0, e), e);
    e = __builtin_fma(lamp[2], dpp_f64_keep<0x114, 0xf>(0.0, e), e);
    e = __builtin_fma(lamp[3], dpp_f64_keep<0x118, 0xf>(0.0, e), e);
    e = __builtin_fma(lam16, dpp_f64_keep<0x142, 0xa>(0.0, e), e);
    e = __builtin_fma(lam32, dpp_f64_keep<0x143, 0xc>(0.0, e), e);
    return e;
}
// the per-lane powers of a scan over chunks of T samples, from lamp[k] = lam^(T*2^k)
struct LanePowers {
    double lane, p16, p32;      // lam^(T*lane), lam^(T*((lane & 15) + 1)), lam^(T*((lane & 31) + 1))
};
__device__ __forceinline__ LanePowers lane_powers(const double (&lamp)[6], int lane) {
    LanePowers r{1.0, 1.0, 1.0};
    const int a = (lane & 15) + 1, b = (lane & 31) + 1;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        if (lane & (1 << k)) r.lane = r.lane * lamp[k];
        if (a & (1 << k)) r.p16 = r.p16 * lamp[k];
        if (b & (1 << k)) r.p32 = r.p32 * lamp[k];
    }
    return r;
}

// Wide forms for a workgroup of NW = 4*G waves that must reproduce, bit for bit, what a 4-wave workgroup
// computes on G consecutive tiles: the wave values are the same, so it is enough to fold them in the same
// order.  sum_carry: running sum entering the first of the G tiles (advanced to the one leaving the last).
template <int NW>
__device__ __forceinline__ double block_excl_sum_wide(double v, double *lds, double &sum_carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inc = wave_incl_sum_dpp(v);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    double base = sum_carry, mine_base = sum_carry, woff = 0.0;
#pragma unroll
    for (int g = 0; g < NW / kWaves; ++g) {
        double tot = 0.0, w_local = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const double t = lds[g * kWaves + w];
            if (g * kWaves + w < wave) w_local = w_local + t;
            tot = tot + t;
        }
        if (g == wave / kWaves) {
            mine_base = base;
            woff = w_local;
        }
        base = base + tot;                                   // carry_sum = carry_sum + tile_total
    }
    __syncthreads();
    sum_carry = base;
    const double ex = dpp_f64_keep<0x138, 0xf>(0.0, inc);   // wave_shr:1 -- the lane before, 0 for lane 0
    return mine_base + (woff + ex);                          // chunk_base = carry_sum + off
}

template <int NW>
__device__ __forceinline__ double block_scan_scalar_affine_wide(double e, const double (&lamp)[6], double lam_wave,
                                                                double lam_lane, double *lds, double &carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double inc = e;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double o = __shfl_up(inc, 1 << k, 64);
        if (lane >= (1 << k)) inc = lamp[k] * o + inc;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    double cw = carry, cn = carry;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        double t = lds[w];
        if (w < wave) cw = lam_wave * cw + t;
        cn = lam_wave * cn + t;
    }
    __syncthreads();
    carry = cn;
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    return lam_lane * cw + ex;
}

// block_excl_sum_wide when every thread contributes the SAME value (a scalar-frequency oscillator on a tile
// whose frames are all live): every wave's total is the same number, so the folds need no exchange and no
// barrier.  Same operations in the same order as the exchanging form, hence the same bits.
// The two numbers block_excl_sum_wide_uniform derives from v alone: this thread's offset inside the tile and what the
// carry advances by per group of kWaves waves.  With them a tile's prefix is `carry + offset` (groups before the
// thread's own first advance the carry): a caller whose v never changes makes them once -- same operations, same bits.
struct UniformPrefix {
    double offset, tot;
};
__device__ __forceinline__ UniformPrefix uniform_prefix(double v) {
    const int wave = threadIdx.x >> 6;
    const double inc = wave_incl_sum_dpp(v);
    const double t = readlane_f64(inc, 63);
    double tot = 0.0, w_local = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < (wave & (kWaves - 1))) w_local = w_local + t;
        tot = tot + t;
    }
    const double ex = dpp_f64_keep<0x138, 0xf>(0.0, inc);
    return UniformPrefix{w_local + ex, tot};
}
template <int NW>
__device__ __forceinline__ double block_excl_sum_wide_uniform(const UniformPrefix &u, double &sum_carry) {
    const int wave = threadIdx.x >> 6;
    double base = sum_carry, mine_base = sum_carry;
#pragma unroll
    for (int g = 0; g < NW / kWaves; ++g) {
        if (g == wave / kWaves) mine_base = base;
        base = base + u.tot;
    }
    sum_carry = base;
    return mine_base + u.offset;
}
template <int NW>
__device__ __forceinline__ double block_excl_sum_wide_uniform(double v, double &sum_carry) {
    return block_excl_sum_wide_uniform<NW>(uniform_prefix(v), sum_carry);
}

// block_scan_scalar_affine_wide with ONE barrier: `lds` holds two images of NW doubles used alternately
// (`parity` flips on every call), so the readers of one image are separated from its next writer by the
// barrier of the call in between.
template <int NW>
__device__ __forceinline__ double block_scan_scalar_affine_wide1(double e, const double (&lamp)[6], double lam_wave,
                                                                 const LanePowers &lp, double *lds, int parity,
                                                                 double &carry) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *img = lds + (parity & 1) * NW;
    const double inc = wave_incl_affine_dpp(e, lamp, lp.p16, lp.p32);
    if (lane == 63) img[wave] = inc;
    __syncthreads();
    double cw = carry, cn = carry;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        double t = img[w];
        if (w < wave) cw = __builtin_fma(lam_wave, cw, t);
        cn = __builtin_fma(lam_wave, cn, t);
    }
    carry = cn;
    const double ex = dpp_f64_keep<0x138, 0xf>(0.0, inc);
    return __builtin_fma(lp.lane, cw, ex);
}

}  // namespace
