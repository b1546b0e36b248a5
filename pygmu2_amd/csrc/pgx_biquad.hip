// pgx_biquad.hip -- BiquadPE with constant coefficients (biquad_pe.py:383-404) as a scan over the constant 2-state map
// z' = A z + B x: the exact reduce + apply pair, the settled single launch, and the BiquadPE(SinePE) window kernels (the
// sine generated in registers; wave runs with deadline pacing).  Scan primitives: pgx_scan.h.

#include <cstdlib>
#include <type_traits>

#include "pgx_common.h"
#include "pgx_scan.h"
#include "pgx_biquad_tables.h"

namespace {

// ================================================================================================
// BiquadPE, constant coefficients
// ================================================================================================
constexpr int kBqTile = kBlock * kBqT;         // 4096 frames
constexpr int kBqMaxSeg = 1024;
constexpr int kBqPow = 11;                     // binary powers of A^segment kept for the fold

struct BqShared {
    M2 pstep[6];       // A^(T*2^k)
    M2 pwave;          // A^(T*64)
    M2 ptile;          // A^(T*256)
    M2 pseg[kBqPow];   // (A^segment)^(2^k)
    V2 wave_tot[kWaves];
    V2 red[kWaves];
};

// MODE 0: reduce (write the segment's zero-state response to agg); MODE 1: apply (produce output).
template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_biquad_const(float *out, int64_t out_stride, const float *in, int64_t in_stride, int64_t n, int channels,
               const double *coef, double *state, const double *state_snapshot, double *agg, int seg_tiles,
               int nseg) {
    __shared__ BqShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chain = blockIdx.y;
    const int inst = chain / channels, ch = chain - inst * channels;
    const int seg = blockIdx.x;

    const double b0 = coef[inst * 5 + 0], b1 = coef[inst * 5 + 1], b2 = coef[inst * 5 + 2];
    const double a1 = coef[inst * 5 + 3], a2 = coef[inst * 5 + 4];

    // ---- loop-invariant matrix powers (thread 0 -> LDS) ----
    if (tid == 0) {
        M2 A{-a1, 1.0, -a2, 0.0};
        M2 p = A;
#pragma unroll
        for (int s = 1; s < kBqT; s <<= 1) p = mm(p, p);     // A^T (T is a power of two)
        for (int k = 0; k < 6; ++k) {
            sh.pstep[k] = p;
            p = mm(p, p);
        }
        sh.pwave = p;                                        // A^(64 T)
        p = mm(p, p);
        p = mm(p, p);
        sh.ptile = p;                                        // A^(256 T)
        if (nseg > 1) {
            // A^segment = ptile^seg_tiles (binary exponentiation), then its binary powers.
            M2 r = m_identity(), q = p;
            for (int e = seg_tiles; e > 0; e >>= 1) {
                if (e & 1) r = mm(r, q);
                q = mm(q, q);
            }
            for (int k = 0; k < kBqPow; ++k) {
                sh.pseg[k] = r;
                r = mm(r, r);
            }
        }
    }
    __syncthreads();

    M2 mlane = m_identity();                                  // A^(T*lane)
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (lane & (1 << k)) mlane = mm(sh.pstep[k], mlane);

    // ---- segment carry-in ----
    V2 carry{0.0, 0.0};
    if (MODE == 1) {
        if (nseg == 1) {
            carry = V2{state[chain * 2 + 0], state[chain * 2 + 1]};
        } else {
            // carry = (A^seg)^seg_index * z_init + sum_{j<seg} (A^seg)^(seg-1-j) * agg_j
            V2 part{0.0, 0.0};
            for (int j = tid; j <= seg; j += kBlock) {
                V2 v;
                int e;
                if (j == seg) {                               // the initial-state term
                    v = V2{state_snapshot[chain * 2 + 0], state_snapshot[chain * 2 + 1]};
                    e = seg;
                } else {
                    v = V2{agg[((int64_t)chain * nseg + j) * 2 + 0], agg[((int64_t)chain * nseg + j) * 2 + 1]};
                    e = seg - 1 - j;
                }
                for (int k = 0; k < kBqPow; ++k)
                    if (e & (1 << k)) v = mv(sh.pseg[k], v);
                part = vadd(part, v);
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                part.x += __shfl_down(part.x, d, 64);
                part.y += __shfl_down(part.y, d, 64);
            }
            if (lane == 0) sh.red[wave] = part;
            __syncthreads();
            carry = V2{0.0, 0.0};
#pragma unroll
            for (int w = 0; w < kWaves; ++w) carry = vadd(carry, sh.red[w]);
            __syncthreads();
        }
    }

    const float *ib = in + (int64_t)inst * in_stride;
    float *ob = out + (int64_t)inst * out_stride;
    V2 final_state{0.0, 0.0};
    bool have_final = false;

    const int64_t tile0 = (int64_t)seg * seg_tiles;
    for (int t = 0; t < seg_tiles; ++t) {
        const int64_t base = (tile0 + t) * kBqTile;
        if (base >= n) break;
        const int64_t f0 = base + (int64_t)tid * kBqT;
        float xf[kBqT];
        load_frames<kBqT>(ib, f0, n, channels, ch, xf);

        // pass 1: zero-state response of this chunk
        V2 e{0.0, 0.0};
#pragma unroll
        for (int j = 0; j < kBqT; ++j) {
            double x = (double)xf[j];
            double y = e.x + b0 * x;
            double z0 = (e.y + b1 * x) - a1 * y;
            e.y = b2 * x - a2 * y;
            e.x = z0;
        }
        // wave scan (offset vectors only; the matrices are the LDS-resident powers)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            V2 o = shfl_up_v2(e, 1 << k);
            if (lane >= (1 << k)) e = vadd(mv(sh.pstep[k], o), e);
        }
        if (lane == 63) sh.wave_tot[wave] = e;
        __syncthreads();
        V2 cw = carry, cn = carry;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            V2 tot = sh.wave_tot[w];
            if (w < wave) cw = vadd(mv(sh.pwave, cw), tot);
            cn = vadd(mv(sh.pwave, cn), tot);
        }
        __syncthreads();
        carry = cn;

        if (MODE == 1) {
            V2 ex = shfl_up_v2(e, 1);
            if (lane == 0) ex = V2{0.0, 0.0};
            V2 z = vadd(mv(mlane, cw), ex);
            float yf[kBqT];
            // pass 2: scipy lfilter DF-II-T operation order from the scanned carry-in
#pragma unroll
            for (int j = 0; j < kBqT; ++j) {
                double x = (double)xf[j];
                double y = z.x + b0 * x;
                double z0 = (z.y + b1 * x) - a1 * y;
                z.y = b2 * x - a2 * y;
                z.x = z0;
                yf[j] = (float)y;
                if (f0 + j == n - 1) {
                    final_state = z;
                    have_final = true;
                }
            }
            store_frames<kBqT>(ob, f0, n, channels, ch, yf);
        }
    }
    if (MODE == 0) {
        if (tid == 0) {
            agg[((int64_t)chain * nseg + seg) * 2 + 0] = carry.x;
            agg[((int64_t)chain * nseg + seg) * 2 + 1] = carry.y;
            if (seg == 0) {
                // snapshot of the carried state for the apply launch (whose last segment overwrites
                // `state` while other segments may not have started yet)
                double *snap = const_cast<double *>(state_snapshot);
                snap[chain * 2 + 0] = state[chain * 2 + 0];
                snap[chain * 2 + 1] = state[chain * 2 + 1];
            }
        }
    } else if (have_final) {
        state[chain * 2 + 0] = final_state.x;
        state[chain * 2 + 1] = final_state.y;
    }
}

// ------------------------------------------------------------------------------------------------
// Settled single launch.  A stable section forgets: once every entry of A^W is below 2^-90 the state W
// frames back no longer reaches the float64 arithmetic of the present.  Each workgroup then recovers
// its carry-in by running the recurrence from zero over the frames that precede its range (outputs
// discarded) instead of waiting for its predecessors: one launch, no cross-workgroup traffic, every
// input frame fetched from HBM once (the warm-up frames are L2/MALL hits of a neighbour's fetch).
// W is evaluated by the host from the coefficients (pgx_biquad_const's settle_frames); slowly decaying
// sections (W above kSbMaxWarm half-tiles) keep the exact reduce + apply pair.
//
// Geometry: 512 threads x 16 frames = one 8192-frame tile, addressed in 4096-frame halves so that the
// smallest plan (one half of warm-up + one half of output per workgroup) is a single scan step.
// Workgroup 0 renders the halves [0, head) and the tail [tail_start, halves): it alone reads the
// carried state (first thing) and writes it (last thing); workgroup g >= 1 renders seg halves from
// head + (g-1)*seg.  head >= warm, so no other workgroup ever needs the carried state.
// ------------------------------------------------------------------------------------------------
constexpr int kSbBlock = 512;
constexpr int kSbWaves = kSbBlock / 64;
constexpr int kSbHalf = (kSbBlock / 2) * kBqT;     // 4096 frames
constexpr int kSbMaxWarm = 16;                     // half-tiles

struct SbShared {
    V2 wave_tot[2][kSbWaves];        // two images used in turn: one barrier per tile (the readers of one image are
};                                   // separated from its next writer by the barrier of the tile in between)

// Staging of a wave's 1024 frames through wave-private LDS: HBM is touched with fully coalesced 16-byte
// accesses (lane l of access i owns frames i*256 + 4l ..), the scan wants 16 consecutive frames per lane.
// Chunk c (16 frames) lives at word c*20: the 4-word pad makes both access patterns bank-conflict free.
constexpr int kStageWords = 64 * 20;

__device__ __forceinline__ void stage_fetch(const float *src, int lane, float (&t)[kBqT]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = *reinterpret_cast<const float4 *>(src + i * 256 + lane * 4);
        t[4 * i] = v.x; t[4 * i + 1] = v.y; t[4 * i + 2] = v.z; t[4 * i + 3] = v.w;
    }
}
__device__ __forceinline__ int stage_slot(int i, int lane) {       // LDS word of frame i*256 + 4*lane
    const int idx = i * 256 + lane * 4;
    return (idx >> 4) * 20 + (idx & 15);
}
// coalesced order (as fetched) -> 16 consecutive frames per lane
__device__ __forceinline__ void stage_to_chunks(float *lds, int lane, float (&t)[kBqT]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4 *>(lds + stage_slot(i, lane)) = make_float4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = *reinterpret_cast<const float4 *>(lds + lane * 20 + 4 * i);
        t[4 * i] = v.x; t[4 * i + 1] = v.y; t[4 * i + 2] = v.z; t[4 * i + 3] = v.w;
    }
}
// 16 consecutive frames per lane -> coalesced stores
__device__ __forceinline__ void stage_store(float *lds, float *dst, int lane, const float (&y)[kBqT]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4 *>(lds + lane * 20 + 4 * i) = make_float4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4 *>(dst + i * 256 + lane * 4) = *reinterpret_cast<const float4 *>(lds + stage_slot(i, lane));
}

__global__ void __launch_bounds__(64)
k_biquad_tables(double *tables, const double *coef) {
    __shared__ M2 ps[6];
    const int lane = threadIdx.x, inst = blockIdx.x;
    double *tb = tables + (int64_t)inst * kBqTableDoubles;
    if (lane == 0) {
        M2 p{-coef[inst * 5 + 3], 1.0, -coef[inst * 5 + 4], 0.0};
#pragma unroll
        for (int s = 1; s < kBqT; s <<= 1) p = mm(p, p);
        for (int k = 0; k < 6; ++k) {
            ps[k] = p;
            tb[4 * k] = p.a; tb[4 * k + 1] = p.b; tb[4 * k + 2] = p.c; tb[4 * k + 3] = p.d;
            p = mm(p, p);
        }
        tb[24] = p.a; tb[25] = p.b; tb[26] = p.c; tb[27] = p.d;
    }
    __syncthreads();
    M2 m = m_identity();
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (lane & (1 << k)) m = mm(ps[k], m);
    double *ml = tb + 28 + 4 * lane;
    ml[0] = m.a; ml[1] = m.b; ml[2] = m.c; ml[3] = m.d;
    if (lane == 0) {
        // first rows of A^j: what a carried state z contributes to the output of the j-th frame after it, y_h[j] =
        // (A^j z).x (the sine-source variant adds it to the zero-state outputs it kept from pass 1)
        M2 q = m_identity();
        const M2 a1m{-coef[inst * 5 + 3], 1.0, -coef[inst * 5 + 4], 0.0};
        for (int j = 0; j < kBqT; ++j) {
            tb[kBqRowsAt + 2 * j] = q.a;
            tb[kBqRowsAt + 2 * j + 1] = q.b;
            q = mm(a1m, q);
        }
    }
}

// SINE: the input is a pure SinePE (sine_pe.py:159-175) generated in registers instead of read from HBM: the chain
// BiquadPE(SinePE) then moves 4 B per frame (its output) in one launch.  A thread's first frame is evaluated exactly
// as k_sine evaluates it (phase0 + w * (n / sr), pgx_sincos_bounded); its other 15 frames turn that (sin, cos) pair
// by the fixed angle w / sr (two multiplies and two fused multiply-adds per frame, error ~1e-16 per step).  The
// reference's own phase carries ~ulp(phase) of rounding noise per sample; the rotated samples sit inside it.
struct SbSine {
    double w, amp, phase0, sr, inv_sr, cos_d, sin_d;
    double two_cos_d;          // 2 cos(w / sr) for the three-term recurrence, or 0: rotate (very low frequencies)
    double tile_cos, tile_sin; // cos / sin of a tile's advance, BLOCK * 16 frames of w / sr (the angle reduced on the host)
    int64_t start;
    double *state_backup;      // receives the carried state on entry (a look-ahead window's snapshot), or nullptr
};

#ifndef PGX_SB_SINE_WAVES
#define PGX_SB_SINE_WAVES 3        // waves per SIMD the sine-source variant is compiled for: 166 VGPRs, no spill (4: 128 + 28 B of scratch per lane, 6 MB of extra HBM traffic per 33 M frames and 5 % slower)
#endif
// BLOCK: threads per workgroup -- 512 (a tile = two halves), or 256 for the sine-source variant (a tile = one half: at its
// 166 VGPRs a CU holds one 8-wave workgroup, whose single barrier per tile then idles the whole CU, or three 4-wave ones)
template <bool MONO, bool STAGED, bool SINE = false, int BLOCK = kSbBlock>
__global__ void __launch_bounds__(BLOCK, MONO ? (SINE ? PGX_SB_SINE_WAVES : 4) : 2)
k_biquad_settled(float *__restrict__ out, int64_t out_stride, const float *__restrict__ in, int64_t in_stride,
                 int64_t n, int channels_arg, const double *__restrict__ coef, const double *__restrict__ tables,
                 double *state, int seg, int head, int tail, int warm, int groups, SbSine sine = SbSine{}) {
    constexpr int kTileHalves = BLOCK * kBqT / kSbHalf;         // halves a tile covers: 2, or 1
    __shared__ SbShared sh;
    __shared__ __attribute__((aligned(16))) float stage_lds[STAGED ? (BLOCK / 64) * kStageWords : 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int channels = MONO ? 1 : channels_arg;
    const int chain = blockIdx.y;
    const int inst = chain / channels, ch = MONO ? 0 : chain - inst * channels;
    // Workgroups are dealt to the 8 XCDs round-robin and each XCD has its own L2.  While the warm-up is
    // a sizeable part of a segment, give every XCD one contiguous run of segments, so that a segment's
    // warm-up frames are its left neighbour's L2 lines (measured: 1M frames fetch 4.3 MB instead of 8.2 MB).
    // Long segments keep the round-robin order (the re-read is ~3% there and it streams ~10% faster).
    const int per_xcd = gridDim.x >> 3;                        // gridDim.x is a multiple of 8
    const int g = seg <= 8 ? (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3) : blockIdx.x;
    if (g >= groups) return;
    const float *ib = in + (int64_t)inst * in_stride;
    float *ob = out + (int64_t)inst * out_stride;
    float *wlds = stage_lds + (STAGED ? wave * kStageWords : 0);
    // STAGED (mono only): a wave whose 1024 frames are all inside the block and 16-byte aligned moves them
    // with coalesced accesses; any other wave takes the per-lane path.  `xn_staged` says which layout xn has.
    const bool io_aligned = STAGED && (SINE || aligned16(ib)) && aligned16(ob);
    bool xn_staged = false;
    const int64_t halves = (n + kSbHalf - 1) / kSbHalf;
    int64_t tail_start = halves - tail;
    if (tail_start < head) tail_start = head;

    // the ranges of this workgroup, in halves: [hb0, he0) and, for workgroup 0 only, [hb1, he1)
    int64_t hb = g == 0 ? 0 : head + (int64_t)(g - 1) * seg;
    int64_t he = g == 0 ? (head < halves ? head : halves) : (hb + seg < tail_start ? hb + seg : tail_start);
    int64_t h = hb == 0 ? 0 : hb - warm;
    int64_t emit_to = he * kSbHalf < n ? he * kSbHalf : n;

    // first tile's frames are requested before anything else so that their latency covers the table loads
    float xn[kBqT];
    int64_t anchor_tile = -(int64_t)1 << 40;                   // SINE: the tile the anchor (sin, cos) below belongs to
    double anchor_s = 0.0, anchor_c = 1.0;
    auto request = [&](int64_t hh) {
        const int64_t w0 = hh * kSbHalf + (int64_t)(tid - lane) * kBqT;      // first frame of this wave
        const int64_t f0 = w0 + lane * kBqT;
        if (SINE) {
            xn_staged = false;
            // The thread's first frame: k_sine's evaluation for the first tile of a run of consecutive tiles, that pair
            // turned by a tile's advance for every further one (4 operations instead of the division and the sincos, ~35;
            // a workgroup's run is a dozen tiles: ~1e-15).
            double sn, cs;
            if (PGX_HOT(hh == anchor_tile + kTileHalves)) {
                sn = __builtin_fma(anchor_s, sine.tile_cos, anchor_c * sine.tile_sin);
                cs = __builtin_fma(anchor_c, sine.tile_cos, -(anchor_s * sine.tile_sin));
            } else {
                const double t = pgx::pgx_div_by((double)(sine.start + f0), sine.sr, sine.inv_sr);
                pgx::pgx_sincos_bounded(sine.phase0 + sine.w * t, sn, cs);
            }
            anchor_tile = hh;
            anchor_s = sn;
            anchor_c = cs;
            if (PGX_HOT(sine.two_cos_d != 0.0)) {
                // three-term recurrence sin(p + (j+1)d) = 2 cos(d) sin(p + jd) - sin(p + (j-1)d): ONE fused multiply-add
                // per frame instead of the four operations of the rotation (the cosine is not needed).  Its error
                // after k steps is <= k ulp / d: 15 steps, d >= 1e-3 (the host's condition) -> below 2e-12
                double s0 = sn, s1 = __builtin_fma(cs, sine.sin_d, sn * sine.cos_d);
#ifndef PGX_C2_NO_UNIT_AMP
                if (PGX_HOT(sine.amp == 1.0)) {
                    // SinePE's default amplitude (C2's): amp * s is s, bit for bit -- sixteen multiplications a tile less
                    // (a wave-uniform choice: sine.amp is a kernel argument)
                    xn[0] = (float)s0;
                    xn[1] = (float)s1;
#pragma unroll
                    for (int j = 2; j < kBqT; ++j) {
                        const double s2 = __builtin_fma(sine.two_cos_d, s1, -s0);
                        xn[j] = (float)s2;
                        s0 = s1;
                        s1 = s2;
                    }
                    return;
                }
#endif
                xn[0] = (float)(sine.amp * s0);
                xn[1] = (float)(sine.amp * s1);
#pragma unroll
                for (int j = 2; j < kBqT; ++j) {
                    const double s2 = __builtin_fma(sine.two_cos_d, s1, -s0);
                    xn[j] = (float)(sine.amp * s2);
                    s0 = s1;
                    s1 = s2;
                }
                return;
            }
#pragma unroll
            for (int j = 0; j < kBqT; ++j) {
                xn[j] = (float)(sine.amp * sn);
                const double s2 = __builtin_fma(cs, sine.sin_d, sn * sine.cos_d);
                cs = __builtin_fma(-sn, sine.sin_d, cs * sine.cos_d);
                sn = s2;
            }
            return;
        }
        xn_staged = STAGED && PGX_HOT(io_aligned && w0 + 64 * kBqT <= emit_to);
        if (xn_staged) {
            stage_fetch(ib + w0, lane, xn);
        } else if (f0 < emit_to) {
            load_frames<kBqT>(ib, f0, n, channels, ch, xn);
        } else {
#pragma unroll
            for (int j = 0; j < kBqT; ++j) xn[j] = 0.0f;
        }
    };
    if (!SINE && hb < he) request(h);

    const double b0 = coef[inst * 5 + 0], b1 = coef[inst * 5 + 1], b2 = coef[inst * 5 + 2];
    const double a1 = coef[inst * 5 + 3], a2 = coef[inst * 5 + 4];
    // uniform loads -> scalar registers
    const double *tb = tables + (int64_t)inst * kBqTableDoubles;
    M2 pstep[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pstep[k] = load_m2(tb + 4 * k);
    const M2 pwave = load_m2(tb + 24);
    // per-lane powers: carry-in of the wave -> lane, previous row(s) -> lane
    const M2 mlane = load_m2(tb + 28 + 4 * lane);
    const M2 m16 = load_m2(tb + 28 + 4 * ((lane & 15) + 1));
    const M2 m32 = load_m2(tb + 28 + 4 * ((lane & 31) + 1));
    // SINE: the first rows of A^j (pass 2) live in LDS, read as broadcasts where they are used.  As 32 uniform values in
    // scalar registers they did not fit beside the scan's matrices: the compiler parked them in the lanes of a vector
    // register and fetched them back with 64 v_readlane per tile -- a sixth of the loop's vector instructions (end of round 4)
    __shared__ __attribute__((aligned(16))) double rows_lds[SINE ? 2 * kBqT : 2];
    if (SINE) {
        if (tid < 2 * kBqT) rows_lds[tid] = tb[kBqRowsAt + tid];
        __syncthreads();
    }

    int image = 0;
#pragma nounroll
    for (int range = 0; range < 2; ++range) {
        if (range == 1) {
            if (g != 0) break;
            hb = tail_start;
            he = halves;
            if (hb >= he) break;
            h = hb - warm;
            emit_to = n;
            if (!SINE) request(h);
        }
        if (hb >= he) continue;
        V2 carry{0.0, 0.0};
        if (hb == 0) {
            carry = V2{state[chain * 2 + 0], state[chain * 2 + 1]};
            if (SINE && sine.state_backup && tid == 0) {          // workgroup 0 alone reads and writes the state
                sine.state_backup[chain * 2 + 0] = carry.x;
                sine.state_backup[chain * 2 + 1] = carry.y;
            }
        }
        const int64_t emit_from = hb * kSbHalf;

#pragma nounroll
        for (; h < he; h += kTileHalves) {
            const int64_t f0 = h * kSbHalf + (int64_t)tid * kBqT;
            float xf[kBqT];
            if (SINE) {
                request(h);                                    // generated, not fetched: nothing to have in flight
#pragma unroll
                for (int j = 0; j < kBqT; ++j) xf[j] = xn[j];
            } else {
#pragma unroll
                for (int j = 0; j < kBqT; ++j) xf[j] = xn[j];
                if (STAGED && xn_staged) stage_to_chunks(wlds, lane, xf);
                if (h + kTileHalves < he) request(h + kTileHalves);                // next tile's frames, in flight during this one
            }
            // zero-state response of the 16-frame chunk
            V2 e{0.0, 0.0};
            const double na1 = -a1, na2 = -a2;
            double yz[SINE ? kBqT : 1];                        // SINE: the zero-state outputs stay for pass 2
#pragma unroll
            for (int j = 0; j < kBqT; ++j) {
                const double x = (double)xf[j];
                const double y = __builtin_fma(b0, x, e.x);
                e.x = __builtin_fma(na1, y, __builtin_fma(b1, x, e.y));
                e.y = __builtin_fma(na2, y, b2 * x);
                if (SINE) yz[j] = y;
            }
            if (!SINE) {
#pragma unroll
                for (int j = 0; j < kBqT; ++j) asm volatile("" : "+v"(xf[j]));   // re-convert in pass 2, keep VGPRs low
            }
            // inclusive scan over the wave: Kogge-Stone inside each 16-lane row (DPP row shifts) ...
            e = mv_add_fma(pstep[0], dpp_v2<0x111, 0xf>(e), e);
            e = mv_add_fma(pstep[1], dpp_v2<0x112, 0xf>(e), e);
            e = mv_add_fma(pstep[2], dpp_v2<0x114, 0xf>(e), e);
            e = mv_add_fma(pstep[3], dpp_v2<0x118, 0xf>(e), e);
            // ... then row 0 -> 1, row 2 -> 3 (lane 15 of the previous row), then rows 0-1 -> 2, 3 (lane 31)
            e = mv_add_fma(m16, dpp_v2<0x142, 0xa>(e), e);
            e = mv_add_fma(m32, dpp_v2<0x143, 0xc>(e), e);
            V2 *tot = sh.wave_tot[image];
            image ^= 1;
            if (lane == 63) tot[wave] = e;
            __syncthreads();
            V2 cw = carry, run = carry;
#pragma unroll
            for (int w = 0; w < BLOCK / 64; ++w) {
                run = mv_add_fma(pwave, run, tot[w]);
                if (w + 1 == wave) cw = run;                   // wave-uniform pick of this wave's carry-in
            }
#ifdef PGX_SB_TWO_BARRIERS
            __syncthreads();
#endif
            carry = run;

            if (PGX_HOT(f0 >= emit_from && f0 < emit_to)) {
                const V2 ex = dpp_v2<0x138, 0xf>(e);           // previous lane's inclusive value, 0 for lane 0
                const V2 zin = mv_add_fma(mlane, cw, ex);
                V2 z = zin;
                float yf[kBqT];
                if (SINE) {
                    // the zero-state outputs of pass 1 plus what the carried state adds, (A^j zin).x: two
                    // multiply-adds per frame instead of the recurrence again (the sine chain is within the rounding
                    // noise of the reference's phase anyway; the plain filter below keeps scipy's operation order)
                    const double *rows = rows_lds;               // (LDS broadcasts: see above)
#pragma unroll
                    for (int j = 0; j < kBqT; ++j)
                        yf[j] = (float)__builtin_fma(rows[2 * j], zin.x, __builtin_fma(rows[2 * j + 1], zin.y, yz[j]));
                } else {
                // scipy lfilter DF-II-T operation order from the scanned carry-in
#pragma unroll
                for (int j = 0; j < kBqT; ++j) {
                    double x = (double)xf[j];
                    double y = z.x + b0 * x;
                    double z0 = (z.y + b1 * x) - a1 * y;
                    z.y = b2 * x - a2 * y;
                    z.x = z0;
                    yf[j] = (float)y;
                }
                }
                const int64_t w0 = f0 - lane * kBqT;
                if (STAGED && PGX_HOT(io_aligned && w0 >= emit_from && w0 + 64 * kBqT <= emit_to))
                    stage_store(wlds, ob + w0, lane, yf);
                else
                    store_frames<kBqT>(ob, f0, n, channels, ch, yf);
                if (PGX_COLD(n - 1 - f0 < kBqT)) {               // the chunk holding the last frame: new state
                    z = zin;
                    for (int j = 0; j <= (int)(n - 1 - f0); ++j) {
                        double x = (double)xf[j];
                        double y = z.x + b0 * x;
                        double z0 = (z.y + b1 * x) - a1 * y;
                        z.y = b2 * x - a2 * y;
                        z.x = z0;
                    }
                    state[chain * 2 + 0] = z.x;
                    state[chain * 2 + 1] = z.y;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Wave runs: BiquadPE(SinePE) over window-sized blocks (pgx_biquad_sine when every wave gets a long run).
// The filter forgets (settle_frames), so a wave needs no carry-in from any other wave: each wave owns a contiguous
// run of 1024-frame chunks (64 lanes x 16 frames), warms up from zero state over the `warm` chunks in front of it
// (outputs discarded) and carries its own state from chunk to chunk, A^1024 carry + e(lane 63): a readlane and four
// fused multiply-adds.  No barrier and no LDS exchange between waves, so the waves of a CU overlap freely; the grid
// is one resident round (the occupancy the runtime reports), so there is no tail round either.
// Per chunk the arithmetic is k_biquad_settled<.., SINE>'s: the same sine, zero-state pass, DPP row scan and pass 2.
// Wave 0 renders the chunks [0, head) and the tail [tail_start, chunks): it alone reads the carried state (first
// thing) and writes it (last thing).  Wave g >= 1 renders `run` chunks from head + (g-1)*run.  head >= warm.
// ------------------------------------------------------------------------------------------------
struct SbRuns {
    double w, amp, phase0, sr, inv_sr, cos_d, sin_d;
    double two_cos_d;            // 2 cos(w / sr) for the three-term recurrence, or 0: rotate (very low frequencies)
    double chunk_cos, chunk_sin; // cos / sin of a chunk's advance, 1024 frames of w / sr (the angle reduced on the host)
    int64_t start;
    double *state_backup;        // receives the carried state on entry (a look-ahead window's snapshot), or nullptr
};
constexpr int kRunChunk = 64 * kBqT;     // 1024 frames: a wave's step
constexpr int kRunBlock = 256;           // four independent waves per workgroup (they share only rows_lds)
#ifndef PGX_SB_RUNS_WAVES
#define PGX_SB_RUNS_WAVES 4              // waves per SIMD k_biquad_sine_runs is compiled for
#endif

// the 16 frames of a lane from the (sin, cos) of its first one, as k_biquad_settled<.., SINE>'s request() makes them
__device__ __forceinline__ void runs_sine16(const SbRuns &sine, double sn, double cs, float (&x)[kBqT]) {
    if (PGX_HOT(sine.two_cos_d != 0.0)) {
        double s0 = sn, s1 = __builtin_fma(cs, sine.sin_d, sn * sine.cos_d);
        if (PGX_HOT(sine.amp == 1.0)) {
            x[0] = (float)s0;
            x[1] = (float)s1;
#pragma unroll
            for (int j = 2; j < kBqT; ++j) {
                const double s2 = __builtin_fma(sine.two_cos_d, s1, -s0);
                x[j] = (float)s2;
                s0 = s1;
                s1 = s2;
            }
            return;
        }
        x[0] = (float)(sine.amp * s0);
        x[1] = (float)(sine.amp * s1);
#pragma unroll
        for (int j = 2; j < kBqT; ++j) {
            const double s2 = __builtin_fma(sine.two_cos_d, s1, -s0);
            x[j] = (float)(sine.amp * s2);
            s0 = s1;
            s1 = s2;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < kBqT; ++j) {
        x[j] = (float)(sine.amp * sn);
        const double s2 = __builtin_fma(cs, sine.sin_d, sn * sine.cos_d);
        cs = __builtin_fma(-sn, sine.sin_d, cs * sine.cos_d);
        sn = s2;
    }
}

__device__ __forceinline__ double readlane63_f64(double v) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
    return __hiloint2double(hi, lo);
}

// Experiment switches of the window kernel (PGX_EXTRA_FLAGS; tools/c2_window_phases.py builds and times them):
//   PGX_SB_RUNS_NO_STORE  the hot path's global stores compiled out: wrong output, the timing of everything else
//   PGX_SB_RUNS_STAMPS    every wave records wall_clock64() (100 MHz) at entry, with its constants ready, after its
//                         first stored chunk and at exit (pgx_biquad_sine_runs_stamps reads them)
//   PGX_SB_RUNS_PACE_SHIFT=k  the pacing thresholds at -1, +1 and +3 times tau / 2^k instead of tau / 4
#ifndef PGX_SB_RUNS_PACE_SHIFT
#define PGX_SB_RUNS_PACE_SHIFT 2
#endif
typedef unsigned int runs_v4u __attribute__((ext_vector_type(4)));

// stage_store for the runs kernel's full, aligned chunks: 16 consecutive frames per lane -> four coalesced 1 KB rows,
// stored write-through (sc1).  A plain store leaves its line dirty in the XCD's L2, and a kernel that ends with up to
// 32 MiB of dirty lines pays for their write-back at the boundary to the next launch: 3.5 us from the last wave's exit
// to the next window's first entry, 1.2 us with write-through.  A run is 4 KB x `run` chunks, a block
// 12.6 M frames and more -- far beyond the 32 MiB of L2 -- so no reader of these lines is served from L2 today and
// nothing is lost when the store drops them.  The buffer resource is based at the chunk (the same address in every
// lane), so every offset is below 4 KB whatever the size of the window.
__device__ __forceinline__ void runs_store_chunk(float *lds, float *dst, int lane, const float (&y)[kBqT]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4 *>(lds + lane * 20 + 4 * i) = make_float4(y[4 * i], y[4 * i + 1], y[4 * i + 2], y[4 * i + 3]);
    const uint64_t p = (uint64_t)dst;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, kRunChunk * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const runs_v4u r = *reinterpret_cast<const runs_v4u *>(lds + stage_slot(i, lane));
#ifdef PGX_SB_RUNS_NO_STORE
        asm volatile("" ::"v"(r));
#else
        __builtin_amdgcn_raw_buffer_store_b128(r, rsrc, lane * 16, i * 1024, 16 /* sc1 */);
#endif
    }
}

// Deadline pacing.  The SIMD issues by priority, then by age, so four resident waves of equal priority do not share it:
// the first dispatched runs at the speed of its own dependent chains, the others in the gaps it leaves, the grid leaves
// in four steps and the last quarter of a window's bytes is written by SIMDs that hold one or two latency-bound waves
// (DESIGN section 7).  A paced wave reads the 100 MHz wall clock at entry and once per chunk and sets its issue priority
// by how far it is behind `done x tau`, tau being the time per chunk the launch was given: ahead of schedule 0, on it 1,
// behind 2, behind by most of a chunk 3.  The waves of a SIMD then advance together and end together.  A priority
// changes no sample and makes no wave wait for another; who renders which chunk stays as it is.
//
// tau comes from the window before, on the device: at exit one wave in kPaceRecordEvery records (launch id << 32) | its ticks
// since entry into words[0] by atomicMax -- a newer launch's value dominates any older one, so nothing is zeroed
// between launches -- and the next launch reads the word in its prologue.  It takes it only under the id the host names
// as the previous runs-launch of the same plan; then tau = ticks x per_chunk (factor / (run + warm)), otherwise 0: no
// pacing, no clock read in the chunk loop and no change of priority.  Wave 0 leaves (id << 32) | tau in words[1] for
// pgx_biquad_sine_pacing_info.  words == nullptr (pacing switched off): the kernel reads no clock at all.
constexpr int kPaceRecordEvery = 61;     // a prime: the recording waves fall on every SIMD, CU and quarter of the dispatch
struct RunsPace {
    unsigned long long *words;
    unsigned id, prev_id;
    float per_chunk;
};

// lag: ticks behind schedule, tau: ticks per chunk; thresholds at -1/4, +1/4 and +3/4 tau.  The pacing state lives in
// vector registers (the kernel has none of the scalar ones to spare) with the same value in every lane; the level goes
// through readfirstlane, so the branches are scalar ones around an s_setprio each (it takes an immediate)
__device__ __forceinline__ void runs_pace_priority(int lag, int tau) {
    const int q = tau >> PGX_SB_RUNS_PACE_SHIFT;
    switch (__builtin_amdgcn_readfirstlane((lag >= -q) + (lag >= q) + (lag >= 3 * q))) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
    }
}

#ifdef PGX_SB_RUNS_STAMPS
constexpr int kRunStampWaves = 4096;
__device__ unsigned long long g_runs_stamps[2][kRunStampWaves][4];
#endif

__global__ void __launch_bounds__(kRunBlock, PGX_SB_RUNS_WAVES)
k_biquad_sine_runs(float *__restrict__ out, int64_t n, const double *__restrict__ coef,
                   const double *__restrict__ tables, double *state, int run, int head, int tail, int warm, int waves,
                   SbRuns sine, RunsPace pace
#ifdef PGX_SB_RUNS_STAMPS
                   , int stamp_slot
#endif
                   ) {
    __shared__ __attribute__((aligned(16))) float stage_lds[(kRunBlock / 64) * kStageWords];
    __shared__ __attribute__((aligned(16))) double rows_lds[2 * kBqT];
#ifdef PGX_SB_RUNS_STAMPS
    unsigned long long stamp[4] = {(unsigned long long)wall_clock64(), 0, 0, 0};
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *tb = tables;
    // the first rows of A^j (pass 2), read as LDS broadcasts (see k_biquad_settled): the kernel's only barrier
    if (tid < 2 * kBqT) rows_lds[tid] = tb[kBqRowsAt + tid];
    __syncthreads();
    const int g = blockIdx.x * (kRunBlock / 64) + wave;
    if (g >= waves) return;
    // pacing: the entry clock, and the previous window's word on its way together with the table loads below
    unsigned pace_t0 = 0;
    unsigned long long pace_prev = 0;
    if (pace.words) {
        pace_t0 = (unsigned)wall_clock64();
        if (pace.prev_id) pace_prev = __hip_atomic_load(pace.words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("" : "+v"(pace_t0));                          // kept in a vector register, as all pacing state is

    float *wlds = stage_lds + wave * kStageWords;
    const bool io_aligned = aligned16(out);
    const int64_t chunks = (n + kRunChunk - 1) / kRunChunk;
    int64_t tail_start = chunks - tail;
    if (tail_start < head) tail_start = head;

    const double b0 = coef[0], b1 = coef[1], b2 = coef[2], a1 = coef[3], a2 = coef[4];
    M2 pstep[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pstep[k] = load_m2(tb + 4 * k);
    const M2 pwave = load_m2(tb + 24);
    const M2 mlane = load_m2(tb + 28 + 4 * lane);
    const M2 m16 = load_m2(tb + 28 + 4 * ((lane & 15) + 1));
    const M2 m32 = load_m2(tb + 28 + 4 * ((lane & 31) + 1));
#ifdef PGX_SB_RUNS_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::"v"(mlane.a), "v"(m16.a), "v"(m32.a), "v"(pwave.a), "v"(b0) : "memory");
    stamp[1] = wall_clock64();
#endif
    // ticks per chunk, or 0: not paced (no history under the id the host expects).  Below 2^24, 0.17 s per chunk
    int pace_tau = 0;
    if (pace.prev_id && (unsigned)(pace_prev >> 32) == pace.prev_id)
        pace_tau = (int)fminf((float)(unsigned)pace_prev * pace.per_chunk, 16777216.0f);
    unsigned pace_due = pace_t0;                               // the clock at which the current chunk is due to begin
    asm volatile("" : "+v"(pace_tau), "+v"(pace_due));

    // renders the chunks [cb, ce) after `warm` chunks of warm-up (from the carried state at chunk 0).  Called once per
    // range, not from a loop over the ranges: the sine's constants are then not hoisted into registers for all of it
    auto render = [&](const int64_t cb, const int64_t ce) {
        int64_t c = cb == 0 ? 0 : cb - warm;
        V2 carry{0.0, 0.0};
        if (cb == 0) {
            carry = V2{state[0], state[1]};
            if (sine.state_backup && lane == 0) {              // wave 0 alone reads and writes the state
                sine.state_backup[0] = carry.x;
                sine.state_backup[1] = carry.y;
            }
        }
        // the lane's first frame: k_sine's evaluation for the first chunk, then turned by a chunk's advance
        double sn, cs;
        {
            const double t = pgx::pgx_div_by((double)(sine.start + c * kRunChunk + lane * kBqT), sine.sr, sine.inv_sr);
            pgx::pgx_sincos_bounded(sine.phase0 + sine.w * t, sn, cs);
        }
#pragma nounroll
        for (; c < ce; ++c) {
            // the clock is read here, where no LDS access is outstanding: it returns on the counter LDS reads return
            // on, and a wait for it further down would hold the pass-2 row reads back
            if (__builtin_amdgcn_readfirstlane(pace_tau)) {
                runs_pace_priority((int)((unsigned)wall_clock64() - pace_due), pace_tau);
                pace_due += (unsigned)pace_tau;
            }
            float xf[kBqT];
            runs_sine16(sine, sn, cs, xf);
            // zero-state response of the lane's 16 frames
            V2 e{0.0, 0.0};
            const double na1 = -a1, na2 = -a2;
            double yz[kBqT];
#pragma unroll
            for (int j = 0; j < kBqT; ++j) {
                const double x = (double)xf[j];
                const double y = __builtin_fma(b0, x, e.x);
                e.x = __builtin_fma(na1, y, __builtin_fma(b1, x, e.y));
                e.y = __builtin_fma(na2, y, b2 * x);
                yz[j] = y;
            }
            // inclusive scan over the wave (k_biquad_settled's)
            e = mv_add_fma(pstep[0], dpp_v2<0x111, 0xf>(e), e);
            e = mv_add_fma(pstep[1], dpp_v2<0x112, 0xf>(e), e);
            e = mv_add_fma(pstep[2], dpp_v2<0x114, 0xf>(e), e);
            e = mv_add_fma(pstep[3], dpp_v2<0x118, 0xf>(e), e);
            e = mv_add_fma(m16, dpp_v2<0x142, 0xa>(e), e);
            e = mv_add_fma(m32, dpp_v2<0x143, 0xc>(e), e);

            const int64_t w0 = c * kRunChunk;
            if (PGX_HOT(c >= cb)) {
                const int64_t f0 = w0 + lane * kBqT;
                const V2 ex = dpp_v2<0x138, 0xf>(e);           // previous lane's inclusive value, 0 for lane 0
                const V2 zin = mv_add_fma(mlane, carry, ex);
                float yf[kBqT];
                const double *rows = rows_lds;
#pragma unroll
                for (int j = 0; j < kBqT; ++j)
                    yf[j] = (float)__builtin_fma(rows[2 * j], zin.x, __builtin_fma(rows[2 * j + 1], zin.y, yz[j]));
                if (PGX_HOT(io_aligned && w0 + kRunChunk <= n))
                    runs_store_chunk(wlds, out + w0, lane, yf);
                else
                    store_frames<kBqT>(out, f0, n, 1, 0, yf);
#ifdef PGX_SB_RUNS_STAMPS
                if (!stamp[2]) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    stamp[2] = wall_clock64();
                }
#endif
                if (PGX_COLD(f0 <= n - 1 && n - 1 - f0 < kBqT)) {  // the lane holding the last frame: new state
                    // its frames made again (bit for bit the same), rather than kept in 16 registers for this branch
                    double rs = sn, rc = cs;
                    asm volatile("" : "+v"(rs), "+v"(rc));
                    runs_sine16(sine, rs, rc, xf);
                    V2 z = zin;
                    for (int j = 0; j <= (int)(n - 1 - f0); ++j) {
                        double x = (double)xf[j];
                        double y = z.x + b0 * x;
                        double z0 = (z.y + b1 * x) - a1 * y;
                        z.y = b2 * x - a2 * y;
                        z.x = z0;
                    }
                    state[0] = z.x;
                    state[1] = z.y;
                }
            }
            // the wave's state after this chunk: what the state in front of it leaves, plus lane 63's inclusive value
            carry = mv_add_fma(pwave, carry, V2{readlane63_f64(e.x), readlane63_f64(e.y)});
            const double s2 = __builtin_fma(sn, sine.chunk_cos, cs * sine.chunk_sin);
            cs = __builtin_fma(cs, sine.chunk_cos, -(sn * sine.chunk_sin));
            sn = s2;
        }
    };
    // the chunks of this wave, and for wave 0 the tail
    // (two copies of the loop, not three: each keeps its xf[] in registers only while the three do not outgrow the
    // compiler's budget for such arrays, and with the pacing code in the loop a third copy's went to scratch)
    {
        const int64_t cb = g == 0 ? 0 : head + (int64_t)(g - 1) * run;
        const int64_t ce = g == 0 ? (head < chunks ? head : chunks) : (cb + run < tail_start ? cb + run : tail_start);
        render(cb, ce);
        if (g == 0) render(tail_start, chunks);
    }
#ifdef PGX_SB_RUNS_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp[3] = wall_clock64();
    if (lane == 0 && g < kRunStampWaves)
        for (int k = 0; k < 4; ++k) g_runs_stamps[stamp_slot & 1][g][k] = stamp[k];
#endif
    // this wave's ticks for the next window's tau: fire and forget, nothing waits for the atomic.  One wave in
    // kPaceRecordEvery records: atomics on one address are served one after the other, about 11 ns each, and with every
    // wave of a 16 M-frame window recording the kernel ended 36 us later (52.8 us against 16.2 us)
    if (pace.words && g % kPaceRecordEvery == 0) {
        const unsigned long long ticks = (unsigned)wall_clock64() - pace_t0;
        if (lane == 0) {
            atomicMax(pace.words, ((unsigned long long)pace.id << 32) | ticks);
            if (g == 0) pace.words[1] = ((unsigned long long)pace.id << 32) | (unsigned)pace_tau;
        }
    }
}

struct BqPlan {
    int seg_tiles;
    int nseg;
};

struct BqSettledPlan {
    bool ok;
    int seg, head, tail, warm, groups;        // in 4096-frame halves
};

BqSettledPlan biquad_settled_plan(int batch, int64_t n, int channels, int64_t settle_frames, bool have_tables,
                                  int workgroups = 512) {
    BqSettledPlan p{};
    if (!have_tables) return p;
    const int64_t halves = pgx::ceil_div(n, kSbHalf);
    const int64_t chains = (int64_t)batch * channels;
    const int64_t warm = pgx::ceil_div(settle_frames, kSbHalf);
    if (settle_frames > 0 && warm <= kSbMaxWarm) {
        int64_t want = workgroups / chains;                    // 512: two resident workgroups per CU, one round
        if (want < 1) want = 1;
        int64_t seg = pgx::ceil_div(halves, want);
        if (seg < warm) seg = warm;                            // warm-up never exceeds the rendered part
        const int64_t head = seg / 2 > warm ? seg / 2 : warm;  // workgroup 0: head + tail ~ one segment
        const int64_t tail = seg - head > 1 ? seg - head : 1;
        if (halves > head + tail) {
            p.ok = true;
            p.seg = (int)seg;
            p.head = (int)head;
            p.tail = (int)tail;
            p.warm = (int)warm;
            p.groups = 1 + (int)pgx::ceil_div(halves - head - tail, seg);
            return p;
        }
    }
    // One workgroup per chain over the whole block: nothing is assumed (the carried state is read, no
    // warm-up), this is just the faster tile engine.  Worth it when the chains alone fill the machine
    // (voice banks) or the block is a tile or two; long lone chains keep the segment-parallel exact pair.
    if (chains >= 64 || halves <= 2) {
        p.ok = true;
        p.seg = (int)halves;
        p.head = (int)halves;
        p.tail = 0;
        p.warm = 0;
        p.groups = 1;
    }
    return p;
}

BqPlan biquad_plan(int batch, int64_t n, int channels) {
    int64_t tiles = pgx::ceil_div(n, kBqTile);
    int64_t chains = (int64_t)batch * channels;
    int64_t want = 512 / chains;                  // aim for ~512 workgroups (2 per CU) in flight
    if (want < 1) want = 1;
    if (want > kBqMaxSeg) want = kBqMaxSeg;
    if (want > tiles) want = tiles;
    BqPlan p;
    p.seg_tiles = (int)pgx::ceil_div(tiles, want);
    p.nseg = (int)pgx::ceil_div(tiles, p.seg_tiles);
    return p;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

size_t pgx_biquad_workspace_bytes(int batch, int64_t n, int channels, int64_t settle_frames) {
    if (batch <= 0 || n <= 0 || channels <= 0) return 0;
    // a caller that passes settle_frames > 0 also passes tables; without them the exact pair may run
    if (settle_frames > 0 && biquad_settled_plan(batch, n, channels, settle_frames, true).ok) return 0;
    BqPlan p = biquad_plan(batch, n, channels);
    if (p.nseg <= 1) return 0;
    size_t chains = (size_t)batch * channels;
    return (chains * 2 + chains * (size_t)p.nseg * 2) * sizeof(double);
}

size_t pgx_biquad_table_doubles(void) { return kBqTableDoubles; }

int pgx_biquad_tables(double *tables, const double *coef, int batch) {
    PGX_REQUIRE_INIT();
    if (batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(tables && coef, "pgx_biquad_tables: bad argument");
    hipLaunchKernelGGL(k_biquad_tables, dim3(batch), dim3(64), 0, pgx::stream(), tables, coef);
    PGX_LAUNCH_CHECK("k_biquad_tables");
    return PGX_OK;
}

int pgx_biquad_const(float *out, int64_t out_stride, const float *in, int64_t in_stride, int batch, int64_t n,
                     int channels, const double *coef, const double *tables, int64_t settle_frames, double *state,
                     void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && coef && state && channels >= 1, "pgx_biquad_const: bad argument");
    PGX_CHECK_ARG(batch == 1 || (out_stride >= n * channels && in_stride >= n * channels),
                  "pgx_biquad_const: instance stride too small");
    PGX_CHECK_ARG((int64_t)batch * channels <= 65535, "pgx_biquad_const: too many chains");
    int chains = batch * channels;
    const BqSettledPlan sp = biquad_settled_plan(batch, n, channels, settle_frames, tables != nullptr);
    if (sp.ok) {
        const dim3 grid(sp.groups == 1 ? 1 : (sp.groups + 7) / 8 * 8, chains);
        if (channels == 1)
            hipLaunchKernelGGL((k_biquad_settled<true, true>), grid, dim3(kSbBlock), 0, pgx::stream(), out,
                               out_stride, in, in_stride, n, channels, coef, tables, state, sp.seg, sp.head,
                               sp.tail, sp.warm, sp.groups);
        else
            hipLaunchKernelGGL((k_biquad_settled<false, false>), grid, dim3(kSbBlock), 0, pgx::stream(), out,
                               out_stride, in, in_stride, n, channels, coef, tables, state, sp.seg, sp.head,
                               sp.tail, sp.warm, sp.groups);
        PGX_LAUNCH_CHECK("k_biquad_settled");
        return PGX_OK;
    }
    BqPlan p = biquad_plan(batch, n, channels);
    dim3 grid(p.nseg, chains);
    if (p.nseg > 1) {
        PGX_CHECK_ARG(workspace != nullptr, "pgx_biquad_const: workspace required for this size");
        double *snap = (double *)workspace;
        double *agg = snap + (size_t)chains * 2;
        hipLaunchKernelGGL(k_biquad_const<0>, grid, dim3(kBlock), 0, pgx::stream(), out, out_stride, in,
                           in_stride, n, channels, coef, state, (const double *)snap, agg, p.seg_tiles, p.nseg);
        PGX_LAUNCH_CHECK("k_biquad_const<reduce>");
        hipLaunchKernelGGL(k_biquad_const<1>, grid, dim3(kBlock), 0, pgx::stream(), out, out_stride, in,
                           in_stride, n, channels, coef, state, (const double *)snap, agg, p.seg_tiles, p.nseg);
        PGX_LAUNCH_CHECK("k_biquad_const<apply>");
    } else {
        hipLaunchKernelGGL(k_biquad_const<1>, grid, dim3(kBlock), 0, pgx::stream(), out, out_stride, in,
                           in_stride, n, channels, coef, state, (const double *)nullptr, (double *)nullptr,
                           p.seg_tiles, p.nseg);
        PGX_LAUNCH_CHECK("k_biquad_const");
    }
    return PGX_OK;
}

// The sine-source variant: 4-wave workgroups, three per CU (PGX_SB_SINE_BLOCK=512: the 8-wave form, one per CU --
// experiments)
static int sine_block() {
    static const int block = getenv("PGX_SB_SINE_BLOCK") ? atoi(getenv("PGX_SB_SINE_BLOCK")) : 256;
    return block == 512 ? 512 : 256;
}
static BqSettledPlan biquad_sine_plan(int64_t n, int64_t settle_frames) {
    static const int want = getenv("PGX_SB_SINE_WGS") ? atoi(getenv("PGX_SB_SINE_WGS")) : (sine_block() == 256 ? 1024 : 512);
    return biquad_settled_plan(1, n, 1, settle_frames, true, want);
}

int pgx_biquad_sine_supported(int64_t n, int64_t settle_frames) {
    return (n > 0 && biquad_sine_plan(n, settle_frames).ok) ? 1 : 0;
}

// Wave runs (k_biquad_sine_runs) for window-sized blocks.  The grid is one resident round: the occupancy the runtime
// reports for the kernel times the CUs, taken once.
constexpr int64_t kRunMinChunks = 4;     // a wave's run below this: the current kernel (measured faster from 16 M frames on)
static int runs_resident_waves() {
    static const int waves = [] {
        int blocks = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_biquad_sine_runs, kRunBlock, 0) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, pgx::device_index()) != hipSuccess)
            return 0;
        return blocks * cus * (kRunBlock / 64);
    }();
    return waves;
}
// The shortest run (in chunks) the wave runs take: PGX_SB_SINE_RUNS=0 forces the current kernel (A/B runs), another
// value replaces kRunMinChunks; pgx_biquad_sine_set_runs overrides it
static int &runs_min_chunks() {
    static int v = getenv("PGX_SB_SINE_RUNS") ? atoi(getenv("PGX_SB_SINE_RUNS")) : (int)kRunMinChunks;
    return v;
}

struct RunsPlan {
    bool ok;
    int run, head, tail, warm, waves;    // in 1024-frame chunks; waves used
};
static RunsPlan biquad_sine_runs_plan(int64_t n, int64_t settle_frames) {
    RunsPlan p{};
    const int resident = runs_resident_waves();
    const int min_chunks = runs_min_chunks();
    if (min_chunks <= 0 || resident <= 0 || settle_frames <= 0) return p;
    const int64_t chunks = pgx::ceil_div(n, (int64_t)kRunChunk);
    const int64_t warm = pgx::ceil_div(settle_frames, (int64_t)kRunChunk);
    const int64_t run = pgx::ceil_div(chunks, (int64_t)resident);
    if (run < min_chunks || run < 4 * warm) return p;       // short runs, or a warm-up above 1/4 of the work
    const int64_t head = run / 2 > warm ? run / 2 : warm;    // wave 0: head + tail = one run
    const int64_t tail = run - head > 1 ? run - head : 1;
    if (chunks <= head + tail) return p;
    p.ok = true;
    p.run = (int)run;
    p.head = (int)head;
    p.tail = (int)tail;
    p.warm = (int)warm;
    p.waves = 1 + (int)pgx::ceil_div(chunks - head - tail, run);
    return p;
}

int pgx_biquad_sine_set_runs(int min_chunks) {
    const int was = runs_min_chunks();
    runs_min_chunks() = min_chunks < 0 ? (int)kRunMinChunks : min_chunks;
    return was;
}

int pgx_biquad_sine_runs_plan(int64_t n, int64_t settle_frames, int out[5]) {
    if (!out || n <= 0 || !pgx::initialised()) return 0;
    const RunsPlan rp = biquad_sine_runs_plan(n, settle_frames);
    if (!rp.ok || !biquad_sine_plan(n, settle_frames).ok) return 0;
    out[0] = rp.run;
    out[1] = rp.head;
    out[2] = rp.tail;
    out[3] = rp.warm;
    out[4] = rp.waves;
    return 1;
}

// Deadline pacing of the wave runs (RunsPace).  PGX_SB_SINE_PACING=0 / 1 replaces the default,
// pgx_biquad_sine_set_pacing overrides it; PGX_SB_SINE_PACE_FACTOR replaces kPaceFactor (experiments).
constexpr int kPaceDefault = 1;
constexpr float kPaceFactor = 1.0f;      // tau = the previous window's longest wave / (run + warm) x this
static int &runs_pacing() {
    static int v = getenv("PGX_SB_SINE_PACING") ? (atoi(getenv("PGX_SB_SINE_PACING")) != 0) : kPaceDefault;
    return v;
}
static float pace_factor() {
    static const float f = getenv("PGX_SB_SINE_PACE_FACTOR") ? (float)atof(getenv("PGX_SB_SINE_PACE_FACTOR")) : kPaceFactor;
    return f;
}
// the two device words of RunsPace (made on first use, released by pgx_shutdown), the id of the last runs-launch and
// its plan: the next launch is paced by its duration only if it has the same plan and follows it directly
static struct {
    unsigned long long *words = nullptr;
    unsigned next_id = 1, last_id = 0;
    int run = 0, warm = 0, waves = 0;
} g_pace;

int pgx_biquad_sine_set_pacing(int mode) {
    const int was = runs_pacing();
    runs_pacing() = mode < 0 ? kPaceDefault : (mode != 0);
    return was;
}

int pgx_biquad_sine_pacing_info(int64_t out[3]) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(out, "pgx_biquad_sine_pacing_info: null output");
    out[0] = out[1] = out[2] = 0;
    if (!g_pace.words) return PGX_OK;
    unsigned long long w[2];
    PGX_HIP(hipMemcpyAsync(w, g_pace.words, sizeof(w), hipMemcpyDeviceToHost, pgx::stream()));
    PGX_HIP(hipStreamSynchronize(pgx::stream()));
    out[0] = (int64_t)(w[0] >> 32);
    out[1] = (int64_t)(w[0] & 0xffffffffull);
    out[2] = (w[1] >> 32) == (w[0] >> 32) ? (int64_t)(w[1] & 0xffffffffull) : 0;
    return PGX_OK;
}

#ifdef PGX_SB_RUNS_STAMPS
static int g_runs_stamp_launch = 0;
// the stamps of the last two window launches, [2][4096][4] ticks of 10 ns; slot = launch number & 1.  Returns the
// number of launches so far (after a device synchronise).
extern "C" int pgx_biquad_sine_runs_stamps(unsigned long long *host_out) {
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_runs_stamps), sizeof(unsigned long long) * 2 * kRunStampWaves * 4) != hipSuccess)
        return -1;
    return g_runs_stamp_launch;
}
#endif

int pgx_biquad_sine(float *out, int64_t start, int64_t n, double sample_rate, double w, double amp, double phase0,
                    const double *coef, const double *tables, int64_t settle_frames, double *state,
                    double *state_backup) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && coef && tables && state && sample_rate > 0, "pgx_biquad_sine: bad argument");
    const int block = sine_block();
    const BqSettledPlan sp = biquad_sine_plan(n, settle_frames);
    PGX_CHECK_ARG(sp.ok, "pgx_biquad_sine: block too short for the single-launch plan (pgx_biquad_sine_supported)");
    // the largest phase of the render has to stay in the bounded sine's range
    const double far = fabs(phase0) + fabs(w) * ((double)(llabs(start) + n) / sample_rate);
    PGX_CHECK_ARG(far < pgx::kSinFastRange, "pgx_biquad_sine: phase beyond the fast sine range");
    // the tone's constants (five long-double sines and cosines) are made once per (w, sample rate): a stream of windows
    // asks for the same tone every time, and they were 1 us of every window opening's host time
    static SbSine cached;
    static bool have = false;
    if (!have || cached.w != w || cached.sr != sample_rate) {
        SbSine c;
        c.w = w;
        c.sr = sample_rate;
        c.inv_sr = 1.0 / sample_rate;
        const long double d = (long double)w / (long double)sample_rate;
        c.cos_d = (double)cosl(d);
        c.sin_d = (double)sinl(d);
        c.two_cos_d = (fabsl(sinl(d)) >= 1e-3L) ? (double)(2.0L * cosl(d)) : 0.0;
        // a tile's advance, block * 16 frames: the angle reduced in long double before the sine and cosine are taken
        const long double turn = 6.283185307179586476925286766559L;
        long double a = d * (long double)(sine_block() * kBqT);
        a -= turn * floorl(a / turn);
        c.tile_cos = (double)cosl(a);
        c.tile_sin = (double)sinl(a);
        cached = c;
        have = true;
    }
    const RunsPlan rp = biquad_sine_runs_plan(n, settle_frames);
    if (rp.ok) {
        static SbRuns runs_cached;
        static bool runs_have = false;
        if (!runs_have || runs_cached.w != w || runs_cached.sr != sample_rate) {
            SbRuns c;
            c.w = cached.w;
            c.sr = cached.sr;
            c.inv_sr = cached.inv_sr;
            c.cos_d = cached.cos_d;
            c.sin_d = cached.sin_d;
            c.two_cos_d = cached.two_cos_d;
            // a chunk's advance, 1024 frames: the angle reduced in long double before the sine and cosine are taken
            const long double turn = 6.283185307179586476925286766559L;
            long double a = (long double)w / (long double)sample_rate * (long double)kRunChunk;
            a -= turn * floorl(a / turn);
            c.chunk_cos = (double)cosl(a);
            c.chunk_sin = (double)sinl(a);
            runs_cached = c;
            runs_have = true;
        }
        SbRuns sine = runs_cached;
        sine.amp = amp;
        sine.phase0 = phase0;
        sine.start = start;
        sine.state_backup = state_backup;
        const int groups = (rp.waves + kRunBlock / 64 - 1) / (kRunBlock / 64);
        RunsPace pace{nullptr, 0, 0, 0.0f};
        if (runs_pacing()) {
            if (!g_pace.words) {                               // first use: two zeroed words, in stream order
                void *p = nullptr;
                PGX_HIP(hipMalloc(&p, 2 * sizeof(unsigned long long)));
                g_pace.words = (unsigned long long *)p;
                PGX_HIP(hipMemsetAsync(p, 0, 2 * sizeof(unsigned long long), pgx::stream()));
            }
            pace.words = g_pace.words;
            if (g_pace.next_id == 0) {                         // the ids wrap: start over, or no new id would dominate
                PGX_HIP(hipMemsetAsync(g_pace.words, 0, 2 * sizeof(unsigned long long), pgx::stream()));
                g_pace.next_id = 1;
                g_pace.last_id = 0;
            }
            pace.id = g_pace.next_id++;
            if (g_pace.last_id && g_pace.run == rp.run && g_pace.warm == rp.warm && g_pace.waves == rp.waves)
                pace.prev_id = g_pace.last_id;
            pace.per_chunk = pace_factor() / (float)(rp.run + rp.warm);
            g_pace.last_id = pace.id;
            g_pace.run = rp.run;
            g_pace.warm = rp.warm;
            g_pace.waves = rp.waves;
        } else {
            g_pace.last_id = 0;
        }
#ifdef PGX_SB_RUNS_STAMPS
        hipLaunchKernelGGL(k_biquad_sine_runs, dim3(groups), dim3(kRunBlock), 0, pgx::stream(), out, n, coef, tables,
                           state, rp.run, rp.head, rp.tail, rp.warm, rp.waves, sine, pace, g_runs_stamp_launch++);
#else
        hipLaunchKernelGGL(k_biquad_sine_runs, dim3(groups), dim3(kRunBlock), 0, pgx::stream(), out, n, coef, tables,
                           state, rp.run, rp.head, rp.tail, rp.warm, rp.waves, sine, pace);
#endif
        PGX_LAUNCH_CHECK("k_biquad_sine_runs");
        return PGX_OK;
    }
    g_pace.last_id = 0;                                        // a render between two windows: the next one runs unpaced
    SbSine sine = cached;
    sine.amp = amp;
    sine.phase0 = phase0;
    sine.start = start;
    sine.state_backup = state_backup;
    const dim3 grid(sp.groups == 1 ? 1 : (sp.groups + 7) / 8 * 8, 1);
    if (block == 256)
        hipLaunchKernelGGL((k_biquad_settled<true, true, true, 256>), grid, dim3(256), 0, pgx::stream(), out,
                           (int64_t)0, (const float *)nullptr, (int64_t)0, n, 1, coef, tables, state, sp.seg, sp.head,
                           sp.tail, sp.warm, sp.groups, sine);
    else
        hipLaunchKernelGGL((k_biquad_settled<true, true, true>), grid, dim3(kSbBlock), 0, pgx::stream(), out,
                           (int64_t)0, (const float *)nullptr, (int64_t)0, n, 1, coef, tables, state, sp.seg, sp.head,
                           sp.tail, sp.warm, sp.groups, sine);
    PGX_LAUNCH_CHECK("k_biquad_settled<sine>");
    return PGX_OK;
}

}  // extern "C"

namespace pgx {

// pgx_shutdown, with the streams drained: the pacing words go, and with them the history a next pgx_init could not use
void biquad_sine_pacing_release() {
    if (g_pace.words) (void)hipFree(g_pace.words);
    g_pace.words = nullptr;
    g_pace.last_id = 0;
}

}  // namespace pgx
