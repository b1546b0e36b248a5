// pgx_noise.hip -- NoisePE (noise_pe.py:28-171): white, pink and brown noise drawn on the device.
//
// The reference draws np.random.default_rng(seed).uniform(-1, 1, n).astype(float32).  numpy's PCG64 is a 128-bit LCG
//     s <- M * s + inc   (M = 0x2360ED051FC65DA44385DF649FCCF645, inc odd, per seed; stepped BEFORE the output is taken)
// with the XSL-RR output  u64 = rotr64(hi ^ lo, hi >> 58), and uniform(-1, 1) is  -1.0 + 2.0 * ((u64 >> 11) * 2^-53)
// in float64.  n steps of the LCG are  s -> M^n * s + inc * S_n,  S_n = 1 + M + ... + M^(n-1), and neither M^n nor S_n
// depends on the seed: the table kSkip holds (M^(2^k), S_(2^k)) for k = 0..63 (made at compile time from M alone), so
// a lane reaches draw number d of a stream with one 128-bit multiply-add pair per set bit of d.  Sample i of a render
// is a pure function of (state, inc, draws consumed before the render + i).
//
// k_noise_white: lane t owns runs of kWhiteRun consecutive samples: one skip-ahead to its first run, one LCG step per
//     sample, one table jump (2^11 draws) from a run to the lane's run in the next tile.
// k_noise_pink (Paul Kellet's filter, noise_pe.py:115-134) and k_noise_brown (:136-149): a workgroup per instance, a
//     tile loop inside.  The whole workgroup draws a tile and forms the elementwise products in LDS; the float32
//     recurrences are then stepped literally, eight samples in registers at a time with the next eight already
//     requested from LDS -- six lanes for the six independent pink taps (two dependent float32
//     operations per sample), one lane for the brown level with its two rail tests -- and the whole workgroup forms the
//     output sum, applies the range and writes the tile.  Re-associating either recurrence changes the float32 bits
//     (DESIGN.md), so they are not scanned.
// Under numpy >= 2 every operation of those loops and of _scale_output (:102-109) is a float32 operation; with
// -ffp-contract=off each `*` and `+` below is one rounding, in the reference's order.  Constants are the float64
// literals of the reference rounded to float32, as numpy rounds a Python float that meets a float32.

#include "pgx_pcg.h"

namespace {

using pgx::kPcgMult;
using pgx::make128;
using pgx::SkipTable;
using pgx::u128;

// the library's one skip table (pgx_pcg.h); other translation units read it through pgx::pcg_skip_table_device()
constexpr SkipTable kSkipHost = pgx::make_skip_table();
__constant__ SkipTable kSkip = pgx::make_skip_table();

constexpr int kLanes = 256;
constexpr int kWhiteRun = 8;                          // consecutive samples per lane and tile
constexpr int kWhiteTileLog2 = 11;
constexpr int kWhiteTile = 1 << kWhiteTileLog2;       // kLanes * kWhiteRun
constexpr int kWhiteMaxGrid = 2048;                   // workgroups per instance at most
constexpr int kSeqRun = 4;
constexpr int kSeqTileLog2 = 10;
constexpr int kSeqTile = 1 << kSeqTileLog2;           // kLanes * kSeqRun
constexpr int kSeqGroup = 8;                          // samples of a stepped chain held in registers at a time
static_assert(kWhiteTile == kLanes * kWhiteRun && kSeqTile == kLanes * kSeqRun, "tile geometry");

// `d` LCG steps from s
__device__ __forceinline__ u128 pcg_skip(u128 s, u128 inc, uint64_t d) { return pgx::pcg_skip_with(kSkip, s, inc, d); }

// the draw that numpy takes from state s (already stepped): float32(-1.0 + 2.0 * ((xsl_rr(s) >> 11) * 2^-53))
__device__ __forceinline__ float pcg_draw(u128 s) {
    const double r = (double)(pgx::pcg_output(s) >> 11) * 0x1p-53;
    return (float)(-1.0 + 2.0 * r);
}

// _scale_output (:102-109): [-1, 1] -> [min_value, max_value], four float32 roundings; the default range is untouched
__device__ __forceinline__ float noise_range(float x, int scaled, float span, float min_value) {
    if (!scaled) return x;
    float v = x + 1.0f;
    v = v * 0.5f;
    v = v * span;
    return v + min_value;
}

__global__ __launch_bounds__(kLanes) void k_noise_white(float *out, int64_t out_stride, int64_t n,
                                                        int64_t tiles_per_group, uint64_t draws,
                                                        const pgx_noise_params *params) {
    const pgx_noise_params p = params[blockIdx.y];
    float *o = out + (int64_t)blockIdx.y * out_stride;
    const int64_t c0 = (int64_t)blockIdx.x * tiles_per_group * kWhiteTile;
    if (c0 >= n) return;
    int64_t c1 = c0 + tiles_per_group * kWhiteTile;
    if (c1 > n) c1 = n;
    const int t = threadIdx.x;
    const u128 inc = make128(p.inc_hi, p.inc_lo);
    // the state BEFORE the lane's first sample: sample i is drawn from the state after consumed + i + 1 steps
    u128 run = pcg_skip(make128(p.state_hi, p.state_lo), inc,
                        (uint64_t)p.consumed + draws + (uint64_t)c0 + (uint64_t)(t * kWhiteRun));
    const u128 jump_a = kSkip.a[kWhiteTileLog2], jump_c = kSkip.c[kWhiteTileLog2] * inc;
    for (int64_t base = c0; base < c1; base += kWhiteTile) {
        const int64_t i0 = base + t * kWhiteRun;
        if (i0 < c1) {
            u128 s = run;
            float v[kWhiteRun];
#pragma unroll
            for (int j = 0; j < kWhiteRun; ++j) {
                s = s * kPcgMult + inc;
                v[j] = noise_range(pcg_draw(s), p.scaled, p.span, p.min_value);
            }
            float *dst = o + i0;
            if (i0 + kWhiteRun <= c1 && ((uintptr_t)dst & 15u) == 0) {
                reinterpret_cast<float4 *>(dst)[0] = make_float4(v[0], v[1], v[2], v[3]);
                reinterpret_cast<float4 *>(dst)[1] = make_float4(v[4], v[5], v[6], v[7]);
            } else {
#pragma unroll
                for (int j = 0; j < kWhiteRun; ++j)
                    if (i0 + j < c1) dst[j] = v[j];
            }
        }
        run = jump_a * run + jump_c;
    }
}

// Pink.  LDS holds 8 floats per sample of the tile: [0..5] w * g_k, replaced by the taps b_k[i] as the six lanes pass,
// [6] w, [7] unused.
__global__ __launch_bounds__(kLanes) void k_noise_pink(float *out, int64_t out_stride, int64_t n, uint64_t draws,
                                                       const pgx_noise_params *params, pgx_noise_state *state) {
    __shared__ float4 tile4[kSeqTile * 2];
    float *tile = reinterpret_cast<float *>(tile4);
    const pgx_noise_params p = params[blockIdx.x];
    pgx_noise_state *st = state + blockIdx.x;
    float *o = out + (int64_t)blockIdx.x * out_stride;
    const int t = threadIdx.x;
    const float g0 = (float)0.0555179, g1 = (float)0.0750759, g2 = (float)0.1538520, g3 = (float)0.3104856,
                g4 = (float)0.5329522, g5 = (float)0.0168980;
    float a = 0.0f, b = 0.0f;
    if (t < 6) {
        a = t == 0 ? (float)0.99886 : t == 1 ? (float)0.99332 : t == 2 ? (float)0.96900 : t == 3 ? (float)0.86650
            : t == 4 ? (float)0.55000 : (float)-0.7616;
        b = st->pink[t];
    }
    float b6_carry = st->pink[6];
    const u128 inc = make128(p.inc_hi, p.inc_lo);
    u128 run = pcg_skip(make128(p.state_hi, p.state_lo), inc, (uint64_t)p.consumed + draws + (uint64_t)(t * kSeqRun));
    const u128 jump_a = kSkip.a[kSeqTileLog2], jump_c = kSkip.c[kSeqTileLog2] * inc;
    for (int64_t base = 0; base < n; base += kSeqTile) {
        const int cnt = (n - base < kSeqTile) ? (int)(n - base) : kSeqTile;
        {   // the tile's draws and their products (draws past the end of the render stay in LDS)
            u128 s = run;
#pragma unroll
            for (int j = 0; j < kSeqRun; ++j) {
                s = s * kPcgMult + inc;
                const float w = pcg_draw(s);
                const int i = t * kSeqRun + j;
                tile4[2 * i] = make_float4(w * g0, w * g1, w * g2, w * g3);
                tile4[2 * i + 1] = make_float4(w * g4, w * g5, w, 0.0f);
            }
            run = jump_a * run + jump_c;
        }
        __syncthreads();
        if (t < 6) {    // b_k = a_k * b_k + w * g_k; the sixth tap: -0.7616 * b5 - w * 0.0168980
            // groups of kSeqGroup samples: the next group's products are requested from LDS before this group's chain
            // runs, so that only the multiply and the add / subtract of each sample wait on one another
            float *mine = tile + t;
            const int groups = cnt / kSeqGroup;
            float cur[kSeqGroup], nxt[kSeqGroup] = {};
            if (groups > 0) {
#pragma unroll
                for (int j = 0; j < kSeqGroup; ++j) cur[j] = mine[j * 8];
            }
            for (int g = 0; g < groups; ++g) {
                float *at = mine + g * kSeqGroup * 8;
                if (g + 1 < groups) {
#pragma unroll
                    for (int j = 0; j < kSeqGroup; ++j) nxt[j] = at[(kSeqGroup + j) * 8];
                }
#pragma unroll
                for (int j = 0; j < kSeqGroup; ++j) {
                    const float fed = a * b;
                    b = (t == 5) ? fed - cur[j] : fed + cur[j];
                    cur[j] = b;
                }
#pragma unroll
                for (int j = 0; j < kSeqGroup; ++j) {
                    at[j * 8] = cur[j];
                    cur[j] = nxt[j];
                }
            }
            for (int i = groups * kSeqGroup; i < cnt; ++i) {
                const float fed = a * b;
                b = (t == 5) ? fed - mine[i * 8] : fed + mine[i * 8];
                mine[i * 8] = b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSeqRun; ++j) {
            const int i = j * kLanes + t;
            if (i < cnt) {
                const float4 x = tile4[2 * i], y = tile4[2 * i + 1];
                const float w = y.z;
                const float b6 = (i == 0) ? b6_carry : tile[(i - 1) * 8 + 6] * (float)0.115926;
                float pink = x.x + x.y;
                pink = pink + x.z;
                pink = pink + x.w;
                pink = pink + y.x;
                pink = pink + y.y;
                pink = pink + b6;
                pink = pink + w * (float)0.5362;
                o[base + i] = noise_range(pink * (float)0.11, p.scaled, p.span, p.min_value);
            }
        }
        b6_carry = tile[(cnt - 1) * 8 + 6] * (float)0.115926;
        __syncthreads();            // the next tile's draws overwrite the LDS tile
    }
    if (t < 6) st->pink[t] = b;
    if (t == 6) st->pink[6] = b6_carry;
}

// One brown step: last = last + d; if last < -1: last = -1 elif last > 1: last = 1 (noise_pe.py:142-146).  The level is
// finite, so the two tests are the median of (last, -1, 1): one instruction behind the add instead of two compares and
// two selects.
__device__ __forceinline__ float brown_step(float last, float d) {
    return __builtin_amdgcn_fmed3f(last + d, -1.0f, 1.0f);
}

// Brown: last = last + w * 0.02, clamped to the rails.
__global__ __launch_bounds__(kLanes) void k_noise_brown(float *out, int64_t out_stride, int64_t n, uint64_t draws,
                                                        const pgx_noise_params *params, pgx_noise_state *state) {
    __shared__ float tile[kSeqTile];
    const pgx_noise_params p = params[blockIdx.x];
    pgx_noise_state *st = state + blockIdx.x;
    float *o = out + (int64_t)blockIdx.x * out_stride;
    const int t = threadIdx.x;
    float last = st->brown;
    const u128 inc = make128(p.inc_hi, p.inc_lo);
    u128 run = pcg_skip(make128(p.state_hi, p.state_lo), inc, (uint64_t)p.consumed + draws + (uint64_t)(t * kSeqRun));
    const u128 jump_a = kSkip.a[kSeqTileLog2], jump_c = kSkip.c[kSeqTileLog2] * inc;
    for (int64_t base = 0; base < n; base += kSeqTile) {
        const int cnt = (n - base < kSeqTile) ? (int)(n - base) : kSeqTile;
        {
            u128 s = run;
            float v[kSeqRun];
#pragma unroll
            for (int j = 0; j < kSeqRun; ++j) {
                s = s * kPcgMult + inc;
                v[j] = pcg_draw(s) * (float)0.02;
            }
            reinterpret_cast<float4 *>(tile)[t] = make_float4(v[0], v[1], v[2], v[3]);
            run = jump_a * run + jump_c;
        }
        __syncthreads();
        if (t == 0) {
            // groups of kSeqGroup samples held in registers, the next group requested before this group's chain runs
            const int groups = cnt / kSeqGroup;
            float cur[kSeqGroup], nxt[kSeqGroup] = {};
            if (groups > 0) {
#pragma unroll
                for (int j = 0; j < kSeqGroup; ++j) cur[j] = tile[j];
            }
            for (int g = 0; g < groups; ++g) {
                float *at = tile + g * kSeqGroup;
                if (g + 1 < groups) {
#pragma unroll
                    for (int j = 0; j < kSeqGroup; ++j) nxt[j] = at[kSeqGroup + j];
                }
#pragma unroll
                for (int j = 0; j < kSeqGroup; ++j) {
                    last = brown_step(last, cur[j]);
                    cur[j] = last;
                }
#pragma unroll
                for (int j = 0; j < kSeqGroup; ++j) {
                    at[j] = cur[j];
                    cur[j] = nxt[j];
                }
            }
            for (int i = groups * kSeqGroup; i < cnt; ++i) {
                last = brown_step(last, tile[i]);
                tile[i] = last;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSeqRun; ++j) {
            const int i = j * kLanes + t;
            if (i < cnt) o[base + i] = noise_range(tile[i], p.scaled, p.span, p.min_value);
        }
        __syncthreads();
    }
    if (t == 0) st->brown = last;
}

}  // namespace

namespace pgx {

const SkipTable *pcg_skip_table_device() {
    void *p = nullptr;
    const hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(kSkip));
    if (e != hipSuccess) {
        fail(PGX_ERR_RUNTIME, std::string("pcg_skip_table_device: ") + hipGetErrorString(e));
        return nullptr;
    }
    return static_cast<const SkipTable *>(p);
}

}  // namespace pgx

extern "C" {

int pgx_noise_skip_table(uint64_t *table) {
    if (!table) return pgx::fail(PGX_ERR_INVALID, "pgx_noise_skip_table: null table");
    for (int k = 0; k < 64; ++k) {
        table[4 * k + 0] = (uint64_t)(kSkipHost.a[k] >> 64);
        table[4 * k + 1] = (uint64_t)kSkipHost.a[k];
        table[4 * k + 2] = (uint64_t)(kSkipHost.c[k] >> 64);
        table[4 * k + 3] = (uint64_t)kSkipHost.c[k];
    }
    return PGX_OK;
}

int pgx_noise_white(float *out, int64_t out_stride, int batch, int64_t n, uint64_t draws,
                    const pgx_noise_params *params) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && out_stride >= n && batch <= 65535, "pgx_noise_white: bad argument");
    const int64_t tiles = pgx::ceil_div(n, kWhiteTile);
    const int64_t groups = tiles < kWhiteMaxGrid ? tiles : kWhiteMaxGrid;
    const int64_t per_group = pgx::ceil_div(tiles, groups);
    hipLaunchKernelGGL(k_noise_white, dim3((unsigned)pgx::ceil_div(tiles, per_group), (unsigned)batch), dim3(kLanes), 0,
                       pgx::stream(), out, out_stride, n, per_group, draws, params);
    PGX_LAUNCH_CHECK("k_noise_white");
    return PGX_OK;
}

int pgx_noise_pink(float *out, int64_t out_stride, int batch, int64_t n, uint64_t draws,
                   const pgx_noise_params *params, pgx_noise_state *state) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && state && out_stride >= n, "pgx_noise_pink: bad argument");
    hipLaunchKernelGGL(k_noise_pink, dim3((unsigned)batch), dim3(kLanes), 0, pgx::stream(), out, out_stride, n, draws,
                       params, state);
    PGX_LAUNCH_CHECK("k_noise_pink");
    return PGX_OK;
}

int pgx_noise_brown(float *out, int64_t out_stride, int batch, int64_t n, uint64_t draws,
                    const pgx_noise_params *params, pgx_noise_state *state) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && state && out_stride >= n, "pgx_noise_brown: bad argument");
    hipLaunchKernelGGL(k_noise_brown, dim3((unsigned)batch), dim3(kLanes), 0, pgx::stream(), out, out_stride, n, draws,
                       params, state);
    PGX_LAUNCH_CHECK("k_noise_brown");
    return PGX_OK;
}

}  // extern "C"
