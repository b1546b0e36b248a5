// pgx_phase.hip -- PEs whose state is a carried phase, the prefix sum of per-sample increments: the stateful SinePE
// (sine_pe.py:177-232) and its bank, and the stateful gate (function_gen_pe.py:157-193).  Scan primitives: pgx_scan.h.

#include <cstdlib>
#include <type_traits>

#include "pgx_common.h"
#include "pgx_scan.h"

namespace {

// ================================================================================================
// SinePE, stateful path
// ================================================================================================
constexpr int kSinT = 8;
constexpr int kSinTile = kBlock * kSinT;

// One tile of the stateful sine: frames [base, base + kSinTile) of a row of n.  The thread's increments are summed serially
// over its kSinT frames, block_excl_sum gives its offset inside the tile and the tile's total (which depends on no carry);
// the phase of a frame is ((carry_sum + off) + loc) + initial.  TOTAL_ONLY: the total alone, nothing else read or written
// -- what the time-parallel bank's first launch needs; the same code, so the same sum.  k_sine_stateful and the bank
// kernels all come through here: their samples are the same by construction (-ffp-contract=off: inlining changes no sum).
template <bool TOTAL_ONLY>
__device__ __forceinline__ double sine_tile(float *out, int64_t base, int64_t n, int channels, double sr,
                                            const pgx_sine_stateful_params &p, const float *freq, const float *amp,
                                            const float *phase_mod, double carry_sum, double initial, double *lds,
                                            double &final_phase, bool &have_final) {
    const double two_pi = 2.0 * kPi;
    const int64_t f0 = base + (int64_t)threadIdx.x * kSinT;
    double loc[kSinT];
    double run = 0.0;
    // the control values of the thread's frames first, unconditionally (clamped index): behind the bounds test every
    // load is waited for at once, one memory latency per value on a kernel that is one workgroup walking the block
    float f_in[kSinT], pm_in[kSinT], a_in[kSinT];
    if (freq) {
#pragma unroll
        for (int j = 0; j < kSinT; ++j) f_in[j] = freq[(f0 + j < n) ? f0 + j : n - 1];
    }
    if (!TOTAL_ONLY && phase_mod) {
#pragma unroll
        for (int j = 0; j < kSinT; ++j) pm_in[j] = phase_mod[(f0 + j < n) ? f0 + j : n - 1];
    }
    if (!TOTAL_ONLY && amp) {
#pragma unroll
        for (int j = 0; j < kSinT; ++j) a_in[j] = amp[(f0 + j < n) ? f0 + j : n - 1];
    }
#pragma unroll
    for (int j = 0; j < kSinT; ++j) {
        double f = p.freq;
        if (freq) f = (f0 + j < n) ? (double)f_in[j] : 0.0;
        double inc = (f0 + j < n) ? (two_pi * f) / sr : 0.0;
        run = run + inc;
        loc[j] = run;
    }
    double tile_total;
    double off = block_excl_sum(run, lds, tile_total);
    if (TOTAL_ONLY) return tile_total;
    const double chunk_base = carry_sum + off;

    float yf[kSinT];
#pragma unroll
    for (int j = 0; j < kSinT; ++j) {
        double ph = (chunk_base + loc[j]) + initial;             // cumsum + initial_phase (:217)
        double pm = p.phase;
        if (phase_mod) pm = (f0 + j < n) ? (double)pm_in[j] : 0.0;
        ph = ph + pm;                                            // + phase_mod (:220-223)
        double a = p.amp;
        if (amp) a = (f0 + j < n) ? (double)a_in[j] : 0.0;
        yf[j] = (float)(a * pgx::pgx_sin(ph));
        if (f0 + j == n - 1) {
            final_phase = ph;
            have_final = true;
        }
    }
    store_frames_tiled<kSinT>(out, f0, n, channels, yf);
    return tile_total;
}

// One workgroup walks a row tile by tile; the carry is the left fold of the tiles' totals, ((0 + T0) + T1) + ...
__device__ __forceinline__ void sine_walk(float *out, int64_t n, int channels, double sr,
                                          const pgx_sine_stateful_params &p, const float *freq, const float *amp,
                                          const float *phase_mod, double *state, double *lds) {
    // sine_pe.py:203-214: first render starts from the scalar phase (0 when phase is a PE)
    const bool inited = state[1] != 0.0;
    const double initial = inited ? state[0] : (p.phase_is_stream ? 0.0 : p.phase);
    double carry_sum = 0.0;
    double final_phase = 0.0;
    bool have_final = false;
    for (int64_t base = 0; base < n; base += kSinTile)
        carry_sum = carry_sum + sine_tile<false>(out, base, n, channels, sr, p, freq, amp, phase_mod, carry_sum, initial,
                                                 lds, final_phase, have_final);
    if (have_final) {
        state[0] = final_phase;
        state[1] = 1.0;
    }
}

__global__ void __launch_bounds__(kBlock)
k_sine_stateful(float *out, int64_t n, int channels, double sr, const pgx_sine_stateful_params *params,
                const float *freq, const float *amp, const float *phase_mod, double *state) {
    __shared__ double lds[kWaves];
    const pgx_sine_stateful_params p = params[0];
    sine_walk(out, n, channels, sr, p, freq, amp, phase_mod, state, lds);
}

// Bank of stateful sines (pgx_sine_stateful_bank, voice_bank.py), the walk: k_sine_stateful with the voice in blockIdx.x.
__global__ void __launch_bounds__(kBlock)
k_sine_stateful_bank(float *out, int64_t out_stride, int64_t n, int channels, double sr,
                     const pgx_sine_stateful_params *params, const float *freq, int64_t freq_stride, const float *amp,
                     int64_t amp_stride, const float *phase_mod, int64_t phase_stride, double *state) {
    __shared__ double lds[kWaves];
    const int64_t v = blockIdx.x;
    const pgx_sine_stateful_params p = params[v];
    sine_walk(out + v * out_stride, n, channels, sr, p, freq ? freq + v * freq_stride : nullptr,
              amp ? amp + v * amp_stride : nullptr, phase_mod ? phase_mod + v * phase_stride : nullptr, state + v * 2, lds);
}

// The time-parallel form: a workgroup per tile and voice, two launches, nothing passes between the workgroups of a launch.
// Voice v's slice of the workspace: {phase, initialised} as they were on entry, then one total per tile.
//   k_sine_bank_totals  tile t's total, exactly as the walk sums it; tile 0's workgroup copies state[v] (the apply launch
//                       overwrites state[v] while others of its workgroups, not resident yet, still need what was there).
//   k_sine_bank_apply   carry = ((0 + T0) + T1) + ... + T(t-1), folded serially in the walk's order (a sum of group sums
//                       is another association); the tile's frames; the owner of frame n - 1 writes state[v].
__global__ void __launch_bounds__(kBlock)
k_sine_bank_totals(int64_t n, double sr, const pgx_sine_stateful_params *params, const float *freq, int64_t freq_stride,
                   const double *state, double *ws, int64_t tiles) {
    __shared__ double lds[kWaves];
    const int64_t t = blockIdx.x, v = blockIdx.y;
    const pgx_sine_stateful_params p = params[v];
    double *slice = ws + v * (tiles + 2);
    double final_phase = 0.0;
    bool have_final = false;
    const double total = sine_tile<true>(nullptr, t * kSinTile, n, 1, sr, p, freq ? freq + v * freq_stride : nullptr,
                                         nullptr, nullptr, 0.0, 0.0, lds, final_phase, have_final);
    if (threadIdx.x == 0) {
        slice[2 + t] = total;
        if (t == 0) {
            slice[0] = state[v * 2 + 0];
            slice[1] = state[v * 2 + 1];
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_sine_bank_apply(float *out, int64_t out_stride, int64_t n, int channels, double sr,
                  const pgx_sine_stateful_params *params, const float *freq, int64_t freq_stride, const float *amp,
                  int64_t amp_stride, const float *phase_mod, int64_t phase_stride, double *state, const double *ws,
                  int64_t tiles) {
    __shared__ double lds[kWaves];
    const int64_t t = blockIdx.x, v = blockIdx.y;
    const pgx_sine_stateful_params p = params[v];
    const double *slice = ws + v * (tiles + 2);
    const bool inited = slice[1] != 0.0;                         // (never state[v]: see above)
    const double initial = inited ? slice[0] : (p.phase_is_stream ? 0.0 : p.phase);
    double carry_sum = 0.0;
    for (int64_t i = 0; i < t; ++i) carry_sum = carry_sum + slice[2 + i];
    double final_phase = 0.0;
    bool have_final = false;
    sine_tile<false>(out + v * out_stride, t * kSinTile, n, channels, sr, p, freq ? freq + v * freq_stride : nullptr,
                     amp ? amp + v * amp_stride : nullptr, phase_mod ? phase_mod + v * phase_stride : nullptr, carry_sum,
                     initial, lds, final_phase, have_final);
    if (have_final) {
        state[v * 2 + 0] = final_phase;
        state[v * 2 + 1] = 1.0;
    }
}

// ================================================================================================
// PeriodicGate with PE-driven frequency / duty / phase: FunctionGenPE's stateful rectangle path
// (function_gen_pe.py:157-193): base = mod(phase0 + [0, cumsum(f/sr)[:-1]], 1); gate = mod(base + ph, 1) < duty.
// One workgroup: exclusive prefix sum of the increments, like the stateful sine.
// state = { carried phase }.
// ================================================================================================
constexpr int kGateT = 8;
constexpr int kGateTile = kBlock * kGateT;

__global__ void __launch_bounds__(kBlock)
k_gate_stateful(float *out, int64_t n, double sr, double freq_scalar, double duty_scalar, double phase_scalar,
                const float *freq, const float *duty, const float *phase, double *state) {
    __shared__ double lds[kWaves];
    const int tid = threadIdx.x;
    const double phase0 = state[0];
    double carry_sum = 0.0;
    for (int64_t base = 0; base < n; base += kGateTile) {
        const int64_t f0 = base + (int64_t)tid * kGateT;
        double loc[kGateT];
        double run = 0.0;
        // control values first, unconditionally (see k_sine_stateful)
        float f_in[kGateT], ph_in[kGateT], d_in[kGateT];
        if (freq) {
#pragma unroll
            for (int j = 0; j < kGateT; ++j) f_in[j] = freq[(f0 + j < n) ? f0 + j : n - 1];
        }
        if (phase) {
#pragma unroll
            for (int j = 0; j < kGateT; ++j) ph_in[j] = phase[(f0 + j < n) ? f0 + j : n - 1];
        }
        if (duty) {
#pragma unroll
            for (int j = 0; j < kGateT; ++j) d_in[j] = duty[(f0 + j < n) ? f0 + j : n - 1];
        }
#pragma unroll
        for (int j = 0; j < kGateT; ++j) {
            loc[j] = run;                                             // exclusive within the chunk
            const double f = freq ? ((f0 + j < n) ? (double)f_in[j] : 0.0) : freq_scalar;
            run = run + ((f0 + j < n) ? f / sr : 0.0);
        }
        double tile_total;
        const double off = block_excl_sum(run, lds, tile_total);
        const double chunk_base = carry_sum + off;
        carry_sum = carry_sum + tile_total;
#pragma unroll
        for (int j = 0; j < kGateT; ++j) {
            if (f0 + j >= n) break;
            const double b = pgx::pgx_mod1(phase0 + (chunk_base + loc[j]));
            const double ph = pgx::pgx_mod1(b + (phase ? (double)ph_in[j] : phase_scalar));
            double d = duty ? (double)d_in[j] : duty_scalar;
            d = d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d);
            out[f0 + j] = (ph < d) ? 1.0f : 0.0f;
        }
    }
    if (tid == 0) state[0] = pgx::pgx_mod1(phase0 + carry_sum);       // mod(phase + sum(dt), 1)
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

int pgx_gate_stateful(float *out, int64_t n, double sample_rate, double freq, double duty, double phase,
                      const float *freq_stream, const float *duty_stream, const float *phase_stream, double *state) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && state && sample_rate > 0, "pgx_gate_stateful: bad argument");
    hipLaunchKernelGGL(k_gate_stateful, dim3(1), dim3(kBlock), 0, pgx::stream(), out, n, sample_rate, freq, duty,
                       phase, freq_stream, duty_stream, phase_stream, state);
    PGX_LAUNCH_CHECK("k_gate_stateful");
    return PGX_OK;
}

int pgx_sine_stateful(float *out, int64_t n, int channels, double sample_rate,
                      const pgx_sine_stateful_params *params, const float *freq, const float *amp,
                      const float *phase_mod, double *state) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && state && channels >= 1 && sample_rate > 0, "pgx_sine_stateful: bad argument");
    hipLaunchKernelGGL(k_sine_stateful, dim3(1), dim3(kBlock), 0, pgx::stream(), out, n, channels, sample_rate,
                       params, freq, amp, phase_mod, state);
    PGX_LAUNCH_CHECK("k_sine_stateful");
    return PGX_OK;
}

// A bank of stateful sines.  Without a workspace, or for blocks of up to two tiles: the walk, a workgroup per voice.  With
// one: a workgroup per tile and voice (k_sine_bank_totals, k_sine_bank_apply).  Row v is pgx_sine_stateful's either way.
constexpr int64_t kSinBankMaxTiles = (int64_t)1 << 22;          // (grid.x; longer rows are walked)

size_t pgx_sine_stateful_bank_workspace_bytes(int64_t n, int batch) {
    if (n <= 0 || batch <= 0) return 0;
    return (size_t)batch * (size_t)(pgx::ceil_div(n, (int64_t)kSinTile) + 2) * sizeof(double);
}

int pgx_sine_stateful_bank(float *out, int64_t out_stride, int batch, int64_t n, int channels, double sample_rate,
                           const pgx_sine_stateful_params *params, const float *freq, int64_t freq_stride,
                           const float *amp, int64_t amp_stride, const float *phase_mod, int64_t phase_stride,
                           double *state, void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && state && channels >= 1 && sample_rate > 0 && batch <= 65535,
                  "pgx_sine_stateful_bank: bad argument");
    PGX_CHECK_ARG(out_stride >= n * channels && (!freq || freq_stride >= n) && (!amp || amp_stride >= n) &&
                      (!phase_mod || phase_stride >= n),
                  "pgx_sine_stateful_bank: a stride below its row");
    const int64_t tiles = pgx::ceil_div(n, (int64_t)kSinTile);
    if (workspace == nullptr || tiles <= 2 || tiles > kSinBankMaxTiles) {
        hipLaunchKernelGGL(k_sine_stateful_bank, dim3(batch), dim3(kBlock), 0, pgx::stream(), out, out_stride, n,
                           channels, sample_rate, params, freq, freq_stride, amp, amp_stride, phase_mod, phase_stride,
                           state);
        PGX_LAUNCH_CHECK("k_sine_stateful_bank");
        return PGX_OK;
    }
    double *ws = (double *)workspace;
    hipLaunchKernelGGL(k_sine_bank_totals, dim3((unsigned)tiles, batch), dim3(kBlock), 0, pgx::stream(), n, sample_rate,
                       params, freq, freq_stride, (const double *)state, ws, tiles);
    PGX_LAUNCH_CHECK("k_sine_bank_totals");
    hipLaunchKernelGGL(k_sine_bank_apply, dim3((unsigned)tiles, batch), dim3(kBlock), 0, pgx::stream(), out, out_stride,
                       n, channels, sample_rate, params, freq, freq_stride, amp, amp_stride, phase_mod, phase_stride,
                       state, (const double *)ws, tiles);
    PGX_LAUNCH_CHECK("k_sine_bank_apply");
    return PGX_OK;
}

}  // extern "C"
