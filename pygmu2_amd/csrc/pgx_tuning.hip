// pgx_tuning.hip -- TransformPE chains that hold a tuning step: pitch <-> frequency and interval <-> ratio under an
// equal temperament or a just-intonation ratio table (pygmu2_amd/temperament.py), next to the named element-wise
// operations of pgx_transform, in one launch with one rounding to float32.
//
// Parity: apart from exp2 and log2 every operation below is one correctly rounded IEEE operation on the operands
// the numpy expression has, in its order (the library is built with -ffp-contract=off; `/` on doubles is the IEEE
// division).  The just table's logarithms are numpy's own bits, uploaded by the host.  exp2 / log2 are the device
// library's, within an ulp or two of numpy's libm (tests/test_gpu_tuning.py measures them through
// pgx_selftest_tuning).  Powers of two with an integer exponent (2.0 ** octaves) are exact here as they are there.
#include "pgx_common.h"

namespace {

constexpr int kBlock = 256;
constexpr double kFloor = 1e-10;            // the reference's guard in front of log2

// 2.0 ** k for an integer-valued double k: exact, inf / 0 beyond the range like numpy's pow, NaN for NaN
__device__ __forceinline__ double pow2_int(double k) {
    if (k != k) return k;
    const double c = k < -2200.0 ? -2200.0 : (k > 2200.0 ? 2200.0 : k);
    return ldexp(1.0, (int)c);
}

__device__ __forceinline__ double et_pitch_to_freq(double x, const pgx_tuning_record &t) {
    return t.reference_freq * exp2((x - t.reference_pitch) / t.divisions);
}

__device__ __forceinline__ double et_freq_to_pitch(double x, const pgx_tuning_record &t) {
    const double f = x < kFloor ? kFloor : x;                           // np.maximum: NaN passes
    return t.reference_pitch + t.divisions * log2(f / t.reference_freq);
}

__device__ __forceinline__ double ji_pitch_to_freq(double x, const pgx_tuning_record &t, const double *tables) {
    const int n = t.num_notes;
    const double nd = t.divisions;
    const double rel = x - t.reference_pitch;
    const double octaves = floor(rel / nd);
    const double degree = rel - octaves * nd;        // in [0, N]; exactly N for a tiny negative rel (index 0, lower octave)
    const double fl = floor(degree);
    const double frac = degree - fl;
    // numpy casts floor(degree) to an integer; beyond that range (|pitch| ~ 1e16 and more, inf, NaN) its index is
    // arbitrary -- here the sample is NaN and nothing is read
    if (!(fabs(fl) < 2147483648.0)) return __builtin_nan("");
    int idx = (int)fl % n;
    if (idx < 0) idx += n;                           // Python's %, as numpy's: never negative
    const double *logs = tables + t.table_offset;
    const double log_floor = logs[idx];
    // logs[N] = log2(ratios[0] * 2.0): the reference doubles the upper ratio only when idx == N - 1 and frac > 0, and
    // takes log2(ratios[0]) when frac == 0 -- there the difference is multiplied by zero, so the N + 1 table gives
    // the same log_interp without the case split
    const double log_ceil = logs[idx + 1];
    const double log_interp = log_floor + frac * (log_ceil - log_floor);
    const double total = exp2(log_interp) * pow2_int(octaves);
    return t.reference_freq * total;
}

__device__ __forceinline__ double ji_freq_to_pitch(double x, const pgx_tuning_record &t, const double *tables) {
    const int n = t.num_notes;
    const double f = x < kFloor ? kFloor : x;
    const double ratio = f / t.reference_freq;
    const double octaves = floor(log2(ratio));
    const double r = ratio / pow2_int(octaves);
    const double *ratios = tables + t.table_offset + n + 1;
    int best = 0;                                    // np.argmin: the first minimum; with a NaN, index 0
    double dbest = fabs(ratios[0] - r);
    for (int i = 1; i < n; ++i) {
        const double d = fabs(ratios[i] - r);
        if (d < dbest) {
            dbest = d;
            best = i;
        }
    }
    return t.reference_pitch + (octaves * t.divisions + (double)best);
}

__device__ __forceinline__ double tuning_step(int code, double v, const pgx_tuning_record &t, const double *tables) {
    switch (code) {
    case 7: return et_pitch_to_freq(v, t);
    case 8: return et_freq_to_pitch(v, t);
    case 9: return t.num_notes >= 2 ? ji_pitch_to_freq(v, t, tables) : __builtin_nan("");    // an equal record: no table
    case 10: return t.num_notes >= 2 ? ji_freq_to_pitch(v, t, tables) : __builtin_nan("");
    default: return v;
    }
}

// The op program is the same for every thread: the loop and its switch branch uniformly, the ops and the records are
// read through the scalar cache, the just table (a few hundred bytes) stays in L1 / L2.
__global__ void __launch_bounds__(kBlock)
k_tuning(float *out, const float *in, int64_t n_elems, const pgx_tuning_op *ops, int nops,
         const pgx_tuning_record *tunings, const double *tables) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n_elems; e += stride) {
        double v = (double)in[e];
        for (int k = 0; k < nops; ++k) {
            const pgx_tuning_op op = ops[k];
            switch (op.code) {                                                 // 0-6: k_transform's arithmetic
            case 0: v = op.p1 + op.p0 * v; break;
            case 1: v = v < op.p0 ? op.p0 : (v > op.p1 ? op.p1 : v); break;
            case 2: v = sqrt(v); break;
            case 3: v = v * v; break;
            case 4: v = fabs(v); break;
            case 5: v = tanh(v); break;
            case 6: v = 1.0 - v; break;
            case 7: case 8: case 9: case 10: v = tuning_step(op.code, v, tunings[op.tuning], tables); break;
            default: break;
            }
        }
        out[e] = (float)v;
    }
}

// A bank of TransformPEs whose chains hold the same steps with per-voice parameters (voice_bank.py): voice blockIdx.y
// runs its own nops ops over its own per_voice elements -- k_transform's arithmetic, element for element.
__global__ void __launch_bounds__(kBlock)
k_transform_bank(float *out, const float *in, int64_t per_voice, const pgx_transform_op *ops, int nops) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t base = (int64_t)blockIdx.y * per_voice;
    ops += (int64_t)blockIdx.y * nops;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < per_voice; e += stride) {
        double v = (double)in[base + e];
        for (int k = 0; k < nops; ++k) {
            const pgx_transform_op op = ops[k];
            switch (op.code) {
            case 0: v = op.p1 + op.p0 * v; break;
            case 1: v = v < op.p0 ? op.p0 : (v > op.p1 ? op.p1 : v); break;
            case 2: v = sqrt(v); break;
            case 3: v = v * v; break;
            case 4: v = fabs(v); break;
            case 5: v = tanh(v); break;
            case 6: v = 1.0 - v; break;
            default: break;
            }
        }
        out[base + e] = (float)v;
    }
}

__global__ void __launch_bounds__(kBlock)
k_selftest_tuning(double *out, const double *in, int64_t n, int code, const pgx_tuning_record *tunings,
                  const double *tables) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += stride)
        out[e] = tuning_step(code, in[e], tunings[0], tables);
}

}  // namespace

extern "C" {

int pgx_tuning(float *out, const float *in, int64_t n_elems, const pgx_tuning_op *ops, int nops,
               const pgx_tuning_record *tunings, const double *tables) {
    PGX_REQUIRE_INIT();
    if (n_elems <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && (ops || nops == 0) && nops >= 0, "pgx_tuning: bad argument");
    PGX_CHECK_ARG(tunings != nullptr, "pgx_tuning: no tuning records (a chain without a tuning step is pgx_transform's)");
    hipLaunchKernelGGL(k_tuning, dim3(pgx::grid_for(n_elems, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in,
                       n_elems, ops, nops, tunings, tables);
    PGX_LAUNCH_CHECK("k_tuning");
    return PGX_OK;
}

int pgx_transform_bank(float *out, const float *in, int64_t per_voice, int batch, const pgx_transform_op *ops,
                       int nops) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(batch >= 0 && batch <= 65535, "pgx_transform_bank: bad argument");
    if (per_voice <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && (ops || nops == 0) && nops >= 0, "pgx_transform_bank: bad argument");
    hipLaunchKernelGGL(k_transform_bank, dim3(pgx::grid_for(per_voice, kBlock), (unsigned)batch), dim3(kBlock), 0,
                       pgx::stream(), out, in, per_voice, ops, nops);
    PGX_LAUNCH_CHECK("k_transform_bank");
    return PGX_OK;
}

int pgx_selftest_tuning(double *out, const double *in, int64_t n, int code, const pgx_tuning_record *tunings,
                        const double *tables) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && tunings, "pgx_selftest_tuning: null pointer");
    PGX_CHECK_ARG(code >= 7 && code <= 10, "pgx_selftest_tuning: code must be 7..10");
    PGX_CHECK_ARG(code < 9 || tables != nullptr, "pgx_selftest_tuning: a just tuning needs its tables");
    hipLaunchKernelGGL(k_selftest_tuning, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in, n,
                       code, tunings, tables);
    PGX_LAUNCH_CHECK("k_selftest_tuning");
    return PGX_OK;
}

}  // extern "C"
