// pgx_lookup.hip -- gather / curve / sample-format kernels of the PEs either side of the hot path
// (SURVEY.md section 8f ranks 3-4): DelayPE's interpolated lookup, PiecewisePE, PCM16 conversion.
//
// All of them are one thread per output frame, HBM-bound, and reproduce the reference's numpy
// expression order (compiled with -ffp-contract=off) so that the linear/step paths are bit-exact.

#include "pgx_common.h"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ double block_excl_sum(double v, double *lds, double &total) {
    return pgx::block_excl_sum<kBlock / 64>(v, lds, total);
}

// ------------------------------------------------------------------------------------------------
// DelayPE / interpolated_lookup (interpolated_lookup.py:28-77, delay_pe.py:170-216)
//   index = float64(start + i) - delay[i];  floor, fraction, clipped neighbours of the rendered
//   source window [win_start, win_start + win_len); out-of-extent indices -> 0.
// ------------------------------------------------------------------------------------------------
// One output frame of _linear_interp / _cubic_interp (interpolated_lookup.py:33-87) at the fractional `index` over the
// window [win_start, win_start + win_len) -- in HBM or staged in LDS: every caller of interpolated_lookup (DelayPE,
// WavetablePE, TimeWarpPE) interpolates through this one function.
__device__ __forceinline__ void interp_at(float *o, const float *win, int64_t win_start, int64_t win_len, int channels,
                                          double index, int cubic, bool oob) {
    const double fl = floor(index);
    const double t = index - fl;
    const int64_t p1 = (int64_t)fl - win_start;
    const int64_t last = win_len - 1;
    auto clip = [last](int64_t v) { return v < 0 ? 0 : (v > last ? last : v); };
    if (!cubic) {
        const float *a = win + clip(p1) * channels;
        const float *b = win + clip(p1 + 1) * channels;
        for (int c = 0; c < channels; ++c) {
            const double v = (1.0 - t) * (double)a[c] + t * (double)b[c];
            o[c] = oob ? 0.0f : (float)v;
        }
    } else {
        const float *q0 = win + clip(p1 - 1) * channels;
        const float *q1 = win + clip(p1) * channels;
        const float *q2 = win + clip(p1 + 1) * channels;
        const float *q3 = win + clip(p1 + 2) * channels;
        const double t2 = t * t;
        const double t3 = t2 * t;
        for (int c = 0; c < channels; ++c) {
            const float p0 = q0[c], pa = q1[c], pb = q2[c], pc = q3[c];
            // float32 sub-expressions, exactly as numpy evaluates `2.0 * p1`, `-p0 + p2`, ... on float32 arrays
            const float k0 = 2.0f * pa;
            const float k1 = -p0 + pb;
            const float k2 = ((2.0f * p0 - 5.0f * pa) + 4.0f * pb) - pc;
            const float k3 = ((-p0 + 3.0f * pa) - 3.0f * pb) + pc;
            const double v = 0.5 * ((((double)k0 + (double)k1 * t) + (double)k2 * t2) + (double)k3 * t3);
            o[c] = oob ? 0.0f : (float)v;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_interp_lookup(float *out, const float *win, int64_t win_start, int64_t win_len, int channels, int64_t start,
                int64_t n, double delay_scalar, const float *delay, int cubic, int bounded, double ext_start,
                double ext_end) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double index = (double)(start + i) - (delay ? (double)delay[i] : delay_scalar);
        const bool oob = bounded && (index < ext_start || index >= ext_end);
        interp_at(out + i * channels, win, win_start, win_len, channels, index, cubic, oob);
    }
}

// One element into a thread's running (min, max) of a range reduction.  np.min / np.max propagate NaN, fmin / fmax drop
// it as soon as a number follows: `nan` is the thread's sticky flag, folded in (lo = hi = NaN) before the workgroup's
// reduction, which keeps a NaN from then on.
__device__ __forceinline__ void range_take(double &lo, double &hi, bool &nan, double v) {
    lo = fmin(lo, v);
    hi = fmax(hi, v);
    nan = nan || v != v;
}

// min / max of float64(start + i) - delay[i] over the block -> result[0..1]  (one workgroup); (NaN, NaN) if any index
// is NaN: the host rejects such a delay stream
__global__ void __launch_bounds__(kBlock)
k_index_range(double *result, const float *delay, int64_t start, int64_t n) {
    __shared__ double smin[kBlock], smax[kBlock];
    double lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) range_take(lo, hi, nan, (double)(start + i) - (double)delay[i]);
    if (nan) lo = hi = NAN;
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = smin[threadIdx.x + s], b = smax[threadIdx.x + s];
            if (a != a || a < smin[threadIdx.x]) smin[threadIdx.x] = a;
            if (b != b || b > smax[threadIdx.x]) smax[threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        result[0] = smin[0];
        result[1] = smax[0];
    }
}

// min / max of a control stream, one (min, max) pair per workgroup (the host folds the few pairs): LadderPE sizes
// the warm-up of its time segments from the lowest cutoff and the highest resonance of the block.  NaN propagates.
__global__ void __launch_bounds__(kBlock)
k_stream_range(double *partials, const float *x, int64_t n) {
    __shared__ double smin[kBlock], smax[kBlock];
    double lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        range_take(lo, hi, nan, (double)x[i]);
    }
    if (nan) lo = hi = NAN;
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = smin[threadIdx.x + s], b = smax[threadIdx.x + s];
            if (a != a || a < smin[threadIdx.x]) smin[threadIdx.x] = a;
            if (b != b || b > smax[threadIdx.x]) smax[threadIdx.x] = b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partials[blockIdx.x * 2 + 0] = smin[0];
        partials[blockIdx.x * 2 + 1] = smax[0];
    }
}

// ------------------------------------------------------------------------------------------------
// WavetablePE (wavetable_pe.py:117-169): out[i] = table[indexer[i]], the index put through the out-of-bounds rule
// first.  mode: 0 zero, 1 clamp, 2 wrap; `finite` == 0 (an unbounded table) leaves the index raw in every mode.
// ------------------------------------------------------------------------------------------------
// The window is staged in LDS up to this size (10 KiB of a CU's 160: LDS never limits the waves on a CU) -- a 2048-frame
// mono table with its guard frames.  Measured per launch (tools/playback_probe.py, profiles/r5_playback_probe.md), staged
// against gathered from global memory: 2 051 floats 6.4 vs 6.9 us at 1 M frames, 4.4 vs 4.4 at 48 000; 4 003 floats 7.2
// vs 7.8 (random indices) but 7.2 vs 6.8 (saw) at 1 M and 5.4 vs 4.4 at 48 000; 8 003 floats slower everywhere (8.7 vs
// 4.4 at 48 000): a table this small lives in the caches anyway, and what staging costs is a grid of few, long workgroups.
constexpr int kWtLdsFloats = 2560;
constexpr int kWtLdsMaxFloats = 16384;    // 64 KiB: the most a launch may ask for (PGX_WT_LDS_FLOATS)

__device__ __forceinline__ double wt_index(double raw, int mode, int finite, double wt_start, double wt_end, bool &oob) {
    oob = false;
    if (!finite) return raw;
    if (mode == 2) {
        // numpy's float `%`: fmod (exact), then the divisor's sign
        const double len = wt_end - wt_start;
        double m = fmod(raw - wt_start, len);
        if (m != 0.0) {
            if (m < 0.0) m += len;
        } else {
            m = copysign(0.0, len);
        }
        return m + wt_start;
    }
    if (mode == 1) {
        const double hi = wt_end - 1.0;                      // np.clip: NaN stays NaN
        return raw < wt_start ? wt_start : (raw > hi ? hi : raw);
    }
    oob = raw < wt_start || raw >= wt_end;
    return raw;
}

// `staged` != 0: the window (kWtLdsFloats floats by default) is copied to LDS once per workgroup and every gather is served
// from there; the grid is sized so that each workgroup has at least as many gathers to make as floats to stage.
__global__ void __launch_bounds__(kBlock)
k_wavetable(float *out, const float *indexer, int64_t n, const float *win, int64_t win_start, int64_t win_len,
            int channels, int cubic, int mode, int finite, double wt_start, double wt_end, int staged) {
    extern __shared__ float tab[];
    if (staged) {
        const int m = (int)(win_len * channels);
        for (int k = threadIdx.x; k < m; k += kBlock) tab[k] = win[k];
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        bool oob;
        const double index = wt_index((double)indexer[i], mode, finite, wt_start, wt_end, oob);
        if (staged) interp_at(out + i * channels, tab, win_start, win_len, channels, index, cubic, oob);
        else interp_at(out + i * channels, win, win_start, win_len, channels, index, cubic, oob);
    }
}

// NaN-propagating min / max of one value per thread over the workgroup -> (lo, hi) on thread 0
__device__ __forceinline__ void block_range(double &lo, double &hi, double *smin, double *smax) {
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double a = smin[threadIdx.x + s], b = smax[threadIdx.x + s];
            if (a != a || a < smin[threadIdx.x]) smin[threadIdx.x] = a;
            if (b != b || b > smax[threadIdx.x]) smax[threadIdx.x] = b;
        }
        __syncthreads();
    }
    lo = smin[0];
    hi = smax[0];
    __syncthreads();
}

// min / max of the processed indices -> result[0..1] (one workgroup): the window of a table that is not kept;
// (NaN, NaN) if any processed index is NaN
__global__ void __launch_bounds__(kBlock)
k_wavetable_range(double *result, const float *indexer, int64_t n, int mode, int finite, double wt_start,
                  double wt_end) {
    __shared__ double smin[kBlock], smax[kBlock];
    double lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        bool oob;
        range_take(lo, hi, nan, wt_index((double)indexer[i], mode, finite, wt_start, wt_end, oob));
    }
    if (nan) lo = hi = NAN;
    block_range(lo, hi, smin, smax);
    if (threadIdx.x == 0) {
        result[0] = lo;
        result[1] = hi;
    }
}

// ------------------------------------------------------------------------------------------------
// TimeWarpPE (timewarp_pe.py:147-184): positions[i] = pos + sum(rate[0..i)), pos += sum(rate).
// The float64 prefix sum runs over segments of kTwTile-frame tiles, one workgroup per segment:
//   k_tw_reduce     each segment's sum of rates -> partials[seg]                  (skipped for one segment)
//   k_tw_positions  offset = partials before the segment, in order; block_excl_sum per tile; positions and the
//                   segment's min / max                                           (one segment: also the finish)
//   k_tw_finish     range[0..1] = min / max over the segments; state[0] += sum(partials)
// ------------------------------------------------------------------------------------------------
constexpr int kTwT = 8;
constexpr int kTwTile = kBlock * kTwT;
constexpr int kTwMaxSeg = PGX_TIMEWARP_WORKSPACE_DOUBLES / 3;

__global__ void __launch_bounds__(kBlock)
k_tw_reduce(double *partials, const float *rate, int64_t n, int64_t seg_frames) {
    __shared__ double lds[kBlock / 64];
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    double carry = 0.0;
    for (int64_t base = first; base < end; base += kTwTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kTwT;
        double run = 0.0;
#pragma unroll
        for (int j = 0; j < kTwT; ++j) run = run + ((f0 + j < end) ? (double)rate[f0 + j] : 0.0);
        double tile_total;
        block_excl_sum(run, lds, tile_total);
        carry = carry + tile_total;
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kBlock)
k_tw_positions(double *positions, double *segrange, double *range, double *state, const double *partials,
               const float *rate, int64_t n, int64_t seg_frames) {
    __shared__ double lds[kBlock / 64];
    __shared__ double smin[kBlock], smax[kBlock];
    const double pos = state[0];
    double carry = 0.0;
    for (int s = 0; s < (int)blockIdx.x; ++s) carry = carry + partials[s];
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    double lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    for (int64_t base = first; base < end; base += kTwTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kTwT;
        double before[kTwT];
        double run = 0.0;
#pragma unroll
        for (int j = 0; j < kTwT; ++j) {
            before[j] = run;
            run = run + ((f0 + j < end) ? (double)rate[f0 + j] : 0.0);
        }
        double tile_total;
        const double off = carry + block_excl_sum(run, lds, tile_total);
        carry = carry + tile_total;
#pragma unroll
        for (int j = 0; j < kTwT; ++j) {
            if (f0 + j < end) {
                const double p = pos + (off + before[j]);
                positions[f0 + j] = p;
                range_take(lo, hi, nan, p);
            }
        }
    }
    if (nan) lo = hi = NAN;
    block_range(lo, hi, smin, smax);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            range[0] = lo;
            range[1] = hi;
            state[0] = pos + carry;
        } else {
            segrange[2 * blockIdx.x + 0] = lo;
            segrange[2 * blockIdx.x + 1] = hi;
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_tw_finish(double *range, double *state, const double *partials, const double *segrange, int nseg) {
    __shared__ double smin[kBlock], smax[kBlock];
    double lo = INFINITY, hi = -INFINITY;
    for (int s = threadIdx.x; s < nseg; s += kBlock) {
        const double a = segrange[2 * s], b = segrange[2 * s + 1];
        if (a != a || a < lo) lo = a;
        if (b != b || b > hi) hi = b;
        if (a != a || b != b) lo = hi = NAN;
    }
    block_range(lo, hi, smin, smax);
    if (threadIdx.x == 0) {
        range[0] = lo;
        range[1] = hi;
        double total = 0.0;
        for (int s = 0; s < nseg; ++s) total = total + partials[s];
        state[0] = state[0] + total;
    }
}

// The read itself: index = positions[i], or pos0 + i * rate for a scalar rate; 0 outside the source's extent, either
// side of which may be open (timewarp_pe.py:165-175).
__global__ void __launch_bounds__(kBlock)
k_timewarp(float *out, int64_t n, const double *positions, double pos0, double rate, const float *win,
           int64_t win_start, int64_t win_len, int channels, int cubic, int has_start, double ext_start, int has_end,
           double ext_end) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double index = positions ? positions[i] : pos0 + (double)i * rate;
        const bool oob = (has_start && index < ext_start) || (has_end && index >= ext_end);
        interp_at(out + i * channels, win, win_start, win_len, channels, index, cubic, oob);
    }
}

// ------------------------------------------------------------------------------------------------
// PiecewisePE (piecewise_pe.py:44-75, 164-229).  transition: 0 step, 1 linear, 2 exponential,
// 3 sigmoid, 4 constant_power.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_piecewise(float *out, int64_t start, int64_t n, int channels, const int64_t *times, const double *values,
            int count, int transition, int hold_first, int hold_last) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t t0 = times[0], t_last = times[count - 1];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const int64_t s = start + i;
        float v = 0.0f;
        if (s < t0) {
            if (hold_first) v = (float)values[0];
        } else if (count == 1) {
            if (s == t0 || hold_last) v = (float)values[0];
        } else if (s >= t_last) {
            if (hold_last) v = (float)values[count - 1];
        } else {
            int lo = 0, hi = count;                        // upper_bound: first time > s
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (times[mid] <= s) lo = mid + 1;
                else hi = mid;
            }
            const int j = lo - 1;                          // times[j] <= s < times[j+1]
            const int64_t s0 = times[j], s1 = times[j + 1];
            const double v0 = values[j], v1 = values[j + 1];
            const double t = ((double)s - (double)s0) / (double)(s1 - s0);
            double r;
            if (transition == 0) {
                r = v0;
            } else if (transition == 2 && !(v0 <= 0.0 || v1 <= 0.0)) {
                r = v0 * pow(v1 / v0, t);
            } else if (transition == 3) {
                double x = 6.0 * (2.0 * t - 1.0);
                x = x < -20.0 ? -20.0 : (x > 20.0 ? 20.0 : x);
                r = v0 + (v1 - v0) * (1.0 / (1.0 + exp(-x)));
            } else if (transition == 4) {
                const double a = 0.5 * 3.141592653589793 * t;
                double sn, cs;
                pgx::pgx_sincos(a, sn, cs);
                r = v0 + (v1 - v0) * (v1 >= v0 ? sn : 1.0 - cs);
            } else {
                r = v0 + (v1 - v0) * t;
            }
            v = (float)r;
        }
        for (int c = 0; c < channels; ++c) out[i * channels + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// PortamentoPE (portamento_pe.py:154-254, what its docstring promises): held pitches with a linear glide at each note's
// start.  A line is a table of ramps {at, len, from, to} ordered by `at`; ramp i owns [at_i, at_{i+1}), the last one
// everything from its `at` on, the first also everything before.  Within a ramp the value is k_piecewise's linear
// transition over [at, at + len], held either side.
//
// A workgroup renders runs of kPortaFrames consecutive frames of one line (blockIdx.y), a wave 64 consecutive items of a
// run: an item is a frame of `channels` samples (VEC == 1), or four frames of a mono line written as one 16-byte store
// (VEC == 4: the frames before the line's first 16-byte boundary and those after its last whole vector are the `edge`
// frames of workgroup 0).  Notes last thousands of frames, so a wave almost always lies in one ramp: it searches the
// `at` column once, for its first frame, and looks at the next ramp's `at`; only when that falls inside the wave does
// each lane look for its own ramp, outwards from the wave's (porta_upper_near: the ramp is a few entries on at most).
// A table of up to kPortaLdsRamps ramps is copied to LDS first (16 KiB of a CU's 160: eight workgroups of it fit, which
// is all the waves a CU holds) and everything is read from there; a longer one is read where it lies.  A launch of this
// kind is a chain of dependent round trips -- offsets, table, search, the ramp's values -- and LDS takes the last two out
// of global memory: tools/portamento_probe.py, profiles/portamento_probe.md.
// ------------------------------------------------------------------------------------------------
constexpr int kPortaLdsRamps = 512;
constexpr int kPortaFrames = 1024;

struct PortaTable {
    const int64_t *at, *len;
    const double *from, *to;
    int count;
};

// first index in [lo, count) whose at > s
__device__ __forceinline__ int porta_upper(const int64_t *at, int lo, int count, int64_t s) {
    int hi = count;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (at[mid] <= s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the same, probing lo, lo + 1, lo + 3, lo + 7 ... first: one or two reads when the answer is lo or lo + 1
__device__ __forceinline__ int porta_upper_near(const int64_t *at, int lo, int count, int64_t s) {
    int hi = lo, step = 1;
    while (hi < count && at[hi] <= s) {
        lo = hi + 1;
        hi += step;
        step <<= 1;
    }
    return porta_upper(at, lo, hi < count ? hi : count, s);
}

// frame s of the ramp before index u (u >= 1: the first ramp owns the frames before its `at` too)
__device__ __forceinline__ float porta_value(const PortaTable &T, int u, int64_t s) {
    if (T.count <= 0) return 0.0f;
    const int j = u - 1;
    const double v0 = T.from[j], v1 = T.to[j];
    const int64_t x = s - T.at[j], len = T.len[j];
    if (x <= 0) return (float)v0;
    if (x >= len) return (float)v1;
    return (float)(v0 + (v1 - v0) * ((double)x / (double)len));
}

// one workgroup's share of a line whose table is T (in LDS or in global memory: inlined once for each)
template <int VEC>
__device__ __forceinline__ void porta_render(float *y, int64_t start, int64_t n, int channels, const PortaTable T) {
    auto least1 = [](int u) { return u < 1 ? 1 : u; };
    // VEC == 4: y + head is the line's first 16-byte boundary, `items` whole vectors follow it
    const int64_t head = VEC == 1 ? 0 : [&] {
        const int64_t h = (int64_t)((0 - ((uintptr_t)y >> 2)) & 3);
        return h < n ? h : n;
    }();
    const int64_t items = (n - head) / VEC;
    constexpr int64_t kItems = kPortaFrames / VEC;                  // items per workgroup and run
    constexpr int kRounds = kItems / kBlock;                        // rounds of kBlock items in a run
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    // the workgroup's runs lie side by side, so a wave's frames only move forward: it searches the table once, for its
    // first frame, and from then on outwards from where it was
    const int64_t runs = pgx::ceil_div(items, kItems), per_group = pgx::ceil_div(runs, (int64_t)gridDim.x);
    const int64_t run_first = blockIdx.x * per_group, run_end = run_first + per_group < runs ? run_first + per_group : runs;
    int ur = porta_upper(T.at, 0, T.count, start + head + (run_first * kItems + wave * 64) * VEC);
    for (int64_t run = run_first; run < run_end; ++run) {
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int64_t q0 = run * kItems + r * kBlock + wave * 64;   // wave-uniform
            if (q0 >= items) break;
            const int64_t q_end = q0 + 64 < items ? q0 + 64 : items;
            const int64_t s_lo = start + head + q0 * VEC, s_hi = start + head + q_end * VEC - 1;
            ur = porta_upper_near(T.at, ur, T.count, s_lo);
            const int u = least1(ur);
            const bool one_ramp = u >= T.count || T.at[u] > s_hi;
            const int64_t q = q0 + lane;
            if (q >= items) continue;
            const int64_t f = head + q * VEC;
            float v[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int64_t s = start + f + j;
                v[j] = porta_value(T, one_ramp ? u : porta_upper_near(T.at, u, T.count, s), s);
            }
            if (VEC == 4) {
                *reinterpret_cast<float4 *>(y + f) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                for (int c = 0; c < channels; ++c) y[f * channels + c] = v[0];
            }
        }
    }
    if (VEC == 4 && blockIdx.x == 0) {
        const int64_t tail_first = head + items * VEC;
        const int64_t edge = head + (n - tail_first);               // at most 3 + 3 frames
        if ((int64_t)threadIdx.x < edge) {
            const int64_t f = (int64_t)threadIdx.x < head ? (int64_t)threadIdx.x : tail_first + (threadIdx.x - head);
            y[f] = porta_value(T, least1(porta_upper(T.at, 0, T.count, start + f)), start + f);
        }
    }
}

template <int VEC>
__global__ void __launch_bounds__(kBlock)
k_portamento(float *out, int64_t out_stride, int64_t start, int64_t n, int channels, const int64_t *ramp_at,
             const int64_t *ramp_len, const double *ramp_from, const double *ramp_to, const int32_t *offsets,
             int lds_ramps) {
    __shared__ int64_t lds_at[kPortaLdsRamps], lds_len[kPortaLdsRamps];
    __shared__ double lds_from[kPortaLdsRamps], lds_to[kPortaLdsRamps];
    const int b = blockIdx.y;
    const int first = offsets[b];
    const PortaTable G{ramp_at + first, ramp_len + first, ramp_from + first, ramp_to + first, offsets[b + 1] - first};
    float *y = out + (int64_t)b * out_stride;
    if (G.count <= lds_ramps) {                                     // (the same for every thread of the workgroup)
        for (int k = threadIdx.x; k < G.count; k += kBlock) {
            lds_at[k] = G.at[k];
            lds_len[k] = G.len[k];
            lds_from[k] = G.from[k];
            lds_to[k] = G.to[k];
        }
        __syncthreads();
        porta_render<VEC>(y, start, n, channels, PortaTable{lds_at, lds_len, lds_from, lds_to, G.count});
    } else {
        porta_render<VEC>(y, start, n, channels, G);
    }
}

// ------------------------------------------------------------------------------------------------
// WAV sample formats: what the reference's writer does to a float32 sample on its way into a PCM_16 file.
// wav_writer_pe.py:67 opens the file through python-soundfile, whose SoundFile.__init__ switches libsndfile to
// clipping conversions (SFC_SET_CLIPPING = SF_TRUE); pcm_write_f2les then uses f2s_clip_array (src/pcm.c):
// scaled = x * 0x8000 in float arithmetic; scaled >= 0x7FFF -> 0x7FFF; scaled <= -0x8000 -> -0x8000; otherwise
// lrintf(scaled) in the default rounding mode (half to even).  Reading (s2f_array): x = s / 0x8000.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_f32_to_pcm16(int16_t *out, const float *in, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float scaled = in[i] * 32768.0f;
        int v;
        if (scaled >= 32767.0f) v = 32767;
        else if (scaled <= -32768.0f) v = -32768;
        else if (scaled != scaled) v = 0;                  // NaN: lrintf's result is unspecified; write silence
        else v = (int)rintf(scaled);                       // round half to even
        out[i] = (int16_t)v;
    }
}

__global__ void __launch_bounds__(kBlock)
k_pcm16_to_f32(float *out, const int16_t *in, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        out[i] = (float)in[i] * (1.0f / 32768.0f);
}

// ------------------------------------------------------------------------------------------------
// SpatialPE (spatial_pe.py:94-144, 179-214, 250-286): channel adaptation and stereo panning, float32
// arithmetic like the reference's numpy expressions.  np.mean of a float32 row adds in numpy's blocked order: fewer
// than 8 terms one after the other; 8 .. 128 (kRowMeanMax) terms on eight running sums r[j] += row[8 i + j], joined as
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), the last n % 8 terms added to that one by one; then / n.  (Beyond
// 128 terms numpy halves the row first: not restated here, the entry points refuse such rows.)
// ------------------------------------------------------------------------------------------------
constexpr int kRowMeanMax = 128;

__device__ __forceinline__ float row_mean(const float *row, int from, int to) {
    const int n = to - from;
    const float *a = row + from;
    float acc;
    if (n < 8) {
        acc = a[0];
        for (int c = 1; c < n; ++c) acc = acc + a[c];
    } else {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i + 8 <= n; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
        }
        acc = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) acc = acc + a[i];
    }
    return acc / (float)n;
}

__global__ void __launch_bounds__(kBlock)
k_channel_adapt(float *out, const float *in, int64_t n, int src_ch, int out_ch) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float *x = in + i * src_ch;
        float *y = out + i * out_ch;
        if (src_ch == 1) {
            for (int c = 0; c < out_ch; ++c) y[c] = x[0];
        } else if (out_ch == 1) {
            y[0] = row_mean(x, 0, src_ch);
        } else if (src_ch == 2 && out_ch == 4) {
            const float cs = row_mean(x, 0, 2);
            y[0] = x[0]; y[1] = x[1]; y[2] = cs; y[3] = cs;
        } else if (src_ch == 4 && out_ch == 2) {
            y[0] = x[0]; y[1] = x[1];
        } else if (out_ch >= src_ch) {                  // (as many: a copy, spatial_pe.py:104-105 -- no channels left to fold)
            for (int c = 0; c < src_ch; ++c) y[c] = x[c];
            for (int c = src_ch; c < out_ch; ++c) y[c] = x[src_ch - 1];
        } else {
            for (int c = 0; c < out_ch; ++c) y[c] = x[c];
            y[out_ch - 1] = y[out_ch - 1] + row_mean(x, out_ch, src_ch);
        }
    }
}

// The one expression for a pan gain in the library (k_pan, k_pan_gains, k_pan_bank, k_pan_mix_batch).
// mode 0: linear (L = 1 - pan, R = pan, pan = (az + 90) / 180); 1: constant power (cos / sin of (az + 90) / 2 deg)
__device__ __forceinline__ void pan_gains(float az, int mode, float &lg, float &rg) {
    az = az < -90.0f ? -90.0f : (az > 90.0f ? 90.0f : az);
    if (mode == 0) {
        const float pan = (az + 90.0f) / 180.0f;
        lg = 1.0f - pan;
        rg = pan;
    } else {
        const float ang = ((az + 90.0f) / 2.0f) * (float)(3.141592653589793 / 180.0);   // np.deg2rad in float32
        lg = cosf(ang);
        rg = sinf(ang);
    }
}

__global__ void __launch_bounds__(kBlock)
k_pan(float *out, const float *in, int64_t n, int src_ch, float az_scalar, const float *az_stream, int mode) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float mono = row_mean(in + i * src_ch, 0, src_ch);
        float lg, rg;
        pan_gains(az_stream ? az_stream[i] : az_scalar, mode, lg, rg);
        out[i * 2 + 0] = mono * lg;
        out[i * 2 + 1] = mono * rg;
    }
}

// gains[v] = {lg, rg} of voice v's scalar azimuth: evaluated once per bank, so that a scalar pan costs the kernels below
// no transcendental per frame.  (Two ordinary vector stores per lane.)
__global__ void __launch_bounds__(kBlock) k_pan_gains(float *gains, const float *azimuth, int batch, int mode) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= batch) return;
    float lg, rg;
    pan_gains(azimuth[v], mode, lg, rg);
    gains[2 * v + 0] = lg;
    gains[2 * v + 1] = rg;
}

// k_pan with the voice in the grid (blockIdx.y): row v of `out` is k_pan over row v of `in`, its gains either the pair
// k_pan_gains made of the voice's scalar azimuth or evaluated per frame from the voice's row of `az`.
__global__ void __launch_bounds__(kBlock)
k_pan_bank(float *out, int64_t out_stride, const float *in, int64_t in_stride, int64_t n, int src_ch, const float *gains,
           const float *az, int64_t az_stride, int mode) {
    const int v = blockIdx.y;
    const float *x = in + (int64_t)v * in_stride;
    float *y = out + (int64_t)v * out_stride;
    float lg = 0.0f, rg = 0.0f;
    if (gains) { lg = gains[2 * v + 0]; rg = gains[2 * v + 1]; }
    else az += (int64_t)v * az_stride;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float mono = row_mean(x + i * src_ch, 0, src_ch);
        if (!gains) pan_gains(az[i], mode, lg, rg);
        y[i * 2 + 0] = mono * lg;
        y[i * 2 + 1] = mono * rg;
    }
}

// out[f] = sum_b {float32(mono_b[f] * lg_b[f]), float32(mono_b[f] * rg_b[f])}: SpatialLinear / SpatialConstantPower voices
// fused into the mix (k_pan per voice, then k_mix_batch).  Each product is rounded to float32 before the ordered float32
// addition, the sum starts from voice 0's product (the sign of a zero survives), exactly as when the two kernels run
// one after the other.  One thread per frame carries both channels' sums, so a voice's sample is loaded once.
// (U voices of one frame, gain_mix_chunk's pattern and reason: every load of the chunk is issued before the first
// product -- a lane's additions are ordered, so what keeps HBM busy is the number of loads in flight per lane.  PARTIAL:
// the batch ends inside the chunk; the loads stay unconditional in form (predicated).  MONO: src_ch == 1, the voice's
// sample is one load; else row_mean over the frame's channels.  STREAM: a row of azimuths per voice, else {lg, rg}.)
template <int U, bool FIRST, bool PARTIAL, bool MONO, bool STREAM>
__device__ __forceinline__ void pan_mix_chunk(float &accl, float &accr, const float *in, int64_t in_stride, int64_t f,
                                              int src_ch, const float *gains, const float *az, int64_t az_stride,
                                              int mode, int b, int batch) {
    float xv[U], lv[U], rv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool on = !PARTIAL || b + u < batch;
        const float *row = in + (int64_t)(b + u) * in_stride + f * src_ch;
        if (MONO) xv[u] = on ? row[0] : 0.0f;
        else xv[u] = on ? row_mean(row, 0, src_ch) : 0.0f;
        if (STREAM) {
            lv[u] = on ? az[(int64_t)(b + u) * az_stride + f] : 0.0f;      // (the azimuth: the gains are made of it below)
        } else {
            lv[u] = on ? gains[2 * (b + u) + 0] : 0.0f;
            rv[u] = on ? gains[2 * (b + u) + 1] : 0.0f;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float lg, rg;
        if (STREAM) pan_gains(lv[u], mode, lg, rg);
        else { lg = lv[u]; rg = rv[u]; }
        const float pl = xv[u] * lg, pr = xv[u] * rg;
        if (FIRST && u == 0) { accl = pl; accr = pr; }
        else if (!PARTIAL || b + u < batch) { accl = accl + pl; accr = accr + pr; }
    }
}

template <bool MONO, bool STREAM>
__global__ void __launch_bounds__(kBlock)
k_pan_mix_batch(float *out, const float *in, int64_t in_stride, int batch, int64_t n, int src_ch, const float *gains,
                const float *az, int64_t az_stride, int mode) {
    // (a frame of several channels is several loads per voice already, on row_mean's eight running sums: 4 voices of
    // those at a time -- 32 of them spill)
    constexpr int U = MONO ? 32 : 4;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < n; f += stride) {
        float accl, accr;
        int b = 0;
        if (batch >= U) {
            pan_mix_chunk<U, true, false, MONO, STREAM>(accl, accr, in, in_stride, f, src_ch, gains, az, az_stride, mode, 0, batch);
            for (b = U; b + U <= batch; b += U)
                pan_mix_chunk<U, false, false, MONO, STREAM>(accl, accr, in, in_stride, f, src_ch, gains, az, az_stride, mode, b, batch);
            if (b < batch)
                pan_mix_chunk<U, false, true, MONO, STREAM>(accl, accr, in, in_stride, f, src_ch, gains, az, az_stride, mode, b, batch);
        } else {
            pan_mix_chunk<U, true, true, MONO, STREAM>(accl, accr, in, in_stride, f, src_ch, gains, az, az_stride, mode, 0, batch);
        }
        out[f * 2 + 0] = accl;
        out[f * 2 + 1] = accr;
    }
}

__global__ void __launch_bounds__(kBlock)
k_mono_mean(float *out, const float *in, int64_t n, int src_ch) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
        out[i] = row_mean(in + i * src_ch, 0, src_ch);
}

// How pgx_wavetable launches k_wavetable (also what pgx_wavetable_plan answers): the window is staged when it fits the
// limit and the launch has at least as many gathers to make as floats to stage.
struct WtPlan {
    int staged;
    int grid;
};

WtPlan wavetable_plan(int64_t n, int64_t window_len, int channels, int cubic) {
    const int64_t floats = window_len * channels;
    const int taps = cubic ? 4 : 2;
    WtPlan p{0, pgx::grid_for(n, kBlock)};
    // PGX_WT_LDS_FLOATS (experiments, tools/playback_probe.py): another staging limit; 0 gathers from global memory
    const char *lds_env = getenv("PGX_WT_LDS_FLOATS");
    int64_t lds_floats = lds_env ? atoi(lds_env) : kWtLdsFloats;
    if (lds_floats > kWtLdsMaxFloats) lds_floats = kWtLdsMaxFloats;
    if (floats <= lds_floats && n * taps * channels >= floats) {
        // a workgroup stages the whole window: give each one at least as many gathers as that costs
        p.staged = 1;
        const int64_t per_group = pgx::ceil_div(floats, (int64_t)taps * channels);
        const int64_t groups = n / (per_group > kBlock ? per_group : kBlock);
        if (groups < p.grid) p.grid = groups < 1 ? 1 : (int)groups;
    }
    return p;
}

}  // namespace

extern "C" {

int pgx_channel_adapt(float *out, const float *in, int64_t n, int src_channels, int out_channels) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && src_channels >= 1 && out_channels >= 1, "pgx_channel_adapt: bad argument");
    PGX_CHECK_ARG(src_channels <= kRowMeanMax, "pgx_channel_adapt: more than 128 source channels");
    hipLaunchKernelGGL(k_channel_adapt, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in, n,
                       src_channels, out_channels);
    PGX_LAUNCH_CHECK("k_channel_adapt");
    return PGX_OK;
}

int pgx_pan(float *out, const float *in, int64_t n, int src_channels, float azimuth, const float *azimuth_stream,
            int constant_power) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && src_channels >= 1, "pgx_pan: bad argument");
    PGX_CHECK_ARG(src_channels <= kRowMeanMax, "pgx_pan: more than 128 source channels");
    hipLaunchKernelGGL(k_pan, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in, n,
                       src_channels, azimuth, azimuth_stream, constant_power ? 1 : 0);
    PGX_LAUNCH_CHECK("k_pan");
    return PGX_OK;
}

int pgx_pan_gains(float *gains, const float *azimuth, int batch, int constant_power) {
    PGX_REQUIRE_INIT();
    if (batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(gains && azimuth, "pgx_pan_gains: bad argument");
    hipLaunchKernelGGL(k_pan_gains, dim3(pgx::grid_for(batch, kBlock)), dim3(kBlock), 0, pgx::stream(), gains, azimuth,
                       batch, constant_power ? 1 : 0);
    PGX_LAUNCH_CHECK("k_pan_gains");
    return PGX_OK;
}

int pgx_pan_bank(float *out, int64_t out_stride, const float *in, int64_t in_stride, int batch, int64_t n,
                 int src_channels, const float *gains, const float *azimuth_stream, int64_t az_stride,
                 int constant_power) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in, "pgx_pan_bank: bad argument");
    PGX_CHECK_ARG(src_channels >= 1 && src_channels <= kRowMeanMax, "pgx_pan_bank: source channels outside 1 .. 128");
    PGX_CHECK_ARG((gains != nullptr) != (azimuth_stream != nullptr),
                  "pgx_pan_bank: exactly one of gains and azimuth_stream");
    PGX_CHECK_ARG(out_stride >= n * 2 && in_stride >= n * src_channels && (!azimuth_stream || az_stride >= n),
                  "pgx_pan_bank: stride too small");
    PGX_CHECK_ARG(batch <= 65535, "pgx_pan_bank: batch too large");
    hipLaunchKernelGGL(k_pan_bank, dim3(pgx::grid_for(n, kBlock), batch), dim3(kBlock), 0, pgx::stream(), out, out_stride,
                       in, in_stride, n, src_channels, gains, azimuth_stream, az_stride, constant_power ? 1 : 0);
    PGX_LAUNCH_CHECK("k_pan_bank");
    return PGX_OK;
}

int pgx_pan_mix_batch(float *out, const float *in, int64_t in_stride, int batch, int64_t n, int src_channels,
                      const float *gains, const float *azimuth_stream, int64_t az_stride, int constant_power) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in, "pgx_pan_mix_batch: bad argument");
    PGX_CHECK_ARG(src_channels >= 1 && src_channels <= kRowMeanMax,
                  "pgx_pan_mix_batch: source channels outside 1 .. 128");
    PGX_CHECK_ARG((gains != nullptr) != (azimuth_stream != nullptr),
                  "pgx_pan_mix_batch: exactly one of gains and azimuth_stream");
    PGX_CHECK_ARG(in_stride >= n * src_channels && (!azimuth_stream || az_stride >= n),
                  "pgx_pan_mix_batch: stride too small");
    const dim3 grid(pgx::grid_for(n, kBlock)), block(kBlock);
    const int mode = constant_power ? 1 : 0;
    const bool mono = src_channels == 1;
#define PGX_PAN_MIX(MONO, STREAM)                                                                                   \
    hipLaunchKernelGGL((k_pan_mix_batch<MONO, STREAM>), grid, block, 0, pgx::stream(), out, in, in_stride, batch, n,  \
                       src_channels, gains, azimuth_stream, az_stride, mode)
    if (azimuth_stream) { if (mono) PGX_PAN_MIX(true, true); else PGX_PAN_MIX(false, true); }
    else { if (mono) PGX_PAN_MIX(true, false); else PGX_PAN_MIX(false, false); }
#undef PGX_PAN_MIX
    PGX_LAUNCH_CHECK("k_pan_mix_batch");
    return PGX_OK;
}

int pgx_mono_mean(float *out, const float *in, int64_t n, int src_channels) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && src_channels >= 1, "pgx_mono_mean: bad argument");
    PGX_CHECK_ARG(src_channels <= kRowMeanMax, "pgx_mono_mean: more than 128 source channels");
    hipLaunchKernelGGL(k_mono_mean, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in, n,
                       src_channels);
    PGX_LAUNCH_CHECK("k_mono_mean");
    return PGX_OK;
}


int pgx_interp_lookup(float *out, const float *window, int64_t window_start, int64_t window_len, int channels,
                      int64_t start, int64_t n, double delay_scalar, const float *delay, int cubic, int bounded,
                      double extent_start, double extent_end) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && window && window_len >= 1 && channels >= 1, "pgx_interp_lookup: bad argument");
    hipLaunchKernelGGL(k_interp_lookup, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, window,
                       window_start, window_len, channels, start, n, delay_scalar, delay, cubic, bounded,
                       extent_start, extent_end);
    PGX_LAUNCH_CHECK("k_interp_lookup");
    return PGX_OK;
}

int pgx_wavetable(float *out, const float *indexer, int64_t n, const float *window, int64_t window_start,
                  int64_t window_len, int channels, int cubic, int oob_mode, int finite, double wt_start,
                  double wt_end) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && indexer && window && window_len >= 1 && channels >= 1 && oob_mode >= 0 && oob_mode <= 2,
                  "pgx_wavetable: bad argument");
    const WtPlan plan = wavetable_plan(n, window_len, channels, cubic);
    const size_t lds_bytes = plan.staged ? (size_t)(window_len * channels) * sizeof(float) : 0;
    hipLaunchKernelGGL(k_wavetable, dim3(plan.grid), dim3(kBlock), lds_bytes, pgx::stream(), out, indexer, n, window,
                       window_start, window_len, channels, cubic ? 1 : 0, oob_mode, finite ? 1 : 0, wt_start, wt_end,
                       plan.staged);
    PGX_LAUNCH_CHECK("k_wavetable");
    return PGX_OK;
}

int pgx_wavetable_plan(int64_t n, int64_t window_len, int channels, int cubic, int out[2]) {
    if (n <= 0) {                                            // pgx_wavetable launches nothing
        if (out) out[0] = out[1] = 0;
        return PGX_OK;
    }
    PGX_CHECK_ARG(out && window_len >= 1 && channels >= 1, "pgx_wavetable_plan: bad argument");
    const WtPlan plan = wavetable_plan(n, window_len, channels, cubic);
    out[0] = plan.staged;
    out[1] = plan.grid;
    return PGX_OK;
}

int pgx_wavetable_range(double *result_dev, const float *indexer, int64_t n, int oob_mode, int finite, double wt_start,
                        double wt_end) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(result_dev && indexer && n >= 1 && oob_mode >= 0 && oob_mode <= 2, "pgx_wavetable_range: bad argument");
    hipLaunchKernelGGL(k_wavetable_range, dim3(1), dim3(kBlock), 0, pgx::stream(), result_dev, indexer, n, oob_mode,
                       finite ? 1 : 0, wt_start, wt_end);
    PGX_LAUNCH_CHECK("k_wavetable_range");
    return PGX_OK;
}

int pgx_timewarp_scan(double *positions, double *range_dev, double *state, double *workspace, const float *rate,
                      int64_t n) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(positions && range_dev && state && workspace && rate && n >= 1, "pgx_timewarp_scan: bad argument");
    const int64_t tiles = pgx::ceil_div(n, kTwTile);
    const int64_t tiles_per_seg = pgx::ceil_div(tiles, kTwMaxSeg);
    const int64_t seg_frames = tiles_per_seg * kTwTile;
    const int nseg = (int)pgx::ceil_div(tiles, tiles_per_seg);
    double *partials = workspace, *segrange = workspace + kTwMaxSeg;
    if (nseg > 1) {
        hipLaunchKernelGGL(k_tw_reduce, dim3(nseg), dim3(kBlock), 0, pgx::stream(), partials, rate, n, seg_frames);
        PGX_LAUNCH_CHECK("k_tw_reduce");
    }
    hipLaunchKernelGGL(k_tw_positions, dim3(nseg), dim3(kBlock), 0, pgx::stream(), positions, segrange, range_dev,
                       state, partials, rate, n, seg_frames);
    PGX_LAUNCH_CHECK("k_tw_positions");
    if (nseg > 1) {
        hipLaunchKernelGGL(k_tw_finish, dim3(1), dim3(kBlock), 0, pgx::stream(), range_dev, state, partials, segrange,
                           nseg);
        PGX_LAUNCH_CHECK("k_tw_finish");
    }
    return PGX_OK;
}

int pgx_timewarp(float *out, int64_t n, const double *positions, double pos0, double rate, const float *window,
                 int64_t window_start, int64_t window_len, int channels, int cubic, int has_start,
                 double extent_start, int has_end, double extent_end) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && window && window_len >= 1 && channels >= 1, "pgx_timewarp: bad argument");
    hipLaunchKernelGGL(k_timewarp, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, n, positions,
                       pos0, rate, window, window_start, window_len, channels, cubic ? 1 : 0, has_start ? 1 : 0,
                       extent_start, has_end ? 1 : 0, extent_end);
    PGX_LAUNCH_CHECK("k_timewarp");
    return PGX_OK;
}

int pgx_index_range(double *result_dev, const float *delay, int64_t start, int64_t n) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(result_dev && delay && n >= 1, "pgx_index_range: bad argument");
    hipLaunchKernelGGL(k_index_range, dim3(1), dim3(kBlock), 0, pgx::stream(), result_dev, delay, start, n);
    PGX_LAUNCH_CHECK("k_index_range");
    return PGX_OK;
}

int pgx_stream_range(double *partials_dev, int parts, const float *x, int64_t n) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(partials_dev && x && n >= 1 && parts >= 1 && parts <= 1024, "pgx_stream_range: bad argument");
    hipLaunchKernelGGL(k_stream_range, dim3(parts), dim3(kBlock), 0, pgx::stream(), partials_dev, x, n);
    PGX_LAUNCH_CHECK("k_stream_range");
    return PGX_OK;
}

int pgx_piecewise(float *out, int64_t start, int64_t n, int channels, const int64_t *times, const double *values,
                  int count, int transition, int hold_first, int hold_last) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && times && values && count >= 1 && channels >= 1 && transition >= 0 && transition <= 4,
                  "pgx_piecewise: bad argument");
    hipLaunchKernelGGL(k_piecewise, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, start, n,
                       channels, times, values, count, transition, hold_first, hold_last);
    PGX_LAUNCH_CHECK("k_piecewise");
    return PGX_OK;
}

int pgx_portamento(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                   const int64_t *ramp_at, const int64_t *ramp_len, const double *ramp_from, const double *ramp_to,
                   const int32_t *offsets) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && ramp_at && ramp_len && ramp_from && ramp_to && offsets && channels >= 1,
                  "pgx_portamento: bad argument");
    PGX_CHECK_ARG(out_stride >= n * channels, "pgx_portamento: stride too small");
    PGX_CHECK_ARG(batch <= 65535, "pgx_portamento: batch too large");
    // PGX_PORTA_LDS_RAMPS (experiments, tools/portamento_probe.py): a lower staging limit; 0 searches global memory
    const char *lds_env = getenv("PGX_PORTA_LDS_RAMPS");
    int lds_ramps = lds_env ? atoi(lds_env) : kPortaLdsRamps;
    if (lds_ramps > kPortaLdsRamps) lds_ramps = kPortaLdsRamps;
    // a workgroup takes one run of kPortaFrames frames, or as many side by side as it takes for the whole grid to be on
    // the chip at once (eight workgroups per CU): the table is copied to LDS once per workgroup, not once per run
    const int64_t runs = pgx::ceil_div(n, kPortaFrames), most = pgx::kNumCU * 8 / batch > 1 ? pgx::kNumCU * 8 / batch : 1;
    const dim3 grid((unsigned)pgx::ceil_div(runs, pgx::ceil_div(runs, most)), batch), block(kBlock);
    // one channel: 16-byte stores between each line's first and last 16-byte boundary
    if (channels == 1)
        hipLaunchKernelGGL(k_portamento<4>, grid, block, 0, pgx::stream(), out, out_stride, start, n, channels, ramp_at,
                           ramp_len, ramp_from, ramp_to, offsets, lds_ramps);
    else
        hipLaunchKernelGGL(k_portamento<1>, grid, block, 0, pgx::stream(), out, out_stride, start, n, channels, ramp_at,
                           ramp_len, ramp_from, ramp_to, offsets, lds_ramps);
    PGX_LAUNCH_CHECK("k_portamento");
    return PGX_OK;
}

int pgx_f32_to_pcm16(int16_t *out, const float *in, int64_t n_elems) {
    PGX_REQUIRE_INIT();
    if (n_elems <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in, "pgx_f32_to_pcm16: null pointer");
    hipLaunchKernelGGL(k_f32_to_pcm16, dim3(pgx::grid_for(n_elems, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in,
                       n_elems);
    PGX_LAUNCH_CHECK("k_f32_to_pcm16");
    return PGX_OK;
}

int pgx_pcm16_to_f32(float *out, const int16_t *in, int64_t n_elems) {
    PGX_REQUIRE_INIT();
    if (n_elems <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in, "pgx_pcm16_to_f32: null pointer");
    hipLaunchKernelGGL(k_pcm16_to_f32, dim3(pgx::grid_for(n_elems, kBlock)), dim3(kBlock), 0, pgx::stream(), out, in,
                       n_elems);
    PGX_LAUNCH_CHECK("k_pcm16_to_f32");
    return PGX_OK;
}

}  // extern "C"
