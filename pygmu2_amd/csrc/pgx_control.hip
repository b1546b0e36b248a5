// pgx_control.hip -- the control-signal PEs: SampleHoldPE / TrackHoldPE (pgx_hold), SlewLimiterPE (pgx_slew) and
// FunctionGenPE (pgx_function_gen_pure / pgx_function_gen_bank / pgx_function_gen_stateful).
//
// All three are sequential per-sample loops in the reference.  Here:
//   * a hold is a max-scan over indices ("the last frame whose control sample passed") followed by a gather --
//     integers only, so the result is the reference's bit for bit however the stream is cut into workgroups;
//   * the slew limiter's one-sample update is a continuous, non-decreasing, piecewise-linear map of the carried
//     value, solved time-parallel by Newton rounds over affine pieces exactly as EnvelopePE's attack != release
//     follower is (k_env_newton / k_env_newton_mw in pgx_envelope.hip, restated here for two other maps);
//   * the function generator's carried phase is a float64 prefix sum over workgroup segments, the scheme of
//     pgx_timewarp_scan.
// float64 inside, float32 at the store.

#include <type_traits>

#include "pgx_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;

__host__ __device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64_keep(double old, double v) {     // lanes without a source keep `old`
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}

// Segments of whole tiles for the two-pass scans below, one workgroup each: a tile per segment until there are
// max_seg of them (a render of one tile is one workgroup and one launch).  The workspace holds the segments' partial
// results and, behind them at kCarriedSlot, the reduce pass's copy of the carried value: the apply pass reads that
// copy, so its last workgroup can advance the state without a third launch.
constexpr int kCarriedSlot = PGX_CONTROL_WORKSPACE_DOUBLES - 1;
constexpr int kHoldMaxSeg = 1024, kFgMaxSeg = 256;
static_assert(kHoldMaxSeg <= kCarriedSlot && kFgMaxSeg <= kCarriedSlot, "workspace layout");
struct SegPlan {
    int64_t seg_frames;
    int nseg;
};
inline SegPlan seg_plan(int64_t n, int tile, int max_seg) {
    const int64_t tiles = pgx::ceil_div(n, tile);
    const int64_t per = pgx::ceil_div(tiles, max_seg);
    return SegPlan{per * tile, (int)pgx::ceil_div(tiles, per)};
}

// ================================================================================================
// SampleHoldPE / TrackHoldPE (sample_hold_pe.py:73-85, track_hold_pe.py:73-85):
//     out[i] = src[j],  j = the last index <= i with control[j] > threshold;  the carried value if there is none.
// Pass 1 (k_hold_reduce): each segment's last passing index -> partials[seg] (-1: none); skipped for one segment.
// Pass 2 (k_hold_apply):  carry = max of the partials before the segment; per tile a block-wide inclusive max-scan
//                         of the threads' last passing indices; gather.  The last workgroup advances the carried value.
// Only channel 0 of source and control is read (strides in floats).  VEC: a mono control stream, it and the output
// 16-byte aligned -- a thread's 8 frames are two float4.
// ================================================================================================
constexpr int kHoldT = 8;
constexpr int kHoldTile = kBlock * kHoldT;

template <bool VEC>
__device__ __forceinline__ void hold_load(float (&c)[kHoldT], const float *ctl, int stride, int64_t f0, int64_t end) {
    if (VEC && f0 + kHoldT <= end) {
        const float4 a = *reinterpret_cast<const float4 *>(ctl + f0);
        const float4 b = *reinterpret_cast<const float4 *>(ctl + f0 + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
        c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < kHoldT; ++j) c[j] = (f0 + j < end) ? ctl[(f0 + j) * stride] : -INFINITY;   // never passes
    }
}

// max over the workgroup; `lds` holds kWaves values; two barriers
__device__ __forceinline__ long long block_max_i64(long long v, long long *lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    long long m = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) m = lds[w] > m ? lds[w] : m;
    __syncthreads();
    return m;
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_hold_reduce(long long *partials, const float *ctl, int ctl_stride, int64_t n, int64_t seg_frames, float threshold,
              const double *state) {
    __shared__ long long lds[kWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<double *>(partials)[kCarriedSlot] = state[0];
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    long long last = -1;
    for (int64_t base = first; base < end; base += kHoldTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kHoldT;
        float c[kHoldT];
        hold_load<VEC>(c, ctl, ctl_stride, f0, end);
#pragma unroll
        for (int j = 0; j < kHoldT; ++j)
            if (c[j] > threshold) last = f0 + j;
    }
    last = block_max_i64(last, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = last;
}

template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_hold_apply(float *out, const float *src, int src_stride, const float *ctl, int ctl_stride, int64_t n,
             int64_t seg_frames, float threshold, double *state, const long long *partials) {
    __shared__ long long lds[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // several segments: the reduce pass left a copy of the carried value, state[0] itself is only written here
    const float held_f = (float)(gridDim.x > 1 ? reinterpret_cast<const double *>(partials)[kCarriedSlot] : state[0]);
    long long carry = -1;                                   // the last passing index before the current tile
    for (int s = threadIdx.x; s < (int)blockIdx.x; s += kBlock) {
        const long long p = partials[s];
        carry = p > carry ? p : carry;
    }
    if (gridDim.x > 1) carry = block_max_i64(carry, lds);
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    for (int64_t base = first; base < end; base += kHoldTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kHoldT;
        float c[kHoldT];
        hold_load<VEC>(c, ctl, ctl_stride, f0, end);
        long long loc[kHoldT];
        long long run = -1;
#pragma unroll
        for (int j = 0; j < kHoldT; ++j) {
            if (c[j] > threshold) run = f0 + j;
            loc[j] = run;
        }
        long long inc = run;                                // inclusive max-scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(inc, d, 64);
            if (lane >= d && o > inc) inc = o;
        }
        if (lane == 63) lds[wave] = inc;
        __syncthreads();
        long long before = carry, total = carry;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const long long t = lds[w];
            if (w < wave && t > before) before = t;
            if (t > total) total = t;
        }
        __syncthreads();
        long long ex = __shfl_up(inc, 1, 64);
        if (lane == 0) ex = -1;
        if (ex > before) before = ex;
        float y[kHoldT];
#pragma unroll
        for (int j = 0; j < kHoldT; ++j) {
            const long long at = loc[j] > before ? loc[j] : before;
            y[j] = (f0 + j < end && at >= 0) ? src[at * src_stride] : held_f;
        }
        if (VEC && f0 + kHoldT <= end) {
            *reinterpret_cast<float4 *>(out + f0) = make_float4(y[0], y[1], y[2], y[3]);
            *reinterpret_cast<float4 *>(out + f0 + 4) = make_float4(y[4], y[5], y[6], y[7]);
        } else {
#pragma unroll
            for (int j = 0; j < kHoldT; ++j)
                if (f0 + j < end) out[f0 + j] = y[j];
        }
        carry = total;
    }
    // (one segment: every thread of this workgroup has read state[0] before the barriers above)
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0 && carry >= 0) state[0] = (double)src[carry * src_stride];
}

// ================================================================================================
// SlewLimiterPE (slew_limiter_pe.py:103-135).  One sample's update of the carried value `cur`,
//     LINEAR       d = x - cur;  d = d > up ? up : (d < -dn ? -dn : d);  cur = cur + d       (up, dn = rate / sr)
//     EXPONENTIAL  e = x - cur;  cur = cur + (e > 0 ? up : dn) * e                           (up, dn = min(rate / sr, 1))
// is a continuous, non-decreasing, piecewise-linear map of cur (slopes 1, 0, 1 / 1-up, 1-dn).  A window of
// NW*64*T samples is solved as k_env_newton solves EnvelopePE's follower: every thread steps its T samples literally
// from its current entry level and records the affine piece (A, B) it passed through -- EXPONENTIAL
// A = (1-up)^rises (1-dn)^(live-rises); LINEAR A = 1 if every sample was clipped, else 0: one unclipped sample
// forgets the entry -- a workgroup scan of the pieces gives every thread a new entry, until no entry moves by more
// than 1e-13 of itself.  Each piece is the exact map on a neighbourhood of the entry it was taken at, so thread k's
// entry is final after at most k+1 rounds and the loop ends.  The samples written are literal steps from entries
// within 1e-13 (relative) of the converged ones.
// stats (optional): [0] += inner rounds, [1] += windows solved, [2] += window-level rounds, [3] += fallbacks.
// ================================================================================================
constexpr double kSlewSettled = 1e-13;

template <int NW, int T>
struct SlewShared {
    double a[2][NW], b[2][NW], pu[T + 1], pd[T + 1], entry;
    int moved[2][NW];
    float io[NW * 64 * T + NW * 64];          // a chunk of T frames padded to T+1 words: conflict-free both ways
};

template <int T>
__device__ __forceinline__ void slew_powers(double *pu, double *pd, double up, double dn) {
    double a = 1.0, b = 1.0;
    for (int k = 0; k <= T; ++k) {
        pu[k] = a;
        pd[k] = b;
        a = a * (1.0 - up);
        b = b * (1.0 - dn);
    }
}

// HBM is touched lane-contiguously (element i of thread tid is frame i*threads + tid of the window); the rounds
// want T consecutive frames per thread.  Both directions go through LDS.
template <int NW, int T>
__device__ __forceinline__ void slew_fetch(SlewShared<NW, T> &sh, double (&x)[T], const float *in, int stride,
                                           int64_t base, int64_t n) {
    constexpr int kThreads = NW * 64;
    const int tid = threadIdx.x;
    float raw[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        int64_t f = base + i * kThreads + tid;
        f = f < n ? f : n - 1;
        raw[i] = in[f * stride];
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int k = i * kThreads + tid;
        sh.io[k + k / T] = raw[i];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < T; ++j) x[j] = (double)sh.io[tid * (T + 1) + j];
    __syncthreads();
}

template <int NW, int T>
__device__ __forceinline__ void slew_store(SlewShared<NW, T> &sh, const double (&y)[T], float *out, int64_t base,
                                           int64_t n) {
    constexpr int kThreads = NW * 64;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < T; ++j) sh.io[tid * (T + 1) + j] = (float)y[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int k = i * kThreads + tid;
        if (base + k < n) out[base + k] = sh.io[k + k / T];
    }
    __syncthreads();
}

// The Newton rounds of one window.  x: the thread's samples, live: how many of them exist, e_in: the window's entry
// level.  Leaves the samples in y and the window's piece (exit = a_tot * e_in + b_tot); returns the rounds taken.
template <int NW, int T, int MODE>
__device__ __forceinline__ int slew_rounds(SlewShared<NW, T> &sh, const double (&x)[T], int live, double e_in,
                                           double up, double dn, double (&y)[T], double &a_tot, double &b_tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double entry = e_in;
    int round = 0;
    for (; round <= NW * 64 + 1; ++round) {
        double cur = entry;
        int count = 0;                                   // LINEAR: clipped samples; EXPONENTIAL: rising samples
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const bool on = j < live;
            double stepped;
            bool flag;
            if (MODE == 0) {
                double d = x[j] - cur;
                flag = d > up || d < -dn;
                d = d > up ? up : (d < -dn ? -dn : d);
                stepped = cur + d;
            } else {
                const double e = x[j] - cur;
                flag = e > 0.0;
                stepped = cur + (flag ? up : dn) * e;
            }
            count += (on && flag) ? 1 : 0;
            cur = on ? stepped : cur;
            y[j] = cur;
        }
        double a = (MODE == 0) ? (count == live ? 1.0 : 0.0) : sh.pu[count] * sh.pd[live - count];
        double b = __builtin_fma(-a, entry, cur);
        // inclusive scan of the pieces over the wave (lanes without a source see the identity)
#define PGX_SLEW_STEP(CTRL, MASK)                                           \
        {                                                                   \
            const double ao = dpp_f64_keep<CTRL, MASK>(1.0, a);             \
            const double bo = dpp_f64_keep<CTRL, MASK>(0.0, b);             \
            b = __builtin_fma(a, bo, b);                                    \
            a = a * ao;                                                     \
        }
        PGX_SLEW_STEP(0x111, 0xf) PGX_SLEW_STEP(0x112, 0xf) PGX_SLEW_STEP(0x114, 0xf) PGX_SLEW_STEP(0x118, 0xf)
        PGX_SLEW_STEP(0x142, 0xa) PGX_SLEW_STEP(0x143, 0xc)
#undef PGX_SLEW_STEP
        const int buf = round & 1;                       // LDS double-buffered by round parity: two barriers a round
        if (lane == 63) {
            sh.a[buf][wave] = a;
            sh.b[buf][wave] = b;
        }
        __syncthreads();
        double cw = e_in, ta = 1.0, tb = 0.0;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            const double wa = sh.a[buf][v], wb = sh.b[buf][v];
            if (v < wave) cw = __builtin_fma(wa, cw, wb);
            tb = __builtin_fma(wa, tb, wb);
            ta = ta * wa;
        }
        a_tot = ta;
        b_tot = tb;
        const double aex = dpp_f64_keep<0x138, 0xf>(1.0, a);                // wave_shr:1 -> exclusive
        const double bex = dpp_f64_keep<0x138, 0xf>(0.0, b);
        const double fresh = __builtin_fma(aex, cw, bex);
        const bool moved = live > 0 && fabs(fresh - entry) > kSlewSettled * (fabs(fresh) + fabs(entry));
        entry = fresh;
        const bool wave_moved = __ballot(moved) != 0ull;
        if (lane == 0) sh.moved[buf][wave] = wave_moved ? 1 : 0;
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) any |= sh.moved[buf][v];
        if (!any) break;
    }
    return round + 1;
}

// One workgroup, window after window from the carried value.
template <int NW, int T, int MODE>
__global__ void __launch_bounds__(NW * 64)
k_slew(float *out, const float *in, int in_stride, int64_t n, double up, double dn, double *state,
       const int *run_flag, int *stats) {
    if (run_flag != nullptr && *run_flag == 0) return;       // armed only when the all-windows form gave up
    __shared__ SlewShared<NW, T> sh;
    constexpr int kWindow = NW * 64 * T;
    const int tid = threadIdx.x;
    double e_in = state[0];
    if (tid == 0) slew_powers<T>(sh.pu, sh.pd, up, dn);
    __syncthreads();
    int rounds = 0, windows = 0;
    for (int64_t base = 0; base < n; base += kWindow) {
        const int64_t f0 = base + (int64_t)tid * T;
        const int live = (n - f0 >= T) ? T : (n - f0 > 0 ? (int)(n - f0) : 0);
        double x[T], y[T], a_tot, b_tot;
        slew_fetch<NW, T>(sh, x, in, in_stride, base, n);
        rounds += slew_rounds<NW, T, MODE>(sh, x, live, e_in, up, dn, y, a_tot, b_tot);
        ++windows;
        slew_store<NW, T>(sh, y, out, base, n);
        e_in = __builtin_fma(a_tot, e_in, b_tot);          // composition of all pieces (dead samples: the identity)
    }
    if (tid == 0) {
        state[0] = e_in;
        if (stats) {
            atomicAdd(stats + 0, rounds);
            atomicAdd(stats + 1, windows);
            if (run_flag) atomicAdd(stats + 3, 1);
        }
    }
}

// A LONG render: all windows at once, one launch per Newton round over the windows' entry levels (k_env_newton_mw's
// scheme).  Round 0: every window is solved from the carried value and publishes its piece.  Round r: a window folds
// the pieces of the windows before it (published in round r-1) onto the carried value; if that is the entry its
// samples were rendered from (1e-13) it republishes its piece, otherwise it renders again and raises the round's
// "moved" flag.  No window moved in a round: converged, later launches return at once.  If the rounds run out,
// k_slew_mw_finish arms k_slew, which renders the block from the carried value: the result never depends on
// convergence.
constexpr int kSlewMwRounds = 8;
constexpr int kSlewNW = 8, kSlewT = 16, kSlewWindow = kSlewNW * 64 * kSlewT;          // 8192
constexpr int64_t kSlewMwMinFrames = 16 * (int64_t)kSlewWindow;
struct SlewMwCtl {
    int moved[kSlewMwRounds + 1];
    int fallback;
};

// the carried value pushed through pieces [0, count): wave 0 only; lanes compose runs of pieces, then a scan
__device__ __forceinline__ double slew_fold(const double *pa, const double *pb, int count, double carried) {
    const int lane = threadIdx.x & 63;
    double a = 1.0, b = 0.0;
    const int per = (count + 63) / 64;
    const int v0 = lane * per, v1 = (v0 + per < count) ? v0 + per : count;
    for (int v = v0; v < v1; ++v) {
        const double av = pa[v], bv = pb[v];
        b = __builtin_fma(av, b, bv);
        a = a * av;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double ao = __shfl_up(a, d, 64), bo = __shfl_up(b, d, 64);
        if (lane >= d) {
            b = __builtin_fma(a, bo, b);
            a = a * ao;
        }
    }
    return __builtin_fma(a, carried, b);                   // lane 63 holds the whole composition
}

template <int MODE>
__global__ void __launch_bounds__(kSlewNW * 64)
k_slew_mw(float *out, const float *in, int in_stride, int64_t n, double up, double dn, const double *state,
          int round, int nwin, double *pa_buf, double *pb_buf, double *guess, SlewMwCtl *ctl, int *stats) {
    constexpr int NW = kSlewNW, T = kSlewT;
    __shared__ SlewShared<NW, T> sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x;
    if (round > 0 && ctl->moved[round - 1] == 0) return;         // converged in an earlier round
    const int64_t base = (int64_t)w * kSlewWindow;
    const int cur = round & 1, prev = cur ^ 1;
    double *pa_cur = pa_buf + (int64_t)cur * nwin, *pb_cur = pb_buf + (int64_t)cur * nwin;
    const double *pa_prev = pa_buf + (int64_t)prev * nwin, *pb_prev = pb_buf + (int64_t)prev * nwin;
    if (wave == 0) {
        const double e = slew_fold(pa_prev, pb_prev, round > 0 ? w : 0, state[0]);
        if (lane == 63) sh.entry = e;
    }
    if (tid == 64) slew_powers<T>(sh.pu, sh.pd, up, dn);
    __syncthreads();
    const double e_in = sh.entry;
    if (round > 0) {
        const double g = guess[w];
        if (fabs(e_in - g) <= kSlewSettled * (fabs(e_in) + fabs(g))) {      // rendered from this entry already
            if (tid == 0) {
                pa_cur[w] = pa_prev[w];
                pb_cur[w] = pb_prev[w];
            }
            return;
        }
    }
    if (tid == 0) {
        ctl->moved[round] = 1;
        guess[w] = e_in;
    }
    const int64_t f0 = base + (int64_t)tid * T;
    const int live = (n - f0 >= T) ? T : (n - f0 > 0 ? (int)(n - f0) : 0);
    double x[T], y[T], a_tot, b_tot;
    slew_fetch<NW, T>(sh, x, in, in_stride, base, n);
    const int rounds = slew_rounds<NW, T, MODE>(sh, x, live, e_in, up, dn, y, a_tot, b_tot);
    slew_store<NW, T>(sh, y, out, base, n);
    if (tid == 0) {
        pa_cur[w] = a_tot;
        pb_cur[w] = b_tot;
        if (stats) {
            atomicAdd(stats + 0, rounds);
            atomicAdd(stats + 1, 1);
        }
    }
}

// After the last round: converged -> the carried value pushed through every piece; otherwise arm k_slew.
__global__ void __launch_bounds__(64)
k_slew_mw_finish(double *state, int nwin, const double *pa_buf, const double *pb_buf, SlewMwCtl *ctl, int rounds,
                 int *stats) {
    int last = 0;                                                 // the last round in which a window moved
    for (int r = 0; r < rounds; ++r)
        if (ctl->moved[r]) last = r;
    if (stats && threadIdx.x == 0) atomicAdd(stats + 2, last + 1);
    if (last >= rounds - 1) {                                     // no later round ran and found nothing to move
        if (threadIdx.x == 0) ctl->fallback = 1;
        return;
    }
    const int cur = (last + 1) & 1;                               // that later round republished every piece
    const double e = slew_fold(pa_buf + (int64_t)cur * nwin, pb_buf + (int64_t)cur * nwin, nwin, state[0]);
    if (threadIdx.x == 63) state[0] = e;
}

// ================================================================================================
// FunctionGenPE (function_gen_pe.py:121-193).
// ================================================================================================
// _piecewise_linear (:121-155) for one sample; duty already clipped to [0, 1]
__device__ __forceinline__ double fg_saw(double p, double duty) {
    const double eps = 1e-12;
    if (duty <= eps) return 2.0 * p - 1.0;
    if (duty >= 1.0 - eps) return 1.0 - 2.0 * p;
    double a = 1.0 - duty;
    a = a < eps ? eps : (a > 1.0 - eps ? 1.0 - eps : a);
    if (p < a) return -1.0 + 2.0 * (p / a);
    return 1.0 - 2.0 * ((p - a) / (1.0 - a));
}
__device__ __forceinline__ double fg_wave(double p, double duty, int saw) {
    duty = duty < 0.0 ? 0.0 : (duty > 1.0 ? 1.0 : duty);                    // np.clip(duty, 0, 1) (:184)
    return saw ? fg_saw(p, duty) : (p < duty ? 1.0 : -1.0);
}

// all parameters scalar: phase = mod(mod(n * dt, 1) + ph, 1) (:166-180) -- the sample of frame `frame`, what
// k_fg_pure and k_fg_bank both store
__device__ __forceinline__ float fg_pure_sample(int64_t frame, double dt, double ph, double duty, int saw) {
    const double base = pgx::pgx_mod1((double)frame * dt);
    return (float)fg_wave(pgx::pgx_mod1(base + ph), duty, saw);
}

// ... `channels` copies of the column
__global__ void __launch_bounds__(kBlock)
k_fg_pure(float *out, int64_t start, int64_t n, int channels, double dt, double ph, double duty, int saw) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const float y = fg_pure_sample(start + i, dt, ph, duty, saw);
        for (int c = 0; c < channels; ++c) out[i * channels + c] = y;
    }
}

// K of them in one launch (voice_bank.py): instance blockIdx.y under params[blockIdx.y], its row out_stride floats
// after the one before.  A workgroup renders tiles of kFgBankTile = 1024 frames, kFgBankT per thread.  A mono row that
// is 16-byte aligned: a thread owns 4 consecutive frames and stores one float4 (the layout of k_sine / k_periodic_gate;
// the row's last, partial group as scalars).  Any other row: a thread owns frames tid, tid + 256, ... of the tile, so
// that a wave's scalar stores are consecutive (k_fg_pure's layout), `channels` copies a frame.
constexpr int kFgBankT = 4;
constexpr int kFgBankTile = kBlock * kFgBankT;

__global__ void __launch_bounds__(kBlock)
k_fg_bank(float *out, int64_t out_stride, int64_t start, int64_t n, int channels, int saw,
          const pgx_function_gen_params *params) {
    const pgx_function_gen_params p = params[blockIdx.y];
    float *o = out + (int64_t)blockIdx.y * out_stride;
    const bool vec = channels == 1 && aligned16(o);
    const int64_t stride = (int64_t)gridDim.x * kFgBankTile;
    for (int64_t tile = (int64_t)blockIdx.x * kFgBankTile; tile < n; tile += stride) {
        if (vec) {
            const int64_t f0 = tile + (int64_t)threadIdx.x * kFgBankT;
            if (f0 >= n) continue;
            float y[kFgBankT];
#pragma unroll
            for (int j = 0; j < kFgBankT; ++j) y[j] = fg_pure_sample(start + f0 + j, p.dt, p.phase, p.duty, saw);
            if (f0 + kFgBankT <= n) {
                *reinterpret_cast<float4 *>(o + f0) = make_float4(y[0], y[1], y[2], y[3]);
            } else {
#pragma unroll
                for (int j = 0; j < kFgBankT; ++j)
                    if (f0 + j < n) o[f0 + j] = y[j];
            }
            continue;
        }
#pragma unroll
        for (int j = 0; j < kFgBankT; ++j) {
            const int64_t f = tile + (int64_t)j * kBlock + threadIdx.x;
            if (f < n) {
                const float y = fg_pure_sample(start + f, p.dt, p.phase, p.duty, saw);
                for (int c = 0; c < channels; ++c) o[f * channels + c] = y;
            }
        }
    }
}

// any PE parameter (:169-177): base = mod(phase0 + [0, cumsum(dt)[:-1]], 1), phase0' = mod(phase0 + sum(dt), 1).
//   k_fg_reduce  each segment's sum of dt -> partials[seg]                          (skipped for one segment)
//   k_fg_apply   offset = the partials before the segment, in order; block_excl_sum per tile; the samples; the last
//                workgroup, whose running sum is then the sum of all partials, advances the carried phase
constexpr int kFgT = 8;
constexpr int kFgTile = kBlock * kFgT;

__device__ __forceinline__ double fg_dt_run(double (&before)[kFgT], const float *freq, double freq_scalar, double sr,
                                            int64_t f0, int64_t end, int64_t n) {
    float f_in[kFgT];
    if (freq) {
#pragma unroll
        for (int j = 0; j < kFgT; ++j) f_in[j] = freq[(f0 + j < n) ? f0 + j : n - 1];
    }
    double run = 0.0;
#pragma unroll
    for (int j = 0; j < kFgT; ++j) {
        before[j] = run;
        const double f = freq ? (double)f_in[j] : freq_scalar;
        run = run + ((f0 + j < end) ? f / sr : 0.0);
    }
    return run;
}

__global__ void __launch_bounds__(kBlock)
k_fg_reduce(double *partials, const float *freq, double freq_scalar, double sr, int64_t n, int64_t seg_frames,
            const double *state) {
    __shared__ double lds[kWaves];
    if (blockIdx.x == 0 && threadIdx.x == 0) partials[kCarriedSlot] = state[0];
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    double carry = 0.0;
    for (int64_t base = first; base < end; base += kFgTile) {
        double before[kFgT], tile_total;
        const double run = fg_dt_run(before, freq, freq_scalar, sr, base + (int64_t)threadIdx.x * kFgT, end, n);
        pgx::block_excl_sum<kWaves>(run, lds, tile_total);
        carry = carry + tile_total;
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kBlock)
k_fg_apply(float *out, int64_t n, int channels, int saw, double sr, double freq_scalar, double duty_scalar,
           double phase_scalar, const float *freq, const float *duty, const float *phase, double *state,
           const double *partials, int64_t seg_frames) {
    __shared__ double lds[kWaves];
    const double phase0 = gridDim.x > 1 ? partials[kCarriedSlot] : state[0];
    double carry = 0.0;
    for (int s = 0; s < (int)blockIdx.x; ++s) carry = carry + partials[s];
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    for (int64_t base = first; base < end; base += kFgTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kFgT;
        double before[kFgT], tile_total;
        const double run = fg_dt_run(before, freq, freq_scalar, sr, f0, end, n);
        const double off = carry + pgx::block_excl_sum<kWaves>(run, lds, tile_total);
        carry = carry + tile_total;
#pragma unroll
        for (int j = 0; j < kFgT; ++j) {
            if (f0 + j >= end) break;
            const double b = pgx::pgx_mod1(phase0 + (off + before[j]));
            const double p = pgx::pgx_mod1(b + (phase ? (double)phase[f0 + j] : phase_scalar));
            const float y = (float)fg_wave(p, duty ? (double)duty[f0 + j] : duty_scalar, saw);
            for (int c = 0; c < channels; ++c) out[(f0 + j) * channels + c] = y;
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) state[0] = pgx::pgx_mod1(phase0 + carry);
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int pgx_hold(float *out, const float *src, int src_channels, const float *control, int control_channels, int64_t n,
             float threshold, double *state, void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && src && control && state && workspace && src_channels >= 1 && control_channels >= 1,
                  "pgx_hold: bad argument");
    const SegPlan p = seg_plan(n, kHoldTile, kHoldMaxSeg);
    long long *partials = static_cast<long long *>(workspace);
    const bool vec = control_channels == 1 && aligned16(out) && aligned16(control);
    if (p.nseg > 1) {
        if (vec)
            hipLaunchKernelGGL(k_hold_reduce<true>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), partials, control,
                               control_channels, n, p.seg_frames, threshold, (const double *)state);
        else
            hipLaunchKernelGGL(k_hold_reduce<false>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), partials, control,
                               control_channels, n, p.seg_frames, threshold, (const double *)state);
        PGX_LAUNCH_CHECK("k_hold_reduce");
    }
    if (vec)
        hipLaunchKernelGGL(k_hold_apply<true>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), out, src, src_channels,
                           control, control_channels, n, p.seg_frames, threshold, state, partials);
    else
        hipLaunchKernelGGL(k_hold_apply<false>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), out, src, src_channels,
                           control, control_channels, n, p.seg_frames, threshold, state, partials);
    PGX_LAUNCH_CHECK("k_hold_apply");
    return PGX_OK;
}

size_t pgx_slew_scratch_bytes(int64_t n) {
    if (n < kSlewMwMinFrames) return sizeof(double);
    const size_t nwin = (size_t)pgx::ceil_div(n, kSlewWindow);
    return (5 * nwin + 8) * sizeof(double);                      // pieces (2 x 2), entries, control
}

int pgx_slew(float *out, const float *in, int in_channels, int64_t n, int mode, double up, double down,
             double *state, double *scratch, int *stats) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && state && scratch && in_channels >= 1 && (mode == 0 || mode == 1) && up > 0.0 &&
                      down > 0.0, "pgx_slew: bad argument");
    PGX_CHECK_ARG(mode == 0 || (up <= 1.0 && down <= 1.0), "pgx_slew: exponential coefficients must be <= 1");
    const int *run_flag = nullptr;
    const int64_t nwin64 = pgx::ceil_div(n, kSlewWindow);
    if (n >= kSlewMwMinFrames && nwin64 <= 0x7fffffff) {
        const int nwin = (int)nwin64;
        double *pa_buf = scratch, *pb_buf = scratch + 2 * (size_t)nwin, *guess = scratch + 4 * (size_t)nwin;
        SlewMwCtl *ctl = reinterpret_cast<SlewMwCtl *>(scratch + 5 * (size_t)nwin);
        if (int rc = pgx_memset(ctl, 0, sizeof(SlewMwCtl))) return rc;
        // (PGX_SLEW_MW_ROUNDS=1 makes every long block give up: the test of the fallback)
        static const int rounds_env = getenv("PGX_SLEW_MW_ROUNDS") ? atoi(getenv("PGX_SLEW_MW_ROUNDS")) : kSlewMwRounds;
        const int rounds = rounds_env < 1 ? 1 : (rounds_env > kSlewMwRounds ? kSlewMwRounds : rounds_env);
        for (int r = 0; r < rounds; ++r) {
            if (mode == 0)
                hipLaunchKernelGGL(k_slew_mw<0>, dim3(nwin), dim3(kSlewNW * 64), 0, pgx::stream(), out, in, in_channels,
                                   n, up, down, (const double *)state, r, nwin, pa_buf, pb_buf, guess, ctl, stats);
            else
                hipLaunchKernelGGL(k_slew_mw<1>, dim3(nwin), dim3(kSlewNW * 64), 0, pgx::stream(), out, in, in_channels,
                                   n, up, down, (const double *)state, r, nwin, pa_buf, pb_buf, guess, ctl, stats);
            PGX_LAUNCH_CHECK("k_slew_mw");
        }
        hipLaunchKernelGGL(k_slew_mw_finish, dim3(1), dim3(64), 0, pgx::stream(), state, nwin, (const double *)pa_buf,
                           (const double *)pb_buf, ctl, rounds, stats);
        PGX_LAUNCH_CHECK("k_slew_mw_finish");
        run_flag = &ctl->fallback;                // the sequential kernel below runs only if that gave up
    }
#define PGX_SLEW_LAUNCH(NW, T)                                                                                      \
    do {                                                                                                            \
        if (mode == 0)                                                                                              \
            hipLaunchKernelGGL((k_slew<NW, T, 0>), dim3(1), dim3(NW * 64), 0, pgx::stream(), out, in, in_channels, n, \
                               up, down, state, run_flag, stats);                                                   \
        else                                                                                                        \
            hipLaunchKernelGGL((k_slew<NW, T, 1>), dim3(1), dim3(NW * 64), 0, pgx::stream(), out, in, in_channels, n, \
                               up, down, state, run_flag, stats);                                                   \
    } while (0)
    if (n <= 1024) PGX_SLEW_LAUNCH(4, 4);
    else PGX_SLEW_LAUNCH(kSlewNW, kSlewT);
#undef PGX_SLEW_LAUNCH
    PGX_LAUNCH_CHECK("k_slew");
    return PGX_OK;
}

int pgx_function_gen_pure(float *out, int64_t start, int64_t n, int channels, int sawtooth, double dt, double phase,
                          double duty) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && channels >= 1, "pgx_function_gen_pure: bad argument");
    hipLaunchKernelGGL(k_fg_pure, dim3(pgx::grid_for(n, kBlock)), dim3(kBlock), 0, pgx::stream(), out, start, n,
                       channels, dt, phase, duty, sawtooth ? 1 : 0);
    PGX_LAUNCH_CHECK("k_fg_pure");
    return PGX_OK;
}

int pgx_function_gen_bank(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                          int sawtooth, const pgx_function_gen_params *params) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && channels >= 1, "pgx_function_gen_bank: bad argument");
    PGX_CHECK_ARG(batch == 1 || out_stride >= n * channels, "pgx_function_gen_bank: out_stride too small");
    PGX_CHECK_ARG(batch <= 65535, "pgx_function_gen_bank: batch too large");
    dim3 grid(pgx::grid_for(pgx::ceil_div(n, kFgBankT), kBlock), batch);
    hipLaunchKernelGGL(k_fg_bank, grid, dim3(kBlock), 0, pgx::stream(), out, out_stride, start, n, channels,
                       sawtooth ? 1 : 0, params);
    PGX_LAUNCH_CHECK("k_fg_bank");
    return PGX_OK;
}

int pgx_function_gen_stateful(float *out, int64_t n, int channels, int sawtooth, double sample_rate, double freq,
                              double duty, double phase, const float *freq_stream, const float *duty_stream,
                              const float *phase_stream, double *state, double *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && state && workspace && channels >= 1 && sample_rate > 0,
                  "pgx_function_gen_stateful: bad argument");
    const SegPlan p = seg_plan(n, kFgTile, kFgMaxSeg);
    if (p.nseg > 1) {
        hipLaunchKernelGGL(k_fg_reduce, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), workspace, freq_stream, freq,
                           sample_rate, n, p.seg_frames, (const double *)state);
        PGX_LAUNCH_CHECK("k_fg_reduce");
    }
    hipLaunchKernelGGL(k_fg_apply, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), out, n, channels, sawtooth ? 1 : 0,
                       sample_rate, freq, duty, phase, freq_stream, duty_stream, phase_stream, state,
                       (const double *)workspace, p.seg_frames);
    PGX_LAUNCH_CHECK("k_fg_apply");
    return PGX_OK;
}

}  // extern "C"
