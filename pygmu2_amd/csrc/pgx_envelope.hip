// pgx_envelope.hip -- EnvelopePE (envelope_pe.py:128-271): a 1-state map; with attack != release a walk over regimes.
// Scan primitives: pgx_scan.h.

#include <cstdlib>
#include <type_traits>

#include "pgx_common.h"
#include "pgx_scan.h"

namespace {

// ================================================================================================
// EnvelopePE (envelope_pe.py:128-271)
// ================================================================================================
// Detector: |x| (peak) or the block-local centred running RMS of scipy.ndimage.uniform_filter1d(x^2,
// size=window, mode='nearest') (envelope_pe.py:208-225).  Output float64 (frames, channels).
// RMS sums each window as head + whole 64-frame blocks + tail (k_env_blocks holds the block sums of squares),
// with the 'nearest' edge samples weighted by how often the clamped window repeats them.
constexpr int kEnvBlock = 64;

__global__ void __launch_bounds__(kBlock)
k_env_blocks(double *blocks, const float *in, int64_t n, int channels) {
    const int lane = threadIdx.x & 63;
    const int64_t nblk = (n + kEnvBlock - 1) / kEnvBlock;
    const int64_t item = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);          // one wave per (block, channel)
    if (item >= nblk * channels) return;
    const int64_t b = item / channels;
    const int c = (int)(item - b * channels);
    const int64_t f = b * kEnvBlock + lane;
    double v = 0.0;
    if (f < n) {
        v = (double)in[f * channels + c];
        v = v * v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d, 64);
    if (lane == 0) blocks[item] = v;
}

__global__ void __launch_bounds__(kBlock)
k_env_detect(double *det, const float *in, const double *blocks, int64_t n, int channels, int rms_window,
             int64_t period) {
    const int64_t total = n * channels;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    auto sq = [&](int64_t f, int c) {
        const double v = (double)in[f * channels + c];
        return v * v;
    };
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += stride) {
        const int64_t i = e / channels;
        const int c = (int)(e - i * channels);
        if (rms_window <= 0) {
            det[e] = fabs((double)in[e]);
            continue;
        }
        // window [i - size/2, i - size/2 + size) with indices clamped to the block ('nearest').  The block is the
        // caller's: when a look-ahead window renders several of the caller's blocks at once (`period` frames each)
        // the detector restarts at every one of their edges, as the reference's per-block filter does
        int64_t p0 = 0, p1 = n;
        if (period > 0) {
            p0 = (i / period) * period;
            p1 = p0 + period < n ? p0 + period : n;
        }
        int64_t lo = i - rms_window / 2, hi = lo + rms_window;
        double acc = 0.0;
        if (lo < p0) {
            acc = acc + (double)(p0 - lo) * sq(p0, c);
            lo = p0;
        }
        if (hi > p1) {
            acc = acc + (double)(hi - p1) * sq(p1 - 1, c);
            hi = p1;
        }
        const int64_t b0 = (lo + kEnvBlock - 1) / kEnvBlock, b1 = hi / kEnvBlock;        // whole blocks [b0, b1)
        if (b0 < b1) {
            for (int64_t f = lo; f < b0 * kEnvBlock; ++f) acc = acc + sq(f, c);
            for (int64_t b = b0; b < b1; ++b) acc = acc + blocks[b * channels + c];
            for (int64_t f = b1 * kEnvBlock; f < hi; ++f) acc = acc + sq(f, c);
        } else {
            for (int64_t f = lo; f < hi; ++f) acc = acc + sq(f, c);
        }
        det[e] = sqrt(acc / (double)rms_window);
    }
}

constexpr int kEnvT = 8;
constexpr int kEnvTile = kBlock * kEnvT;

// attack == release (envelope_pe.py:167-180): one-pole lfilter  y = z + c*x;  z = (1-c)*y.
__global__ void __launch_bounds__(kBlock)
k_env_onepole(float *out, const double *det, int64_t n, int channels, double coeff, double *state) {
    __shared__ double lds[kWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ch = blockIdx.x;
    const double lam = 1.0 - coeff;
    double lamp[6], lam_wave, lam_lane = 1.0;
    {
        double l = lam;
#pragma unroll
        for (int s = 1; s < kEnvT; s <<= 1) l = l * l;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            lamp[k] = l;
            if (lane & (1 << k)) lam_lane = lam_lane * l;
            l = l * l;
        }
        lam_wave = l;
    }
    double carry = state[ch];
    double final_y = 0.0;
    bool have_final = false;
    for (int64_t base = 0; base < n; base += kEnvTile) {
        const int64_t f0 = base + (int64_t)tid * kEnvT;
        double xs[kEnvT];
        double e = 0.0;
#pragma unroll
        for (int j = 0; j < kEnvT; ++j) {
            xs[j] = (f0 + j < n) ? det[(f0 + j) * channels + ch] : 0.0;
            // dead samples must act as the identity map, so the zero-state response only folds live ones
            if (f0 + j < n) e = lam * e + coeff * xs[j];
            else e = lam * e;
        }
        double y = block_scan_scalar_affine(e, lamp, lam_wave, lam_lane, lds, carry);
        float yf[kEnvT];
#pragma unroll
        for (int j = 0; j < kEnvT; ++j) {
            const double z = lam * y;
            const double yn = z + coeff * xs[j];
            yf[j] = (float)yn;
            if (f0 + j < n) y = yn;
            if (f0 + j == n - 1) {
                final_y = yn;
                have_final = true;
            }
        }
        store_frames<kEnvT>(out, f0, n, channels, ch, yf);
    }
    if (have_final) state[ch] = final_y;
}


// attack != release (envelope_pe.py:259-271), time-parallel.  One sample's update
//     e' = e + c(e) * (t - e),   c = attack if t > e else release
// is a continuous, increasing, two-piece linear map of e, so a thread's T samples compose to a piecewise linear
// map whose piece around a given entry level is found by stepping the samples literally from that level.  A
// window of NW*64*T samples is solved by Newton's method on that piecewise linear system: every thread steps its
// samples from its current entry level (reference arithmetic), recording the affine piece (A, B) it passed
// through; a workgroup scan of the pieces gives every thread a new entry level; repeat until no entry level
// moves by more than 1e-13 of itself.  Thread k's entry is final after at most k+1 rounds (it only depends on
// threads before it), so the loop ends; in practice it takes 2..6 rounds (semismooth Newton).  The samples written
// are literal steps from entry levels within 1e-13 of the converged ones: against the sequential reference they
// differ by that much (float32 output resolves 6e-8).  `det` == nullptr: peak detection fused (|in|).
constexpr double kEnvSettled = 1e-13;
template <int NW, int T, bool PEAK>
__global__ void __launch_bounds__(NW * 64)
k_env_newton(float *out, const float *in, const double *det, int64_t n, int channels, double attack_coeff,
             double release_coeff, double *state, const int *run_flag) {
    if (run_flag != nullptr && *run_flag == 0) return;       // armed only when the all-windows form gave up
    __shared__ double s_a[2][NW], s_b[2][NW], s_pa[T + 1], s_pr[T + 1];
    __shared__ int s_moved[2][NW];
    constexpr int kWindow = NW * 64 * T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ch = blockIdx.x;
    double e_in = state[ch];
    if (tid == 0) {                                   // (1-c)^k: a thread's slope is a product of these
        double pa = 1.0, pr = 1.0;
        for (int k = 0; k <= T; ++k) {
            s_pa[k] = pa;
            s_pr[k] = pr;
            pa = pa * (1.0 - attack_coeff);
            pr = pr * (1.0 - release_coeff);
        }
    }
    __syncthreads();

    // HBM is touched with lane-contiguous accesses (element i of thread tid is frame i*NW*64 + tid of the window);
    // the rounds want T consecutive frames per thread.  Both directions go through LDS, a chunk of T frames padded
    // to T+1 words so that neither access pattern conflicts.  (Thread-contiguous global accesses cost 8x the L1->L2
    // requests here: 2 us per window, as much as the rounds.)
    using Raw = typename std::conditional<PEAK, float, double>::type;
    constexpr int kThreads = NW * 64;
    __shared__ Raw s_x[kWindow + kWindow / T];
    __shared__ float s_y[kWindow + kWindow / T];
    Raw raw[T];
    auto fetch = [&](int64_t wbase) {                 // branch-free (clamped) so that the loads pipeline
#pragma unroll
        for (int i = 0; i < T; ++i) {
            int64_t f = wbase + i * kThreads + tid;
            f = f < n ? f : n - 1;
            if constexpr (PEAK) raw[i] = in[f * channels + ch];
            else raw[i] = det[f * channels + ch];
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const int k = i * kThreads + tid;
            s_x[k + k / T] = raw[i];
        }
    };
    double t[T];
    auto take = [&]() {
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const Raw v = s_x[tid * (T + 1) + j];
            t[j] = PEAK ? fabs((double)v) : (double)v;
        }
    };
    fetch(0);
    stage();
    __syncthreads();
    take();
    for (int64_t base = 0; base < n; base += kWindow) {
        const int64_t f0 = base + (int64_t)tid * T;
        const int live = (n - f0 >= T) ? T : (n - f0 > 0 ? (int)(n - f0) : 0);
        const bool has_next = base + kWindow < n;
        const bool full = base + kWindow <= n;
        if (has_next) fetch(base + kWindow);                               // next window, in flight

        // Two barriers per round (pieces, then the "an entry level moved" flags); LDS is double-buffered by round
        // parity so that no third one is needed.
        double entry = e_in, exit_level = e_in;
        double y[T];
        for (int round = 0; round <= NW * 64 + 1; ++round) {
            double e = entry;
            int attacks = 0;
            if (full) {                                  // every thread owns T live samples: no per-sample guard
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const bool attack = t[j] > e;
                    e = e + (attack ? attack_coeff : release_coeff) * (t[j] - e);
                    attacks += attack ? 1 : 0;
                    y[j] = e;
                }
            } else {
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const bool on = j < live;
                    const bool attack = t[j] > e;
                    const double stepped = e + (attack ? attack_coeff : release_coeff) * (t[j] - e);
                    attacks += (on && attack) ? 1 : 0;
                    e = on ? stepped : e;
                    y[j] = e;
                }
            }
            // the affine piece this thread passed through: slope from the regime counts, offset from the exit
            double a = s_pa[attacks] * s_pr[live - attacks];
            double b = __builtin_fma(-a, entry, e);
            // inclusive scan of the pieces over the wave (lanes without a source see the identity)
#define PGX_ENV_STEP(CTRL, MASK)                                            \
            {                                                               \
                const double ao = dpp_f64_keep<CTRL, MASK>(1.0, a);         \
                const double bo = dpp_f64_keep<CTRL, MASK>(0.0, b);         \
                b = __builtin_fma(a, bo, b);                                \
                a = a * ao;                                                 \
            }
            PGX_ENV_STEP(0x111, 0xf) PGX_ENV_STEP(0x112, 0xf) PGX_ENV_STEP(0x114, 0xf) PGX_ENV_STEP(0x118, 0xf)
            PGX_ENV_STEP(0x142, 0xa) PGX_ENV_STEP(0x143, 0xc)
#undef PGX_ENV_STEP
            const int buf = round & 1;
            if (lane == 63) {
                s_a[buf][wave] = a;
                s_b[buf][wave] = b;
            }
            __syncthreads();
            double cw = e_in, cn = e_in;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const double wa = s_a[buf][w], wb = s_b[buf][w];
                if (w < wave) cw = __builtin_fma(wa, cw, wb);
                cn = __builtin_fma(wa, cn, wb);
            }
            exit_level = cn;
            const double aex = dpp_f64_keep<0x138, 0xf>(1.0, a);            // wave_shr:1 -> exclusive
            const double bex = dpp_f64_keep<0x138, 0xf>(0.0, b);
            const double fresh = __builtin_fma(aex, cw, bex);
            // settled when no entry level moves by more than rounding noise (the offsets above carry ~1e-16)
            const bool moved = live > 0 && fabs(fresh - entry) > kEnvSettled * (fabs(fresh) + fabs(entry));
            entry = fresh;
            const bool wave_moved = __ballot(moved) != 0ull;
            if (lane == 0) s_moved[buf][wave] = wave_moved ? 1 : 0;
            __syncthreads();
            int any = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) any |= s_moved[buf][w];
            if (!any) break;
        }
#pragma unroll
        for (int j = 0; j < T; ++j) s_y[tid * (T + 1) + j] = (float)y[j];
        if (has_next) stage();
        __syncthreads();                               // (the next writes to s_x / s_y come after the next rounds' barriers)
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const int k = i * kThreads + tid;
            if (base + k < n) out[(base + k) * channels + ch] = s_y[k + k / T];
        }
        if (has_next) take();
        e_in = exit_level;                           // composition of all pieces (dead samples are the identity)
    }
    if (tid == 0) state[ch] = e_in;
}

// The same follower over a LONG block (look-ahead windows hand it millions of frames): all 8192-sample windows
// at once.  A window's exit level is an affine function of its entry level on the piece the trajectory runs
// through (A = product of the per-sample slopes, tiny after thousands of samples), so the entry levels of all
// windows solve a piecewise linear system of their own, again by Newton rounds -- one launch per round:
//   round 0   every window is solved (the inner rounds above) from the carried level and publishes its piece;
//   round r   a window folds the pieces of the windows before it (published in round r-1) onto the carried
//             level; if that entry is the one its samples were rendered from (1e-13) it republishes its piece and
//             is done, otherwise it renders again from the new entry and raises the round's "moved" flag.
// No window moved in a round = every window was rendered from the entry the others imply: converged; later
// launches return at once.  Window w is final after at most w+1 rounds, audio settles in 2..4 (a window forgets
// its entry by orders of magnitude).  If kEnvMwRounds are not enough the finishing kernel arms the sequential
// kernel above, which then renders the block from the carried state: the result never depends on convergence.
constexpr int kEnvMwRounds = 8;
constexpr int kEnvMwNW = 8, kEnvMwT = 16, kEnvMwWindow = kEnvMwNW * 64 * kEnvMwT;      // 8192
struct EnvMwCtl {
    int moved[kEnvMwRounds + 1];
    int fallback;
};
template <bool PEAK>
__global__ void __launch_bounds__(kEnvMwNW * 64)
k_env_newton_mw(float *out, const float *in, const double *det, int64_t n, int channels, double attack_coeff,
                double release_coeff, const double *state, int round, int nwin, double *pa_buf, double *pb_buf,
                double *guess, EnvMwCtl *ctl) {
    constexpr int NW = kEnvMwNW, T = kEnvMwT, kWindow = kEnvMwWindow, kThreads = NW * 64;
    __shared__ double s_a[2][NW], s_b[2][NW], s_pa[T + 1], s_pr[T + 1], s_entry;
    __shared__ int s_moved[2][NW];
    using Raw = typename std::conditional<PEAK, float, double>::type;
    __shared__ Raw s_x[kWindow + kWindow / T];
    __shared__ float s_y[kWindow + kWindow / T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x, ch = blockIdx.y;
    if (round > 0 && ctl->moved[round - 1] == 0) return;         // converged in an earlier round
    const int64_t base = (int64_t)w * kWindow;
    const int cur = round & 1, prev = cur ^ 1;
    double *pa_cur = pa_buf + ((int64_t)cur * channels + ch) * nwin, *pb_cur = pb_buf + ((int64_t)cur * channels + ch) * nwin;
    const double *pa_prev = pa_buf + ((int64_t)prev * channels + ch) * nwin;
    const double *pb_prev = pb_buf + ((int64_t)prev * channels + ch) * nwin;

    // request the window's frames first: their latency covers the fold below
    Raw raw[T];
#pragma unroll
    for (int i = 0; i < T; ++i) {
        int64_t f = base + i * kThreads + tid;
        f = f < n ? f : n - 1;
        if constexpr (PEAK) raw[i] = in[f * channels + ch];
        else raw[i] = det[f * channels + ch];
    }
    if (tid == 0) {
        double pa = 1.0, pr = 1.0;
        for (int k = 0; k <= T; ++k) {
            s_pa[k] = pa;
            s_pr[k] = pr;
            pa = pa * (1.0 - attack_coeff);
            pr = pr * (1.0 - release_coeff);
        }
    }
    // entry level: the carried level pushed through the pieces of windows 0..w-1 (wave 0: lanes compose runs of
    // pieces, then a scan over the lanes)
    if (wave == 0) {
        double a = 1.0, b = 0.0;
        if (round > 0) {
            const int per = (w + 63) / 64;
            const int v0 = lane * per, v1 = (v0 + per < w) ? v0 + per : w;
            for (int v = v0; v < v1; ++v) {
                const double av = pa_prev[v], bv = pb_prev[v];
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
        }
        if (lane == 63) s_entry = __builtin_fma(a, state[ch], b);
    }
    __syncthreads();
    const double e_in = s_entry;
    if (round > 0) {
        const double g = guess[(int64_t)ch * nwin + w];
        if (fabs(e_in - g) <= kEnvSettled * (fabs(e_in) + fabs(g))) {      // rendered from this entry already
            if (tid == 0) {
                pa_cur[w] = pa_prev[w];
                pb_cur[w] = pb_prev[w];
            }
            return;
        }
    }
    if (tid == 0) {
        ctl->moved[round] = 1;
        guess[(int64_t)ch * nwin + w] = e_in;
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int k = i * kThreads + tid;
        s_x[k + k / T] = raw[i];
    }
    __syncthreads();
    double t[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const Raw v = s_x[tid * (T + 1) + j];
        t[j] = PEAK ? fabs((double)v) : (double)v;
    }
    const int64_t f0 = base + (int64_t)tid * T;
    const int live = (n - f0 >= T) ? T : (n - f0 > 0 ? (int)(n - f0) : 0);
    double entry = e_in, a_tot = 1.0, b_tot = 0.0;
    double y[T];
    for (int rnd = 0; rnd <= NW * 64 + 1; ++rnd) {
        double e = entry;
        int attacks = 0;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const bool on = j < live;
            const bool attack = t[j] > e;
            const double stepped = e + (attack ? attack_coeff : release_coeff) * (t[j] - e);
            attacks += (on && attack) ? 1 : 0;
            e = on ? stepped : e;
            y[j] = e;
        }
        double a = s_pa[attacks] * s_pr[live - attacks];
        double b = __builtin_fma(-a, entry, e);
#define PGX_ENV_STEP(CTRL, MASK)                                            \
        {                                                                   \
            const double ao = dpp_f64_keep<CTRL, MASK>(1.0, a);             \
            const double bo = dpp_f64_keep<CTRL, MASK>(0.0, b);             \
            b = __builtin_fma(a, bo, b);                                    \
            a = a * ao;                                                     \
        }
        PGX_ENV_STEP(0x111, 0xf) PGX_ENV_STEP(0x112, 0xf) PGX_ENV_STEP(0x114, 0xf) PGX_ENV_STEP(0x118, 0xf)
        PGX_ENV_STEP(0x142, 0xa) PGX_ENV_STEP(0x143, 0xc)
#undef PGX_ENV_STEP
        const int buf = rnd & 1;
        if (lane == 63) {
            s_a[buf][wave] = a;
            s_b[buf][wave] = b;
        }
        __syncthreads();
        double cw = e_in, ta = 1.0, tb = 0.0;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            const double wa = s_a[buf][v], wb = s_b[buf][v];
            if (v < wave) cw = __builtin_fma(wa, cw, wb);
            tb = __builtin_fma(wa, tb, wb);                       // the window's piece: exit = ta * entry + tb
            ta = ta * wa;
        }
        a_tot = ta;
        b_tot = tb;
        const double aex = dpp_f64_keep<0x138, 0xf>(1.0, a);
        const double bex = dpp_f64_keep<0x138, 0xf>(0.0, b);
        const double fresh = __builtin_fma(aex, cw, bex);
        const bool moved = live > 0 && fabs(fresh - entry) > kEnvSettled * (fabs(fresh) + fabs(entry));
        entry = fresh;
        const bool wave_moved = __ballot(moved) != 0ull;
        if (lane == 0) s_moved[buf][wave] = wave_moved ? 1 : 0;
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) any |= s_moved[buf][v];
        if (!any) break;
    }
#pragma unroll
    for (int j = 0; j < T; ++j) s_y[tid * (T + 1) + j] = (float)y[j];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int k = i * kThreads + tid;
        if (base + k < n) out[(base + k) * channels + ch] = s_y[k + k / T];
    }
    if (tid == 0) {
        pa_cur[w] = a_tot;
        pb_cur[w] = b_tot;
    }
}

// After the last round: converged -> the new carried level is the carried level pushed through every piece;
// otherwise arm the sequential kernel.
__global__ void __launch_bounds__(64)
k_env_mw_finish(double *state, int channels, int nwin, const double *pa_buf, const double *pb_buf, EnvMwCtl *ctl,
                int rounds) {
    const int lane = threadIdx.x;
    int last = 0;                                                 // the last round in which a window moved
    for (int r = 0; r < rounds; ++r)
        if (ctl->moved[r]) last = r;
    const bool converged = last < rounds - 1;                     // a later round ran and found nothing to move
    if (!converged) {
        if (lane == 0 && blockIdx.x == 0) ctl->fallback = 1;
        return;
    }
    // pieces of the converged configuration: published by the last round that ran to its end, i.e. `last` (a round
    // in which nothing moved republishes the same pieces); round last + 1, if launched, returned at once
    const int ch = blockIdx.x;
    const int cur = (last + 1) & 1;                               // that later round republished every piece
    const double *pa = pa_buf + ((int64_t)cur * channels + ch) * nwin, *pb = pb_buf + ((int64_t)cur * channels + ch) * nwin;
    double a = 1.0, b = 0.0;
    const int per = (nwin + 63) / 64;
    const int v0 = lane * per, v1 = (v0 + per < nwin) ? v0 + per : nwin;
    for (int v = v0; v < v1; ++v) {
        b = __builtin_fma(pa[v], b, pb[v]);
        a = a * pa[v];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double ao = __shfl_up(a, d, 64), bo = __shfl_up(b, d, 64);
        if (lane >= d) {
            b = __builtin_fma(a, bo, b);
            a = a * ao;
        }
    }
    if (lane == 63) state[ch] = __builtin_fma(a, state[ch], b);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

constexpr int64_t kEnvMwMinFrames = 16 * (int64_t)kEnvMwWindow;      // from here on all windows at once

size_t pgx_envelope_scratch_bytes(int64_t n, int channels) {
    if (n <= 0 || channels <= 0) return 0;
    const size_t base = (size_t)(n + (n + kEnvBlock - 1) / kEnvBlock) * channels;
    const size_t nwin = (size_t)((n + kEnvMwWindow - 1) / kEnvMwWindow);
    return (base + 5 * nwin * channels + 8) * sizeof(double);              // + pieces (2 x 2), entries, control
}

int pgx_envelope(float *out, const float *in, int64_t n, int channels, double attack_coeff,
                 double release_coeff, int one_pole, int rms_window, int64_t rms_period, double *state,
                 double *scratch) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && in && state && scratch && channels >= 1, "pgx_envelope: bad argument");
    const bool fused_peak = !one_pole && rms_window <= 0;                   // |x| is taken inside the follower
    if (!fused_peak) {
        double *blocks = scratch + n * channels;                            // after the detector output
        if (rms_window > 0) {
            const int64_t items = (n + kEnvBlock - 1) / kEnvBlock * channels;
            hipLaunchKernelGGL(k_env_blocks, dim3((unsigned)((items + kWaves - 1) / kWaves)), dim3(kBlock), 0,
                               pgx::stream(), blocks, in, n, channels);
            PGX_LAUNCH_CHECK("k_env_blocks");
        }
        hipLaunchKernelGGL(k_env_detect, dim3(pgx::grid_for(n * channels, kBlock)), dim3(kBlock), 0, pgx::stream(),
                           scratch, in, blocks, n, channels, rms_window, rms_period);
        PGX_LAUNCH_CHECK("k_env_detect");
    }
    if (one_pole) {
        hipLaunchKernelGGL(k_env_onepole, dim3(channels), dim3(kBlock), 0, pgx::stream(), out,
                           (const double *)scratch, n, channels, attack_coeff, state);
        PGX_LAUNCH_CHECK("k_env_onepole");
    } else {
        const double *det = fused_peak ? nullptr : (const double *)scratch;
        const int *run_flag = nullptr;
        const int64_t nwin64 = (n + kEnvMwWindow - 1) / kEnvMwWindow;
        if (n >= kEnvMwMinFrames && nwin64 <= 65535 && channels <= 65535) {
            // all windows at once, one launch per Newton round over the windows' entry levels
            const int nwin = (int)nwin64;
            double *mw = scratch + (size_t)(n + (n + kEnvBlock - 1) / kEnvBlock) * channels;
            double *pa_buf = mw, *pb_buf = mw + 2 * (size_t)nwin * channels, *guess = mw + 4 * (size_t)nwin * channels;
            EnvMwCtl *ctl = reinterpret_cast<EnvMwCtl *>(mw + 5 * (size_t)nwin * channels);
            if (int rc = pgx_memset(ctl, 0, sizeof(EnvMwCtl))) return rc;
            // (PGX_ENV_MW_ROUNDS=1 makes every block give up: the test of the fallback)
            static const int rounds_env = getenv("PGX_ENV_MW_ROUNDS") ? atoi(getenv("PGX_ENV_MW_ROUNDS")) : kEnvMwRounds;
            const int rounds = rounds_env < 1 ? 1 : (rounds_env > kEnvMwRounds ? kEnvMwRounds : rounds_env);
            for (int r = 0; r < rounds; ++r) {
                if (fused_peak)
                    hipLaunchKernelGGL(k_env_newton_mw<true>, dim3(nwin, channels), dim3(kEnvMwNW * 64), 0,
                                       pgx::stream(), out, in, det, n, channels, attack_coeff, release_coeff,
                                       (const double *)state, r, nwin, pa_buf, pb_buf, guess, ctl);
                else
                    hipLaunchKernelGGL(k_env_newton_mw<false>, dim3(nwin, channels), dim3(kEnvMwNW * 64), 0,
                                       pgx::stream(), out, in, det, n, channels, attack_coeff, release_coeff,
                                       (const double *)state, r, nwin, pa_buf, pb_buf, guess, ctl);
                PGX_LAUNCH_CHECK("k_env_newton_mw");
            }
            hipLaunchKernelGGL(k_env_mw_finish, dim3(channels), dim3(64), 0, pgx::stream(), state, channels, nwin,
                               (const double *)pa_buf, (const double *)pb_buf, ctl, rounds);
            PGX_LAUNCH_CHECK("k_env_mw_finish");
            run_flag = &ctl->fallback;                // the sequential kernel below runs only if that gave up
        }
#define PGX_ENV_LAUNCH(NW, T, PEAK)                                                                               \
        hipLaunchKernelGGL((k_env_newton<NW, T, PEAK>), dim3(channels), dim3(NW * 64), 0, pgx::stream(), out, in, det, \
                           n, channels, attack_coeff, release_coeff, state, run_flag)
        if (n <= 1024) {
            if (fused_peak) PGX_ENV_LAUNCH(4, 4, true);
            else PGX_ENV_LAUNCH(4, 4, false);
        } else if (n <= 2048) {
            if (fused_peak) PGX_ENV_LAUNCH(8, 4, true);
            else PGX_ENV_LAUNCH(8, 4, false);
        } else if (n <= 4096) {
            if (fused_peak) PGX_ENV_LAUNCH(8, 8, true);
            else PGX_ENV_LAUNCH(8, 8, false);
        } else {                                     // 8192-sample windows: fewest rounds x windows (measured)
            if (fused_peak) PGX_ENV_LAUNCH(8, 16, true);
            else PGX_ENV_LAUNCH(8, 16, false);
        }
#undef PGX_ENV_LAUNCH
        PGX_LAUNCH_CHECK("k_env_newton");
    }
    return PGX_OK;
}

}  // extern "C"
