// pgx_tone.hip -- BiquadPE(SinePE) over window-sized blocks in closed form (pgx_biquad_tone).
//
// A constant-coefficient section driven by a pure tone answers, once its transient has died (settle_frames), with the
// same tone scaled by |H(e^jd)| and shifted by arg H(e^jd), d = w / sr.  The window kernels of pgx_biquad.hip already assume
// the settled condition for every wave but the first; they still run the two-pass float64 recurrence, which is what
// makes a wave own a contiguous run, carry its state and warm up.  Here a frame is
//     out[i] = float32(amp |H| sin((phase0 + arg H) + w (start + i) / sr))
// and nothing is carried from frame to frame but the rotation of a (sin, cos) pair.  What the closed form leaves out is
// the filter's answer to the float32 rounding of the input samples: at most 2^-25 sum|h| / |H| of the output's peak,
// which pgx_biquad_tone_supported bounds by 1.2e-7 (sum|h| / |H| <= 4).
//
// Layout: one workgroup per 16 KB piece (4096 frames), every thread four groups of four consecutive frames, a group one
// 16-byte store, so a wave instruction writes 1 KB contiguous and a workgroup's instruction 4 KB (the store shape of
// tools/microbench/fill_rate.hip "B").  Every thread evaluates the anchor of its first group exactly as k_sine does
// (pgx_div_by, pgx_sincos_bounded) -- an anchor shared by the piece would cost every lane the same sincos plus a turn from
// a table -- turns it by 1024 frames from group to group and makes the four frames of a group by the rotation (frame 1)
// and the three-term recurrence (frames 2, 3), or by rotations alone for tiny step angles (two_cos_d == 0, as in
// k_biquad_settled<.., SINE>).
//
// The carried state.  Workgroup 0 alone touches it: its piece covers [0, settle_frames) (settle_frames <= 4096 is one of
// the conditions of pgx_biquad_tone_supported) and it adds the zero-input response of dz = state_in - z_ss(start - 1)
// there, y_h[i] = (A^i dz).x, from the tables of pgx_biquad_tables (A^1024, A^(16 q), first rows of A^r).  z_ss(m) is the DF-II-T state of the steady solution after
// frame m with x the float32-rounded tone: s2 = b2 x[m] - a2 y[m], s1 = b2 x[m-1] - a2 y[m-1] + b1 x[m] - a1 y[m].
// state_backup receives state_in bit for bit, state leaves as z_ss(start + n - 1) (n >= 2 settle_frames: dz's part is
// below 2^-90 there).
#include "pgx_common.h"

#include <cmath>

// Switches of tools/c2_resident_probe.py (variants measured at cache-resident window sizes; the defaults are what
// ships): the groups of four frames per thread (8: two 16 KB pieces per workgroup, which moves every second anchor) and
// the cache policy of the full-group stores (16: sc1, write-through; 0: plain).
#ifndef PGX_TONE_GROUPS
#define PGX_TONE_GROUPS 4
#endif
#ifndef PGX_TONE_STORE_AUX
#define PGX_TONE_STORE_AUX 16
#endif

namespace {

constexpr int kToneBlock = 256;
constexpr int kToneGroups = PGX_TONE_GROUPS;              // groups of four frames per thread
constexpr int kToneGroupStride = kToneBlock * 4;          // 1024 frames between a thread's groups
constexpr int kTonePiece = kToneGroupStride * kToneGroups;   // 4096 frames = 16 KB per workgroup
// the layout of pgx_biquad_tables (pgx_biquad.hip k_biquad_tables): A^1024 at 24, A^(16 q) at 28 + 4 q (q < 64), the
// first rows of A^r (r < 16) at 284; pgx_biquad_tone checks the total against pgx_biquad_table_doubles()
constexpr int kTabWave = 24, kTabLane = 28, kTabRows = 28 + 4 * 64, kTabDoubles = kTabRows + 2 * 16;
constexpr double kToneNoiseRatio = 4.0;                   // sum|h| / |H| above this: the chain is declined

struct ToneArgs {
    double w, amp, phase0, sr, inv_sr;
    double phase_t;              // phase0 + arg H
    double gain;                 // amp |H|
    double hr, hi;               // amp Re H, amp Im H: y_ss = hr sin(phase) + hi cos(phase)
    double cos_d, sin_d;         // a frame's advance, w / sr
    double two_cos_d;            // 2 cos(w / sr) for the three-term recurrence, or 0: rotate (very low frequencies)
    double cos_g, sin_g;         // a group stride's advance, 1024 frames (the angle reduced on the host)
    double b1, b2, a1, a2;
    int64_t start, settle;
};

typedef unsigned int tone_v4u __attribute__((ext_vector_type(4)));

// the steady solution's DF-II-T state after absolute frame m
__device__ __forceinline__ void tone_steady_state(const ToneArgs &a, int64_t m, double &zx, double &zy) {
    double x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
#pragma nounroll
    for (int k = 0; k < 2; ++k) {                          // frame m - 1, then frame m (one copy of the sincos)
        const double t = pgx::pgx_div_by((double)(m - 1 + k), a.sr, a.inv_sr);
        double sn, cs;
        pgx::pgx_sincos_bounded(a.phase0 + a.w * t, sn, cs);
        x0 = x1;
        y0 = y1;
        x1 = (double)(float)(a.amp * sn);                  // SinePE's float32 sample
        y1 = __builtin_fma(a.hr, sn, a.hi * cs);
    }
    zy = a.b2 * x1 - a.a2 * y1;
    zx = (a.b2 * x0 - a.a2 * y0) + (a.b1 * x1 - a.a1 * y1);
}

// HEAD: workgroup 0's piece, which adds the zero-input response of dz to the frames below settle.
// SPLIT: frames [split, n) go to tail[0 ...] instead of out[split ...] (0 < split < n or split == 0: the window's last
// block in a buffer of its own).  Which frame a thread makes, from which anchor and how, does not depend on it: only the
// address of the store does.  A piece that lies wholly on one side -- all but one -- chooses its destination once,
// uniformly, and stores as the unsplit kernel does; the one piece that holds the split decides per group of four.
template <bool HEAD, bool SPLIT>
__device__ __forceinline__ void tone_piece(float *__restrict__ out, int64_t n, const double *__restrict__ tables,
                                           const ToneArgs &a, int64_t piece, bool aligned, double dzx, double dzy,
                                           float *__restrict__ tail, int64_t split, bool tail_aligned) {
    const int tid = threadIdx.x;
    const int64_t p0 = piece * kTonePiece;
    const int64_t f0 = p0 + 4 * tid;
    if (f0 >= n) return;
    // dst[0] is frame p0 of the piece's destination, which ends in front of frame lim
    float *dst = out + p0;
    int64_t lim = n;
    bool straddle = false;
    if (SPLIT) {
        if (p0 >= split) {
            dst = tail + (p0 - split);
            aligned = tail_aligned;
        } else {
            lim = split;
            straddle = split < p0 + kTonePiece;
        }
    }
    double sn, cs;
    {
        const double t = pgx::pgx_div_by((double)(a.start + f0), a.sr, a.inv_sr);
        pgx::pgx_sincos_bounded(a.phase_t + a.w * t, sn, cs);
    }
    sn *= a.gain;
    cs *= a.gain;
    // full, aligned groups are stored write-through (sc1) through a buffer resource based at the piece, as the window
    // kernel of pgx_biquad.hip stores its chunks (no dirty lines left for the launch boundary); the resource ends with the
    // piece or with the block, so a store beyond either would be dropped
    const int64_t left = lim - p0;
    const uint64_t base = (uint64_t)dst;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base), hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(((uint64_t)hi << 32) | lo), 0, (int)(left < kTonePiece ? left : kTonePiece) * 4, 0x00020000);
    // the piece that holds the split: a second resource, based at the tail, which ends with the piece or with the block
    __amdgpu_buffer_rsrc_t rsrc_tail = rsrc;
    if (SPLIT && straddle) {
        const uint64_t tbase = (uint64_t)tail;
        const uint32_t tlo = __builtin_amdgcn_readfirstlane((uint32_t)tbase),
                       thi = __builtin_amdgcn_readfirstlane((uint32_t)(tbase >> 32));
        const int64_t end = n - p0 < kTonePiece ? n : p0 + kTonePiece;
        rsrc_tail = __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)thi << 32) | tlo), 0, (int)(end - split) * 4,
                                                      0x00020000);
    }
#pragma unroll
    for (int u = 0; u < kToneGroups; ++u) {
        const int64_t f = f0 + (int64_t)u * kToneGroupStride;
        double y[4];
        y[0] = sn;
        y[1] = __builtin_fma(cs, a.sin_d, sn * a.cos_d);
        if (PGX_HOT(a.two_cos_d != 0.0)) {
            y[2] = __builtin_fma(a.two_cos_d, y[1], -y[0]);
            y[3] = __builtin_fma(a.two_cos_d, y[2], -y[1]);
        } else {
            const double c1 = __builtin_fma(-sn, a.sin_d, cs * a.cos_d);
            y[2] = __builtin_fma(c1, a.sin_d, y[1] * a.cos_d);
            const double c2 = __builtin_fma(-y[1], a.sin_d, c1 * a.cos_d);
            y[3] = __builtin_fma(c2, a.sin_d, y[2] * a.cos_d);
        }
        if (HEAD && PGX_COLD(f < a.settle)) {
            // (A^i dz).x for i = f .. f + 3: i = 1024 k + 16 q + r, and f is a multiple of 4, so the four share k and q
            const int k = (int)(f >> 10), q = (int)(f >> 4) & 63, r = (int)f & 15;
            double vx = dzx, vy = dzy;
            const double *pw = tables + kTabWave;
            for (int kk = 0; kk < k; ++kk) {
                const double nx = __builtin_fma(pw[0], vx, pw[1] * vy);
                vy = __builtin_fma(pw[2], vx, pw[3] * vy);
                vx = nx;
            }
            const double *pq = tables + kTabLane + 4 * q;
            const double qx = __builtin_fma(pq[0], vx, pq[1] * vy), qy = __builtin_fma(pq[2], vx, pq[3] * vy);
            const double *rows = tables + kTabRows + 2 * r;
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] += __builtin_fma(rows[2 * j], qx, rows[2 * j + 1] * qy);
        }
        if (f < n) {
            if (SPLIT && PGX_COLD(straddle)) {
                const tone_v4u v = {__float_as_uint((float)y[0]), __float_as_uint((float)y[1]),
                                    __float_as_uint((float)y[2]), __float_as_uint((float)y[3])};
                if (aligned && f + 4 <= split) {
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (tid * 4 + u * kToneGroupStride) * 4, 0,
                                                           PGX_TONE_STORE_AUX /* sc1 */);
                } else if (tail_aligned && f >= split && f + 4 <= n) {
                    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc_tail, (int)(f - split) * 4, 0,
                                                           PGX_TONE_STORE_AUX /* sc1 */);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t g = f + j;
                        if (g < split) out[g] = (float)y[j];
                        else if (g < n) tail[g - split] = (float)y[j];
                    }
                }
            } else if (PGX_HOT(aligned && f + 4 <= lim)) {
                const tone_v4u v = {__float_as_uint((float)y[0]), __float_as_uint((float)y[1]),
                                    __float_as_uint((float)y[2]), __float_as_uint((float)y[3])};
                __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (tid * 4 + u * kToneGroupStride) * 4, 0,
                                                       PGX_TONE_STORE_AUX /* sc1 */);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (SPLIT) {
                        if (f + j < lim) dst[f - p0 + j] = (float)y[j];
                    } else {
                        if (f + j < n) out[f + j] = (float)y[j];
                    }
                }
            }
        }
        if (u + 1 < kToneGroups) {
            const double s2 = __builtin_fma(cs, a.sin_g, sn * a.cos_g);
            cs = __builtin_fma(-sn, a.sin_g, cs * a.cos_g);
            sn = s2;
        }
    }
}

template <bool SPLIT>
__device__ __forceinline__ void tone_block(float *__restrict__ out, int64_t n, const double *__restrict__ tables,
                                           double *state, double *state_backup, const ToneArgs &a,
                                           float *__restrict__ tail, int64_t split) {
    const bool aligned = ((uintptr_t)out & 15) == 0;
    // a 16-byte store into the tail: the split on a group's edge and the tail's base on a 16-byte one
    const bool tail_aligned = SPLIT && ((uintptr_t)tail & 15) == 0 && (split & 3) == 0;
    if (blockIdx.x != 0) {
        tone_piece<false, SPLIT>(out, n, tables, a, (int64_t)blockIdx.x, aligned, 0.0, 0.0, tail, split, tail_aligned);
        return;
    }
    // workgroup 0: every thread reads the carried state before thread 0 replaces it
    const double sx = state[0], sy = state[1];
    // the steady solution's state in front of the block and at its end (one copy of the code, every thread: uniform)
    double zx = 0.0, zy = 0.0, ex = 0.0, ey = 0.0;
#pragma nounroll
    for (int k = 0; k < 2; ++k) {
        zx = ex;
        zy = ey;
        tone_steady_state(a, k == 0 ? a.start - 1 : a.start + n - 1, ex, ey);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (state_backup) {
            state_backup[0] = sx;
            state_backup[1] = sy;
        }
        state[0] = ex;
        state[1] = ey;
    }
    // one piece, not a loop over ceil(settle / 4096) of them: around a loop the compiler keeps the sincos' constants in
    // registers and 84 - 108 bytes per lane of the whole kernel went to scratch (pgx_biquad_tone_supported: settle <= 4096)
    tone_piece<true, SPLIT>(out, n, tables, a, 0, aligned, sx - zx, sy - zy, tail, split, tail_aligned);
}

// Eight waves per SIMD (<= 64 VGPRs): nothing but the stores is waited for, and the more waves the more of them in flight
__global__ void __launch_bounds__(kToneBlock, 8)
k_biquad_tone(float *__restrict__ out, int64_t n, const double *__restrict__ tables, double *state,
              double *state_backup, ToneArgs a) {
    tone_block<false>(out, n, tables, state, state_backup, a, nullptr, n);
}

// ... with frames [split, n) stored to tail[0 ...] (pgx_biquad_tone_window_split): an instantiation of its own, so that
// the unsplit kernel keeps its registers and its instructions
__global__ void __launch_bounds__(kToneBlock, 8)
k_biquad_tone_split(float *__restrict__ out, float *__restrict__ tail, int64_t split, int64_t n,
                    const double *__restrict__ tables, double *state, double *state_backup, ToneArgs a) {
    tone_block<true>(out, n, tables, state, state_backup, a, tail, split);
}

// |H(e^jd)|, arg H and sum|h| of one coefficient set, kept for the set asked about last: a stream of windows asks for
// the same chain every time
struct ToneFilter {
    double w, sr, b0, b1, b2, a1, a2;
    long double hr, hi;          // H(e^jd), d = w / sr
    double gain;                 // |H|
    int64_t l1_frames;           // what l1 was summed over; 0: not yet
    double l1;
};

static long double tone_response(double w, double sr, double b0, double b1, double b2, double a1, double a2,
                                 long double &hr, long double &hi) {
    const long double d = (long double)w / (long double)sr;
    const long double c1 = cosl(d), s1 = -sinl(d), c2 = cosl(2.0L * d), s2 = -sinl(2.0L * d);   // e^-jd, e^-2jd
    const long double nr = b0 + b1 * c1 + b2 * c2, ni = b1 * s1 + b2 * s2;
    const long double dr = 1.0L + a1 * c1 + a2 * c2, di = a1 * s1 + a2 * s2;
    const long double den = dr * dr + di * di;
    hr = (nr * dr + ni * di) / den;
    hi = (ni * dr - nr * di) / den;
    return hypotl(hr, hi);
}

static double tone_l1(int64_t frames, double b0, double b1, double b2, double a1, double a2) {
    double s0 = 0.0, s1 = 0.0, l1 = 0.0, x = 1.0;        // DF-II-T impulse response
    for (int64_t i = 0; i < frames; ++i) {
        const double y = s0 + b0 * x;
        s0 = s1 + b1 * x - a1 * y;
        s1 = b2 * x - a2 * y;
        l1 += fabs(y);
        x = 0.0;
    }
    return l1;
}

static ToneFilter &tone_filter(double w, double sr, double b0, double b1, double b2, double a1, double a2) {
    static ToneFilter f{};
    static bool have = false;
    if (!have || f.w != w || f.sr != sr || f.b0 != b0 || f.b1 != b1 || f.b2 != b2 || f.a1 != a1 || f.a2 != a2) {
        f = ToneFilter{w, sr, b0, b1, b2, a1, a2, 0.0L, 0.0L, 0.0, 0, 0.0};
        f.gain = (double)tone_response(w, sr, b0, b1, b2, a1, a2, f.hr, f.hi);
        have = true;
    }
    return f;
}

static bool tone_supported(int64_t n, int64_t settle, double w, double sr, double b0, double b1, double b2, double a1,
                           double a2) {
    // settle <= one piece: the carried state's response ends inside the piece of workgroup 0, which alone handles the state
    if (settle <= 0 || settle > kTonePiece || n < 2 * settle || !(sr > 0.0)) return false;
    if (!(fabs(w) * ((double)n / sr) < pgx::kSinFastRange)) return false;
    ToneFilter &f = tone_filter(w, sr, b0, b1, b2, a1, a2);
    if (f.l1_frames != settle) {
        f.l1 = tone_l1(settle, b0, b1, b2, a1, a2);
        f.l1_frames = settle;
    }
    return std::isfinite(f.gain) && std::isfinite(f.l1) && f.l1 <= kToneNoiseRatio * f.gain;
}

// Frames per look-ahead window of a stream of these windows.  The kernel is bound by its stores.  A stream has one big
// buffer live: a window's last block is stored to a buffer of its own (k_biquad_tone_split), so a caller that keeps the
// last snippet it pulled keeps those 4 MB and the window's buffer returns to the pool when the window is used up; the
// next window gets the same address and is stored over lines that are still in the 256 MiB memory-side cache.  Into one
// rewritten buffer the kernel costs 0.552 - 0.576 us per M frames from 36 M to 67 M frames (into two in turn 0.587 at
// 36 M, 0.60 at 40 M, 0.67 from 48 M on: tools/c2_resident_probe.py single), and the larger the window the less of the
// host's cost of an opening falls on a step.  The sweep of profiles/c2_single_window.md, bench.py at 1 M-frame steps,
// Msamples/s, three runs per size alternated with the parent's 1 536 000 - 1 667 000 (36 M-frame windows, two buffers):
// 36 M 1 503 000 - 1 526 000 (the host bounds it: an opening costs more than the parent's), 44 M 1 676 000 - 1 721 000,
// 48 M 1 739 000 - 1 781 000, 52 M 1 772 000 - 1 795 000, 56 M 1 790 000 - 1 813 000, 60 M 1 788 000 - 1 803 000,
// 64 M 1 804 000 - 1 821 000, 67 M 1 774 000 - 1 811 000.  64 M has the highest minimum; the probe's 64 M-frame launch is
// also its cheapest per frame (35.3 us, 0.552 us per M frames).  With PGX_TONE_SPLIT_TAIL=0 two buffers alternate again,
// and 36 M is the size to ask for (PGX_TONE_WINDOW_FRAMES).
constexpr int64_t kToneWindowFrames = 64000000;

static int64_t tone_window_frames_env() {
    const char *e = getenv("PGX_TONE_WINDOW_FRAMES");      // 0: no preference
    if (e && *e) {
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end != e && v >= 0) return (int64_t)v;
    }
    return kToneWindowFrames;
}

// One chain's launch constants: everything of a window launch that does not depend on (out, start, n, state).
struct TonePlan {
    ToneArgs a;                  // start is filled in per launch
    const double *tables;
    double phase_abs, w_abs;     // |phase0|, |w|: the per-launch range checks
};

// false: the chain is one pgx_biquad_tone_supported declines whatever the block length
static bool tone_make_plan(TonePlan &p, double sample_rate, double w, double amp, double phase0, double b0, double b1,
                           double b2, double a1, double a2, const double *tables, int64_t settle_frames) {
    if (!tables || !(sample_rate > 0.0)) return false;
    if (!tone_supported(2 * settle_frames, settle_frames, w, sample_rate, b0, b1, b2, a1, a2)) return false;
    const ToneFilter &f = tone_filter(w, sample_rate, b0, b1, b2, a1, a2);
    // the tone's constants, made once per (w, sample rate) in long double
    static ToneArgs cached;
    static bool have = false;
    if (!have || cached.w != w || cached.sr != sample_rate) {
        ToneArgs c{};
        c.w = w;
        c.sr = sample_rate;
        c.inv_sr = 1.0 / sample_rate;
        const long double d = (long double)w / (long double)sample_rate;
        c.cos_d = (double)cosl(d);
        c.sin_d = (double)sinl(d);
        c.two_cos_d = (fabsl(sinl(d)) >= 1e-3L) ? (double)(2.0L * cosl(d)) : 0.0;
        const long double turn = 6.283185307179586476925286766559L;
        long double g = d * (long double)kToneGroupStride;
        g -= turn * floorl(g / turn);
        c.cos_g = (double)cosl(g);
        c.sin_g = (double)sinl(g);
        cached = c;
        have = true;
    }
    ToneArgs a = cached;
    a.amp = amp;
    a.phase0 = phase0;
    a.phase_t = phase0 + (double)atan2l(f.hi, f.hr);
    a.gain = amp * f.gain;
    a.hr = amp * (double)f.hr;
    a.hi = amp * (double)f.hi;
    a.b1 = b1;
    a.b2 = b2;
    a.a1 = a1;
    a.a2 = a2;
    a.start = 0;
    a.settle = settle_frames;
    p.a = a;
    p.tables = tables;
    p.phase_abs = fabs(phase0);
    p.w_abs = fabs(w);
    return true;
}

// tail_frames > 0: frames [n - tail_frames, n) go to out_tail[0 ...]
static int tone_launch(const TonePlan &p, float *out, int64_t start, int64_t n, double *state, double *state_backup,
                       const char *who, float *out_tail = nullptr, int64_t tail_frames = 0) {
    PGX_CHECK_ARG(tail_frames >= 0 && tail_frames <= n, std::string(who) + ": tail_frames outside [0, n]");
    PGX_CHECK_ARG(tail_frames == 0 || out_tail, std::string(who) + ": tail frames and no out_tail");
    PGX_CHECK_ARG((out || tail_frames == n) && state, std::string(who) + ": bad argument");
    PGX_CHECK_ARG(pgx_biquad_table_doubles() == (size_t)kTabDoubles, std::string(who) + ": table layout changed");
    // what of pgx_biquad_tone_supported depends on the block: n >= 2 settle_frames and the phase advance over it
    PGX_CHECK_ARG(n >= 2 * p.a.settle && p.w_abs * ((double)n / p.a.sr) < pgx::kSinFastRange,
                  std::string(who) + ": chain or block not supported (pgx_biquad_tone_supported)");
    // the largest phase of the render (and of the frame before it) has to stay in the bounded sine's range
    const double far = p.phase_abs + p.w_abs * ((double)(llabs(start) + n + 1) / p.a.sr);
    PGX_CHECK_ARG(far + 4.0 < pgx::kSinFastRange, std::string(who) + ": phase beyond the fast sine range");
    ToneArgs a = p.a;
    a.start = start;
    const int64_t pieces = pgx::ceil_div(n, (int64_t)kTonePiece);
    PGX_CHECK_ARG(pieces <= 0x7fffffff, std::string(who) + ": block too long");
    if (tail_frames > 0) {
        hipLaunchKernelGGL(k_biquad_tone_split, dim3((unsigned)pieces), dim3(kToneBlock), 0, pgx::stream(), out, out_tail,
                           n - tail_frames, n, p.tables, state, state_backup, a);
        PGX_LAUNCH_CHECK("k_biquad_tone_split");
        return PGX_OK;
    }
    hipLaunchKernelGGL(k_biquad_tone, dim3((unsigned)pieces), dim3(kToneBlock), 0, pgx::stream(), out, n, p.tables, state,
                       state_backup, a);
    PGX_LAUNCH_CHECK("k_biquad_tone");
    return PGX_OK;
}

}  // namespace

extern "C" {

int pgx_biquad_tone_supported(int64_t n, int64_t settle_frames, double w, double sample_rate, double b0, double b1,
                              double b2, double a1, double a2) {
    return tone_supported(n, settle_frames, w, sample_rate, b0, b1, b2, a1, a2) ? 1 : 0;
}

double pgx_biquad_tone_gain(double w, double sample_rate, double b0, double b1, double b2, double a1, double a2) {
    long double hr, hi;
    return (double)tone_response(w, sample_rate, b0, b1, b2, a1, a2, hr, hi);
}

double pgx_biquad_tone_l1(int64_t settle_frames, double b0, double b1, double b2, double a1, double a2) {
    return tone_l1(settle_frames, b0, b1, b2, a1, a2);
}

int64_t pgx_biquad_tone_window_frames(void) {
    static const int64_t frames = tone_window_frames_env();
    return frames;
}

void *pgx_biquad_tone_plan(double sample_rate, double w, double amp, double phase0, double b0, double b1, double b2,
                           double a1, double a2, const double *tables, int64_t settle_frames) {
    TonePlan *p = new TonePlan;
    if (!tone_make_plan(*p, sample_rate, w, amp, phase0, b0, b1, b2, a1, a2, tables, settle_frames)) {
        delete p;
        return nullptr;
    }
    return p;
}

int pgx_biquad_tone_plan_free(void *plan) {
    delete static_cast<TonePlan *>(plan);
    return PGX_OK;
}

int pgx_biquad_tone_window(const void *plan, float *out, int64_t start, int64_t n, double *state, double *state_backup) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(plan, "pgx_biquad_tone_window: no plan");
    return tone_launch(*static_cast<const TonePlan *>(plan), out, start, n, state, state_backup, "pgx_biquad_tone_window");
}

int pgx_biquad_tone_window_split(const void *plan, float *out, float *out_tail, int64_t tail_frames, int64_t start,
                                 int64_t n, double *state, double *state_backup) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(tail_frames >= 0 && (n <= 0 || tail_frames <= n), "pgx_biquad_tone_window_split: tail_frames outside [0, n]");
    PGX_CHECK_ARG(tail_frames == 0 || out_tail, "pgx_biquad_tone_window_split: tail frames and no out_tail");
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(plan, "pgx_biquad_tone_window_split: no plan");
    return tone_launch(*static_cast<const TonePlan *>(plan), out, start, n, state, state_backup,
                       "pgx_biquad_tone_window_split", out_tail, tail_frames);
}

int pgx_biquad_tone_split_tail(void) {
    static const int wanted = []() {
        const char *e = getenv("PGX_TONE_SPLIT_TAIL");
        return (e && e[0] == '0' && e[1] == 0) ? 0 : 1;
    }();
    return wanted;
}

int pgx_biquad_tone(float *out, int64_t start, int64_t n, double sample_rate, double w, double amp, double phase0,
                    double b0, double b1, double b2, double a1, double a2, const double *tables,
                    int64_t settle_frames, double *state, double *state_backup) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && tables && state && sample_rate > 0, "pgx_biquad_tone: bad argument");
    TonePlan p;
    PGX_CHECK_ARG(tone_make_plan(p, sample_rate, w, amp, phase0, b0, b1, b2, a1, a2, tables, settle_frames),
                  "pgx_biquad_tone: chain or block not supported (pgx_biquad_tone_supported)");
    return tone_launch(p, out, start, n, state, state_backup, "pgx_biquad_tone");
}

}  // extern "C"
