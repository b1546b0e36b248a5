// pgx_sources.hip -- the synth sources KarplusStrongPE (karplus_strong_pe.py:61-220) and AnalogOscPE
// (analog_osc_pe.py:34-267).
//
// KarplusStrongPE: one period of noise in a circular line, per frame
//     ov = f32(f32(rho * f32(buf[r] + buf[r+1])) * 0.5)
//     ao = f32(f32(f32(c * ov) + ap_in) - f32(c * ap_out)),  buf[r] = ao,  r = (r + 1) % N
// in float32, in the reference's operation order: the library is built with -ffp-contract=off, so every line is one
// rounding and the output is bit-exact.  Lane per string.  Within any N - 1 consecutive frames the line positions a
// frame reads were written one period earlier, so a lane gathers a chunk of up to kKsChunk + 1 line values at once
// (the loads are off the recurrence) and then runs the chunk's serial chain from registers: the only dependent work
// per frame is the multiply and the subtract on ap_out.  Lines of a workgroup's strings that fit in LDS are staged
// there for the render; longer ones (1 Hz at 192 kHz is N = 192 000) are read and written in global memory / L2.
//
// AnalogOscPE: float64 throughout, one float32 rounding on output.  The pure rectangle is a function of the frame
// index (one element-wise launch).  The sawtooth integrates its derivative and the stateful form integrates the phase
// increment: those go through a three-pass float64 scan (per-workgroup sums, one workgroup scanning the sums with the
// carried state, per-workgroup re-evaluation), twice for the stateful sawtooth.  The carried phase / saw value live in
// a device state blob; nothing here synchronises.  A bank of oscillators (pgx_analog_osc_bank, voice_bank.py) is the same
// kernels with the voice as a grid dimension -- blockIdx.y of a pass, a scan workgroup per voice -- on per-voice parameters,
// streams, state and workspace slice: the launches of one PE, each voice's samples bit for bit.

#include "pgx_common.h"

namespace {

// ================================================================================================
// KarplusStrongPE
// ================================================================================================
constexpr int kKsLanes = 64;            // strings per workgroup (one wave)
constexpr int kKsChunk = 64;            // frames per gather
constexpr int64_t kKsLdsBytes = 64 * 1024;

template <typename Line>
__device__ __forceinline__ void ks_run(Line *buf, const pgx_ks_params &p, pgx_ks_state &st, float *o, int64_t start,
                                       int64_t n, int channels) {
    const int N = p.n;
    const float c = p.c;
    int r = st.r;
    float ap_in = st.ap_in, ap_out = st.ap_out;
    const int lmax = (N - 1 < kKsChunk) ? N - 1 : kKsChunk;
    for (int64_t i = 0; i < n;) {
        const int L = (n - i < lmax) ? (int)(n - i) : lmax;
        const int64_t g0 = start + i;
        // the common chunk: whole, no wrap of the line inside it, mono, one rho -- straight-line code with constant
        // offsets (a lone string is issue-bound: every instruction per frame counts)
        if (L == kKsChunk && r + kKsChunk < N && channels == 1 &&
            (!p.two_phase || g0 >= p.switch_at || g0 + kKsChunk <= p.switch_at)) {
            const float rho = (p.two_phase && g0 >= p.switch_at) ? p.rho_damping : p.rho;
            Line *line = buf + r;
            float b[kKsChunk + 1];
#pragma unroll
            for (int j = 0; j <= kKsChunk; ++j) b[j] = line[j];
#pragma unroll
            for (int j = 0; j < kKsChunk; ++j) {
                const float s = b[j] + b[j + 1];
                const float ov = (rho * s) * 0.5f;
                const float ff = (c * ov) + ap_in;
                const float ao = ff - (c * ap_out);
                ap_in = ov;
                ap_out = ao;
                b[j] = ao;
            }
            float *row = o + i;
#pragma unroll
            for (int j = 0; j < kKsChunk; ++j) {
                line[j] = b[j];
                row[j] = b[j];
            }
            r += kKsChunk;
            i += kKsChunk;
            continue;
        }
        float b[kKsChunk + 1];
        // positions r .. r + kKsChunk (mod N): always inside the line; only the first L + 1 are used, and none of
        // those is written before it is read (L <= N - 1)
        int q = r;
#pragma unroll
        for (int j = 0; j <= kKsChunk; ++j) {
            b[j] = buf[q];
            q = (q + 1 == N) ? 0 : q + 1;
        }
#pragma unroll
        for (int j = 0; j < kKsChunk; ++j) {
            if (j < L) {
                const float rho = (p.two_phase && g0 + j >= p.switch_at) ? p.rho_damping : p.rho;
                const float s = b[j] + b[j + 1];
                const float ov = (rho * s) * 0.5f;
                const float ff = (c * ov) + ap_in;
                const float ao = ff - (c * ap_out);
                ap_in = ov;
                ap_out = ao;
                b[j] = ao;
            }
        }
        q = r;
#pragma unroll
        for (int j = 0; j < kKsChunk; ++j) {
            if (j < L) {
                buf[q] = b[j];
                float *row = o + (i + j) * channels;
                for (int ch = 0; ch < channels; ++ch) row[ch] = b[j];
                q = (q + 1 == N) ? 0 : q + 1;
            }
        }
        r += L;
        if (r >= N) r -= N;
        i += L;
    }
    st.r = r;
    st.ap_in = ap_in;
    st.ap_out = ap_out;
}

// kLds: the workgroup's lines are copied to LDS (lane l's at l * max_line) and back after the render
template <bool kLds>
__global__ void __launch_bounds__(kKsLanes)
k_karplus_strong(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                 const pgx_ks_params *params, float *lines, pgx_ks_state *state, int max_line) {
    extern __shared__ float ks_lds[];
    const int first = blockIdx.x * kKsLanes;
    const int here = (batch - first < kKsLanes) ? batch - first : kKsLanes;
    const int s = first + (int)threadIdx.x;
    if (kLds) {
        for (int k = 0; k < here; ++k) {
            const pgx_ks_params q = params[first + k];
            for (int x = threadIdx.x; x < q.n; x += kKsLanes) ks_lds[(int64_t)k * max_line + x] = lines[q.line_offset + x];
        }
        __syncthreads();
    }
    if (s < batch) {
        const pgx_ks_params p = params[s];
        pgx_ks_state st = state[s];
        float *o = out + (int64_t)s * out_stride;
        if (kLds) ks_run(ks_lds + (int64_t)threadIdx.x * max_line, p, st, o, start, n, channels);
        else ks_run(lines + p.line_offset, p, st, o, start, n, channels);
        state[s] = st;
    }
    if (kLds) {
        __syncthreads();
        for (int k = 0; k < here; ++k) {
            const pgx_ks_params q = params[first + k];
            for (int x = threadIdx.x; x < q.n; x += kKsLanes) lines[q.line_offset + x] = ks_lds[(int64_t)k * max_line + x];
        }
    }
}

// The plucks of a score: string k of the launch is notes[k], with its own parameter block, line, state, first frame,
// frame count and destination.  `group` strings per workgroup, a lane each (lanes group .. 63 only help to stage).  A
// workgroup stages its lines in LDS at a stride of ITS longest line when they fit in the lds_floats the launch was
// given, and otherwise works in global memory: one 1 Hz string does not take the other workgroups off the LDS path.
// A launch of at most kKsInline strings carries notes[] in its kernel arguments (k_karplus_score_inline): nothing is
// uploaded for it, which is what a streamed block of a score with a handful of sounding plucks needs.
constexpr int kKsInline = PGX_SCORE_INLINE;
struct KsInline {
    pgx_ks_note n[kKsInline];
};

__device__ __forceinline__ void ks_score_body(float *ks_lds, float *out, int channels, const pgx_ks_note *notes,
                                              int count, int group, int max_line, int lds_floats) {
    const int first = blockIdx.x * group;
    const int here = (count - first < group) ? count - first : group;
    int stride = 2;
    bool ok = true;
    for (int k = 0; k < here; ++k) {
        const int n = notes[first + k].params->n;
        stride = n > stride ? n : stride;
        ok = ok && n >= 2;                                 // (ks_run's chunks are N - 1 frames: N < 2 would never end)
    }
    ok = ok && stride <= max_line;                         // a line longer than the caller said: nothing is touched
    const bool use_lds = ok && (int64_t)here * stride <= lds_floats;
    if (use_lds) {
        for (int k = 0; k < here; ++k) {
            const pgx_ks_note q = notes[first + k];
            const float *src = q.line + q.params->line_offset;
            const int n = q.params->n;
            for (int x = threadIdx.x; x < n; x += kKsLanes) ks_lds[k * stride + x] = src[x];
        }
        __syncthreads();
    }
    if (ok && (int)threadIdx.x < here) {
        const pgx_ks_note q = notes[first + (int)threadIdx.x];
        const pgx_ks_params p = *q.params;
        pgx_ks_state st = *q.state;
        float *o = out + q.dst;
        if (use_lds) ks_run(ks_lds + (int)threadIdx.x * stride, p, st, o, q.start, q.frames, channels);
        else ks_run(q.line + p.line_offset, p, st, o, q.start, q.frames, channels);
        *q.state = st;
    }
    if (use_lds) {
        __syncthreads();
        for (int k = 0; k < here; ++k) {
            const pgx_ks_note q = notes[first + k];
            float *dst = q.line + q.params->line_offset;
            const int n = q.params->n;
            for (int x = threadIdx.x; x < n; x += kKsLanes) dst[x] = ks_lds[k * stride + x];
        }
    }
}

__global__ void __launch_bounds__(kKsLanes)
k_karplus_score(float *out, int channels, const pgx_ks_note *notes, int count, int group, int max_line,
                int lds_floats) {
    extern __shared__ float ks_lds[];
    ks_score_body(ks_lds, out, channels, notes, count, group, max_line, lds_floats);
}

__global__ void __launch_bounds__(kKsLanes)
k_karplus_score_inline(float *out, int channels, KsInline notes, int count, int group, int max_line, int lds_floats) {
    extern __shared__ float ks_lds[];
    ks_score_body(ks_lds, out, channels, notes.n, count, group, max_line, lds_floats);
}

// ================================================================================================
// AnalogOscPE
// ================================================================================================
constexpr int kOscBlock = 256;
constexpr int kOscWaves = kOscBlock / 64;
constexpr int kOscT = 8;
constexpr int kOscTile = kOscBlock * kOscT;

// _blep (analog_osc_pe.py:118-141): u**4 as (u*u)*(u*u), the rounding numpy's vectorised power gives here
__device__ __forceinline__ double osc_blep(double t, double dt) {
    double y = 0.0;
    if (t < 2.0 * dt) {
        const double x = t / dt;
        const double u = 2.0 - x;
        y = (u * u) * (u * u);
        if (t < dt) {
            const double v = 1.0 - x;
            y = y - 4.0 * ((v * v) * (v * v));
        }
    }
    return y / 12.0;
}

// _blep_residual (:143-152)
__device__ __forceinline__ double osc_residual(double t, double dt) {
    const double tm = pgx::pgx_mod1(t);
    return osc_blep(tm, dt) - osc_blep(1.0 - tm, dt);
}

struct OscFrame {
    double dt, dtb, duty;     // signed increment, |dt| clipped for the BLEP window, clipped duty
};

// :212-221
__device__ __forceinline__ OscFrame osc_frame(double freq, double duty, double sr) {
    OscFrame f;
    f.dt = freq / sr;
    f.dtb = fmin(fmax(fabs(f.dt), 1e-12), 0.5);
    const double edge = fmax(1e-5, 2.0 * f.dtb);
    f.duty = fmin(fmax(duty, edge), 1.0 - edge);
    return f;
}

// :229-238
__device__ __forceinline__ double osc_rect(double phase, const OscFrame &f) {
    const double base = (phase < f.duty) ? 1.0 : -1.0;
    const double r0 = osc_residual(phase, f.dtb);
    const double r1 = osc_residual(phase - f.duty, f.dtb);
    return (base + r0) - r1;
}

// :240-260: the corrected derivative times the signed increment
__device__ __forceinline__ double osc_saw_dy(double phase, const OscFrame &f) {
    const double a = 1.0 - f.duty;
    const double u1 = 2.0 / a;
    const double u2 = -2.0 / (1.0 - a);
    const double u = (phase < a) ? u1 : u2;
    const double delta = u2 - u1;
    const double uc = (u + (-0.5 * delta) * osc_residual(phase, f.dtb)) + (0.5 * delta) * osc_residual(phase - a, f.dtb);
    return uc * f.dt;
}

// _piecewise_linear_value (:195-201)
__device__ __forceinline__ double osc_piecewise(double phase0, double a) {
    if (phase0 < a) return -1.0 + 2.0 * (phase0 / a);
    return 1.0 - 2.0 * ((phase0 - a) / (1.0 - a));
}

// Block-wide exclusive prefix sum of one double per thread plus the block total (two barriers).
__device__ __forceinline__ double osc_block_excl(double v, double *lds, double &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = o + inc;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    double woff = 0.0, tot = 0.0;
#pragma unroll
    for (int w = 0; w < kOscWaves; ++w) {
        const double t = lds[w];
        if (w < wave) woff = woff + t;
        tot = tot + t;
    }
    __syncthreads();
    total = tot;
    double ex = __shfl_up(inc, 1, 64);
    if (lane == 0) ex = 0.0;
    return woff + ex;
}

__device__ __forceinline__ void osc_store(float *out, int64_t f, int channels, double y) {
    const float v = (float)y;
    float *row = out + f * channels;
    for (int ch = 0; ch < channels; ++ch) row[ch] = v;
}

struct OscScalars {
    double freq, duty, sample_rate;   // scalar parameters (streams override freq / duty)
    int waveform;                     // 0 rectangle, 1 sawtooth
};

struct OscArgs {
    OscScalars p;
    int64_t start, n;
    int channels;
    const float *freq, *duty;     // stateful: float32 streams or NULL (scalar)
    // a bank: the voice is blockIdx.y of a pass (blockIdx.x of a scan); voice v writes at out + v * out_stride, reads
    // params[v] (NULL: p.freq / p.duty, the single PE) and its streams at + v * stride
    const pgx_osc_params *params;
    int64_t out_stride, freq_stride, duty_stride;
};

// What voice v sees: its scalars, its streams.
__device__ __forceinline__ OscArgs osc_voice(OscArgs a, int v) {
    if (a.params) {
        a.p.freq = a.params[v].freq;
        a.p.duty = a.params[v].duty;
    }
    if (a.freq) a.freq += (int64_t)v * a.freq_stride;
    if (a.duty) a.duty += (int64_t)v * a.duty_stride;
    return a;
}

__device__ __forceinline__ OscFrame osc_frame_at(const OscArgs &a, int64_t f) {
    const double fr = a.freq ? (double)a.freq[f] : a.p.freq;
    const double du = a.duty ? (double)a.duty[f] : a.p.duty;
    return osc_frame(fr, du, a.p.sample_rate);
}

// workspace layout (doubles): [0, nb) sums, [nb, 2 nb) offsets, [2 nb, 2 nb + 4) seeds {phase0, y0}; a voice owns two
// of these (dt scan, dy scan), voice after voice
struct OscWs {
    double *sum, *off, *seed;
};
__host__ __device__ __forceinline__ int64_t osc_ws_doubles(int64_t nb) { return 2 * nb + 4; }
__device__ __forceinline__ OscWs osc_ws(double *ws, int64_t nb, int v) {
    ws += (int64_t)v * (2 * osc_ws_doubles(nb));
    return {ws, ws + nb, ws + 2 * nb};
}

// pure rectangle: phase = mod(idx * dt[0], 1) (:185-187)
__global__ void __launch_bounds__(kOscBlock) k_osc_pure_rect(float *out, OscArgs bank) {
    const OscArgs a = osc_voice(bank, blockIdx.y);
    out += (int64_t)blockIdx.y * a.out_stride;
    const OscFrame fr = osc_frame(a.p.freq, a.p.duty, a.p.sample_rate);
    for (int64_t f = (int64_t)blockIdx.x * kOscBlock + threadIdx.x; f < a.n; f += (int64_t)gridDim.x * kOscBlock) {
        const double phase = pgx::pgx_mod1((double)(a.start + f) * fr.dt);
        osc_store(out, f, a.channels, osc_rect(phase, fr));
    }
}

// The phase of frame f.  Pure: from the index.  Stateful: phase0 + exclusive prefix of dt (needs the dt scan).
// kPass 0: stateful, sum dt per workgroup.
// kPass 1: phases known (pure, or stateful after the dt scan): rectangle -> emit; sawtooth -> sum dy per workgroup.
// kPass 2: sawtooth: y0 + exclusive prefix of dy -> emit.
template <bool kPure, int kPass>
__global__ void __launch_bounds__(kOscBlock) k_osc_pass(float *out, OscArgs bank, double *ws_raw, double *ws2_raw,
                                                        int64_t nb) {
    __shared__ double lds[kOscWaves];
    const OscArgs a = osc_voice(bank, blockIdx.y);
    out += (int64_t)blockIdx.y * a.out_stride;
    const OscWs ws = osc_ws(ws_raw, nb, blockIdx.y);       // dt scan (stateful) / dy scan (pure)
    const OscWs wy = osc_ws(ws2_raw, nb, blockIdx.y);      // dy scan (stateful)
    const int64_t f0 = (int64_t)blockIdx.x * kOscTile + (int64_t)threadIdx.x * kOscT;
    OscFrame fr[kOscT];
    double phase[kOscT];
#pragma unroll
    for (int j = 0; j < kOscT; ++j) {
        const int64_t f = (f0 + j < a.n) ? f0 + j : a.n - 1;
        fr[j] = kPure ? osc_frame(a.p.freq, a.p.duty, a.p.sample_rate) : osc_frame_at(a, f);
        if (f0 + j >= a.n) fr[j].dt = 0.0;
    }
    double total;
    if (!kPure) {
        double run = 0.0, loc[kOscT];
#pragma unroll
        for (int j = 0; j < kOscT; ++j) {
            loc[j] = run;
            run = run + fr[j].dt;
        }
        const double off = osc_block_excl(run, lds, total);
        if (kPass == 0) {
            if (threadIdx.x == 0) ws.sum[blockIdx.x] = total;
            return;
        }
        const double base = ws.off[blockIdx.x] + off;
#pragma unroll
        for (int j = 0; j < kOscT; ++j) phase[j] = pgx::pgx_mod1(ws.seed[0] + (base + loc[j]));
    } else {
#pragma unroll
        for (int j = 0; j < kOscT; ++j) phase[j] = pgx::pgx_mod1((double)(a.start + f0 + j) * fr[j].dt);
    }
    if (a.p.waveform == 0) {        // rectangle (pass 1 only)
#pragma unroll
        for (int j = 0; j < kOscT; ++j)
            if (f0 + j < a.n) osc_store(out, f0 + j, a.channels, osc_rect(phase[j], fr[j]));
        return;
    }
    const OscWs &wd = kPure ? ws : wy;
    double run = 0.0, loc[kOscT];
#pragma unroll
    for (int j = 0; j < kOscT; ++j) {
        loc[j] = run;
        if (f0 + j < a.n) run = run + osc_saw_dy(phase[j], fr[j]);
    }
    const double off = osc_block_excl(run, lds, total);
    if (kPass == 1) {
        if (threadIdx.x == 0) wd.sum[blockIdx.x] = total;
        return;
    }
    const double base = wd.off[blockIdx.x] + off;
    const double y0 = wd.seed[1];
#pragma unroll
    for (int j = 0; j < kOscT; ++j)
        if (f0 + j < a.n) osc_store(out, f0 + j, a.channels, y0 + (base + loc[j]));
}

// One workgroup: exclusive scan of the nb workgroup sums.  kWhat 0: the dt scan of the stateful form (seeds the phase
// from the carried state, or 0 on a restart; carries mod(phase0 + sum dt, 1)).  kWhat 1: the dy scan of the stateful
// sawtooth (seeds y0 from the carried saw value, or -1 on a restart; carries y0 + sum dy).  kWhat 2: the dy scan of the
// pure sawtooth (y0 from phase[0], :253-256).  A workgroup per voice, on the voice's workspace and state.
template <int kWhat>
__global__ void __launch_bounds__(kOscBlock) k_osc_scan(double *ws_raw, int64_t nb, double *state, int restart,
                                                        OscArgs bank) {
    __shared__ double lds[kOscWaves];
    const OscWs ws = osc_ws(ws_raw, nb, blockIdx.x);
    if (kWhat != 2) state += 2 * (int64_t)blockIdx.x;
    double carry = 0.0;
    for (int64_t b0 = 0; b0 < nb; b0 += kOscTile) {
        const int64_t i0 = b0 + (int64_t)threadIdx.x * kOscT;
        double run = 0.0, loc[kOscT];
#pragma unroll
        for (int j = 0; j < kOscT; ++j) {
            loc[j] = run;
            if (i0 + j < nb) run = run + ws.sum[i0 + j];
        }
        double total;
        const double off = osc_block_excl(run, lds, total);
#pragma unroll
        for (int j = 0; j < kOscT; ++j)
            if (i0 + j < nb) ws.off[i0 + j] = carry + (off + loc[j]);
        carry = carry + total;
    }
    if (threadIdx.x == 0) {
        if (kWhat == 0) {
            const double ph0 = restart ? 0.0 : state[0];
            ws.seed[0] = ph0;
            state[0] = pgx::pgx_mod1(ph0 + carry);
            if (restart) state[1] = -1.0;
        } else if (kWhat == 1) {
            const double y0 = state[1];
            ws.seed[1] = y0;
            state[1] = y0 + carry;
        } else {
            const OscArgs a = osc_voice(bank, blockIdx.x);
            const OscFrame fr = osc_frame(a.p.freq, a.p.duty, a.p.sample_rate);
            const double ph0 = pgx::pgx_mod1((double)a.start * fr.dt);
            ws.seed[1] = osc_piecewise(ph0, 1.0 - fr.duty);
        }
    }
}

}  // namespace

extern "C" {

int pgx_karplus_strong(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                       const pgx_ks_params *params, float *lines, pgx_ks_state *state, int max_line) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && lines && state && channels >= 1 && max_line >= 2 && start >= 0 &&
                      out_stride >= n * channels,
                  "pgx_karplus_strong: bad argument");
    const int grid = (int)pgx::ceil_div(batch, kKsLanes);
    const int lanes = batch < kKsLanes ? batch : kKsLanes;
    const int64_t lds = (int64_t)lanes * max_line * (int64_t)sizeof(float);
    if (lds <= kKsLdsBytes) {
        hipLaunchKernelGGL(k_karplus_strong<true>, dim3(grid), dim3(kKsLanes), (size_t)lds, pgx::stream(), out,
                           out_stride, batch, start, n, channels, params, lines, state, max_line);
    } else {
        hipLaunchKernelGGL(k_karplus_strong<false>, dim3(grid), dim3(kKsLanes), 0, pgx::stream(), out, out_stride,
                           batch, start, n, channels, params, lines, state, max_line);
    }
    PGX_LAUNCH_CHECK("k_karplus_strong");
    return PGX_OK;
}

int pgx_karplus_score(float *out, int channels, const pgx_ks_note *notes, int count, int group, int max_line,
                      int notes_on_host) {
    PGX_REQUIRE_INIT();
    if (count <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && notes && channels >= 1 && group >= 1 && group <= kKsLanes && max_line >= 2 &&
                      (!notes_on_host || count <= kKsInline),
                  "pgx_karplus_score: bad argument");
    const int grid = (int)pgx::ceil_div(count, group);
    const int lanes = count < group ? count : group;
    int64_t lds = (int64_t)lanes * max_line * (int64_t)sizeof(float);
    if (lds > kKsLdsBytes) lds = kKsLdsBytes;
    const int lds_floats = (int)(lds / (int64_t)sizeof(float));
    if (notes_on_host) {
        KsInline inl = {};
        for (int i = 0; i < count; ++i) inl.n[i] = notes[i];
        hipLaunchKernelGGL(k_karplus_score_inline, dim3(grid), dim3(kKsLanes), (size_t)lds, pgx::stream(), out,
                           channels, inl, count, group, max_line, lds_floats);
    } else {
        hipLaunchKernelGGL(k_karplus_score, dim3(grid), dim3(kKsLanes), (size_t)lds, pgx::stream(), out, channels,
                           notes, count, group, max_line, lds_floats);
    }
    PGX_LAUNCH_CHECK("k_karplus_score");
    return PGX_OK;
}

size_t pgx_analog_osc_workspace_bytes(int64_t n) {
    if (n <= 0) return 0;
    const int64_t nb = pgx::ceil_div(n, kOscTile);
    return (size_t)(2 * osc_ws_doubles(nb)) * sizeof(double);
}

size_t pgx_analog_osc_bank_workspace_bytes(int64_t n, int batch) {
    if (n <= 0 || batch <= 0) return 0;
    return (size_t)batch * pgx_analog_osc_workspace_bytes(n);
}

// `batch` voices (the single PE: 1, a.params NULL): the voice is the grid's y of a pass and the x of a scan.
static int osc_launch(float *out, const OscArgs &a, int batch, void *workspace, double *state, int restart,
                      bool pure) {
    const int64_t nb = pgx::ceil_div(a.n, kOscTile);
    PGX_CHECK_ARG(nb < (int64_t)1 << 31, "pgx_analog_osc: too many frames");
    PGX_CHECK_ARG(batch <= 65535, "pgx_analog_osc: too many voices");
    double *ws = static_cast<double *>(workspace);
    double *ws2 = ws + osc_ws_doubles(nb);
    const dim3 b(kOscBlock), voices((unsigned)batch);
    hipStream_t s = pgx::stream();
    if (a.p.waveform == 0 && pure) {
        hipLaunchKernelGGL(k_osc_pure_rect, dim3(pgx::grid_for(a.n, kOscBlock), (unsigned)batch), b, 0, s, out, a);
        PGX_LAUNCH_CHECK("k_osc_pure_rect");
        return PGX_OK;
    }
    const dim3 g((unsigned)nb, (unsigned)batch);
    const bool saw = a.p.waveform != 0;
    if (pure) {
        hipLaunchKernelGGL((k_osc_pass<true, 1>), g, b, 0, s, out, a, ws, ws2, nb);
        hipLaunchKernelGGL((k_osc_scan<2>), voices, b, 0, s, ws, nb, state, restart, a);
        hipLaunchKernelGGL((k_osc_pass<true, 2>), g, b, 0, s, out, a, ws, ws2, nb);
    } else {
        hipLaunchKernelGGL((k_osc_pass<false, 0>), g, b, 0, s, out, a, ws, ws2, nb);
        hipLaunchKernelGGL((k_osc_scan<0>), voices, b, 0, s, ws, nb, state, restart, a);
        hipLaunchKernelGGL((k_osc_pass<false, 1>), g, b, 0, s, out, a, ws, ws2, nb);
        if (saw) {
            hipLaunchKernelGGL((k_osc_scan<1>), voices, b, 0, s, ws2, nb, state, restart, a);
            hipLaunchKernelGGL((k_osc_pass<false, 2>), g, b, 0, s, out, a, ws, ws2, nb);
        }
    }
    PGX_LAUNCH_CHECK("k_osc_pass");
    return PGX_OK;
}

int pgx_analog_osc_pure(float *out, int64_t start, int64_t n, int channels, double sample_rate, int waveform,
                        double freq, double duty, void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && channels >= 1 && sample_rate > 0 && (waveform == 0 || waveform == 1),
                  "pgx_analog_osc_pure: bad argument");
    PGX_CHECK_ARG(waveform == 0 || workspace, "pgx_analog_osc_pure: the sawtooth needs a workspace");
    OscArgs a{{freq, duty, sample_rate, waveform}, start, n, channels, nullptr, nullptr, nullptr, 0, 0, 0};
    return osc_launch(out, a, 1, workspace, nullptr, 0, true);
}

int pgx_analog_osc_stateful(float *out, int64_t n, int channels, double sample_rate, int waveform, double freq,
                            double duty, const float *freq_stream, const float *duty_stream, int restart,
                            double *state, void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && state && workspace && channels >= 1 && sample_rate > 0 && (waveform == 0 || waveform == 1),
                  "pgx_analog_osc_stateful: bad argument");
    OscArgs a{{freq, duty, sample_rate, waveform}, 0, n, channels, freq_stream, duty_stream, nullptr, 0, 0, 0};
    return osc_launch(out, a, 1, workspace, state, restart, false);
}

int pgx_analog_osc_bank(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                        double sample_rate, int waveform, const pgx_osc_params *params, const float *freq_streams,
                        int64_t freq_stride, const float *duty_streams, int64_t duty_stride, int stateful, int restart,
                        double *state, void *workspace) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(batch >= 0, "pgx_analog_osc_bank: bad argument");
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && params && channels >= 1 && sample_rate > 0 && (waveform == 0 || waveform == 1) &&
                      out_stride >= n * channels && (!freq_streams || freq_stride >= n) &&
                      (!duty_streams || duty_stride >= n),
                  "pgx_analog_osc_bank: bad argument");
    if (stateful) {
        PGX_CHECK_ARG(state && workspace, "pgx_analog_osc_bank: the stateful form needs state and workspace");
    } else {
        PGX_CHECK_ARG(!freq_streams && !duty_streams, "pgx_analog_osc_bank: the pure form takes no streams");
        PGX_CHECK_ARG(waveform == 0 || workspace, "pgx_analog_osc_bank: the sawtooth needs a workspace");
    }
    OscArgs a{{0.0, 0.0, sample_rate, waveform}, stateful ? 0 : start, n, channels, freq_streams, duty_streams, params,
              out_stride, freq_stride, duty_stride};
    return osc_launch(out, a, batch, workspace, stateful ? state : nullptr, stateful ? restart : 0, !stateful);
}

}  // extern "C"
