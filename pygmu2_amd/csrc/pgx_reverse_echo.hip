// pgx_reverse_echo.hip -- ReversePitchEchoPE (pgx_reverse_echo).
//
// The reference runs three stages in one per-sample loop (reverse_pitch_echo_pe.py, _reverse_pitch_echo_numba): a
// one-pole on the echo-block size, a two-head time-domain pitch shifter over a circular buffer, and a double-buffered
// echo whose previous block is played back reversed (or alternately forward) under a Hann window.  Only three things in
// it are sequential: the scalar recurrences (smoothed size, read position), the walk over echo-block boundaries, and
// the dependency of echo block k on echo block k-1.  Three launches, stream-ordered, no workgroup talks to another:
//   * plan  (one workgroup): the smoothed size as a float64 affine scan and the read position as a float64 prefix sum,
//           tile by tile, into the workspace; then one lane walks the echo-block boundaries (one step per echo block
//           of >= 64 frames) into a table of segments and writes the carried record for the next render;
//   * pitch (grid-wide, a thread per frame and channel): the two interpolated heads, gathered by TIME from
//           [carried history | this window's input] -- slot s of the reference's circular buffer holds, at frame t, the
//           input of frame t - ((write slot - s) mod len) -- into a float64 workspace array; the last `len` inputs
//           become the other half of the history;
//   * echo  (one workgroup per channel): loops over the table; inside an echo block every frame is independent, the
//           threads stride over it; one __syncthreads() between consecutive segments.
// Discontinuous decisions (rint of the target and of the smoothed size, the unity bypass, alternate >= 0.5, the clamps)
// use the reference's operations on the widened float32 inputs; the smoothed size, the read position and the window
// are continuous in the output and are re-associated.

#include "pgx_common.h"

namespace {

constexpr int kPlanBlock = 256;
constexpr int kPlanWaves = kPlanBlock / 64;
constexpr int kPitchBlock = 256;
constexpr int kEchoBlock = 512;
constexpr int64_t kMinBlock = PGX_REVERSE_ECHO_MIN_BLOCK;
constexpr double kMaxFeedback = PGX_REVERSE_ECHO_MAX_FEEDBACK;
constexpr double kMinRatio = PGX_REVERSE_ECHO_MIN_RATIO;
constexpr double kUnityBand = PGX_REVERSE_ECHO_UNITY_BAND;

// what the later launches need of the record as it stood BEFORE this render
struct Header {
    int64_t segments;
    int64_t pitch_write_pos;
    int32_t pitch_parity;
    int32_t pad;
};

// the part of one echo block that lies inside this render
struct Segment {
    int64_t first;       // frame of the window
    int64_t count;
    int64_t write_idx;   // == read index, at `first`
    int64_t prev_len;
    int32_t reverse;
    int32_t current_is_a;
};

struct Layout {
    size_t table, smoothed, read_pos, pitched, total;
    int64_t capacity;
};
inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }
inline Layout layout(int64_t n, int channels) {
    Layout l;
    l.capacity = n / kMinBlock + 2;                       // a partial block at either end, whole ones between
    l.table = align16(sizeof(Header));
    l.smoothed = align16(l.table + (size_t)l.capacity * sizeof(Segment));
    l.read_pos = l.smoothed + (size_t)n * sizeof(double);
    l.pitched = l.read_pos + (size_t)n * sizeof(double);
    l.total = l.pitched + (size_t)n * (size_t)channels * sizeof(double);
    return l;
}

__device__ __forceinline__ double control(const float *stream, double scalar, int64_t t) {
    return stream ? (double)stream[t] : scalar;          // the reference's .astype(np.float64)
}

// reverse_pitch_echo_pe.py:87-94
__device__ __forceinline__ double target_samples(double seconds, double sr, int64_t rows) {
    double t = seconds * sr;
    const double lo = (double)kMinBlock, hi = (double)(rows - 1);
    if (!isfinite(t)) t = lo;
    if (t < lo) t = lo;
    if (t > hi) t = hi;
    return rint(t);
}

// :99-103
__device__ __forceinline__ int64_t locked_block(double smoothed, int64_t rows) {
    const double r = rint(smoothed);
    int64_t b = (r >= (double)kMinBlock) ? ((r <= (double)(rows - 1)) ? (int64_t)r : rows - 1) : kMinBlock;   // NaN: 64
    return b;
}

// :106-108; a NaN ratio (the reference fails on it) counts as the smallest
__device__ __forceinline__ double clamped_ratio(double r) { return (r >= kMinRatio) ? r : kMinRatio; }

__device__ __forceinline__ double wrap(double x, double len) {
    double r = x - len * floor(x / len);
    if (r >= len) r -= len;
    return (r >= 0.0) ? r : 0.0;
}

__global__ void __launch_bounds__(kPlanBlock)
k_reverse_echo_plan(pgx_reverse_echo_state *state, Header *header, Segment *table, int64_t capacity, double *smoothed_ws,
                    double *read_pos_ws, const float *block_stream, double block_scalar, const float *pitch_stream,
                    double pitch_scalar, const float *alt_stream, double alt_scalar, int64_t n, double sr, int64_t rows,
                    int64_t len, double alpha) {
    __shared__ double lds[2 * kPlanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const pgx_reverse_echo_state s0 = *state;
    double smoothed = s0.smoothed, pos = s0.read_pos;
    const double dlen = (double)len;
    for (int64_t base = 0; base < n; base += kPlanBlock) {
        const int64_t t = base + threadIdx.x;
        const bool live = t < n;
        if (block_stream) {
            // s' = (1 - alpha) s + alpha target as a scan of affine maps s -> A s + B (later o earlier)
            double A = 1.0, B = 0.0;
            if (live) {
                A = 1.0 - alpha;
                B = alpha * target_samples((double)block_stream[t], sr, rows);
            }
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double oA = __shfl_up(A, d, 64), oB = __shfl_up(B, d, 64);
                if (lane >= d) {
                    B = A * oB + B;
                    A = A * oA;
                }
            }
            if (lane == 63) {
                lds[wave] = A;
                lds[kPlanWaves + wave] = B;
            }
            __syncthreads();
            double in = smoothed, all = smoothed;
#pragma unroll
            for (int w = 0; w < kPlanWaves; ++w) {
                const double wA = lds[w], wB = lds[kPlanWaves + w];
                if (w < wave) in = wA * in + wB;
                all = wA * all + wB;
            }
            __syncthreads();
            if (live) smoothed_ws[t] = A * in + B;
            smoothed = all;
        }
        double total;
        const double ratio = live ? clamped_ratio(control(pitch_stream, pitch_scalar, t)) : 0.0;
        const double before = pgx::block_excl_sum<kPlanWaves>(ratio, lds, total);
        if (live) read_pos_ws[t] = wrap(pos + before, dlen);
        pos = wrap(pos + total, dlen);
    }
    if (!block_stream) smoothed = target_samples(block_scalar, sr, rows);   // the one-pole rests on a constant target
    __syncthreads();                                      // smoothed_ws is read below by one lane
    if (threadIdx.x != 0) return;
    int64_t w = s0.write_idx, cur = s0.current_block, prev = s0.prev_len, k = 0;
    int32_t reverse = s0.reverse, is_a = s0.current_is_a;
    for (int64_t t = 0; t < n && k < capacity;) {
        if (w == 0) cur = locked_block(block_stream ? smoothed_ws[t] : smoothed, rows);
        const int64_t left = cur - w > 0 ? cur - w : 1;
        const int64_t count = left < n - t ? left : n - t;
        Segment seg;
        seg.first = t;
        seg.count = count;
        seg.write_idx = w;
        seg.prev_len = prev;
        seg.reverse = reverse;
        seg.current_is_a = is_a;
        table[k++] = seg;
        t += count;
        w += count;
        if (w >= cur) {                                   // :240-252, at the block's last frame
            is_a = 1 - is_a;
            prev = cur;
            w = 0;
            reverse = (control(alt_stream, alt_scalar, t - 1) >= 0.5) ? 1 - reverse : 1;
        }
    }
    Header h;
    h.segments = k;
    h.pitch_write_pos = s0.pitch_write_pos;
    h.pitch_parity = s0.pitch_parity;
    h.pad = 0;
    *header = h;
    pgx_reverse_echo_state s1 = s0;
    s1.smoothed = smoothed;
    s1.read_pos = pos;
    s1.write_idx = s1.read_idx = w;
    s1.current_block = cur;
    s1.prev_len = prev;
    s1.reverse = reverse;
    s1.current_is_a = is_a;
    s1.pitch_write_pos = (s0.pitch_write_pos + n) % len;
    s1.pitch_parity = 1 - s0.pitch_parity;
    *state = s1;
}

// The input of frame m of the window, or of the carried history for m < 0 (m > -len): history row j holds frame j - len.
__device__ __forceinline__ double input_at(const float *in, const double *hist, int64_t m, int64_t len, int channels,
                                           int c) {
    return m >= 0 ? (double)in[m * channels + c] : hist[(len + m) * channels + c];
}

__global__ void __launch_bounds__(kPitchBlock)
k_reverse_echo_pitch(double *pitched, double *hist_all, const Header *header, const double *read_pos_ws, const float *in,
                     const float *pitch_stream, double pitch_scalar, int64_t n, int channels, int64_t len) {
    const int64_t g = (int64_t)blockIdx.x * kPitchBlock + threadIdx.x;
    const int64_t t = g / channels;
    const int c = (int)(g - t * channels);
    const Header h = *header;
    const double *hist = hist_all + (int64_t)h.pitch_parity * len * channels;
    if (t < len)                                          // the history the next render starts from: frames n - len .. n - 1
        hist_all[(int64_t)(1 - h.pitch_parity) * len * channels + g] = input_at(in, hist, n - len + t, len, channels, c);
    if (t >= n) return;
    const double ratio = clamped_ratio(control(pitch_stream, pitch_scalar, t));
    if (fabs(ratio - 1.0) < kUnityBand) {                 // :118-124
        pitched[g] = (double)in[g];
        return;
    }
    const double dlen = (double)len, half = dlen / 2.0;
    const double rp = read_pos_ws[t];
    // :164-179 (rp lies in [0, len): `% len` is the identity)
    int64_t idx0 = (int64_t)floor(rp);
    idx0 = idx0 < 0 ? 0 : (idx0 > len - 1 ? len - 1 : idx0);
    const int64_t idx1 = idx0 + 1 >= len ? 0 : idx0 + 1;
    const double frac = rp - (double)idx0;
    double pos2 = rp + half;
    if (pos2 >= dlen) pos2 -= dlen;
    int64_t idx2 = (int64_t)floor(pos2);
    idx2 = idx2 < 0 ? 0 : (idx2 > len - 1 ? len - 1 : idx2);
    const int64_t idx3 = idx2 + 1 >= len ? 0 : idx2 + 1;
    const double frac2 = pos2 - (double)idx2;
    // :183-188, against the write position after its increment
    const int64_t slot = (h.pitch_write_pos + t) % len;  // where frame t was just written
    const int64_t wp = slot + 1 >= len ? 0 : slot + 1;
    double dist = fabs(rp - (double)wp);
    if (dist > half) dist = dlen - dist;
    const double f = dist / half;
    // slot s holds the input of frame t - ((slot - s) mod len)
    const double b0 = input_at(in, hist, t - (slot - idx0 + len) % len, len, channels, c);
    const double b1 = input_at(in, hist, t - (slot - idx1 + len) % len, len, channels, c);
    const double b2 = input_at(in, hist, t - (slot - idx2 + len) % len, len, channels, c);
    const double b3 = input_at(in, hist, t - (slot - idx3 + len) % len, len, channels, c);
    const double s1 = (1.0 - frac) * b0 + frac * b1;      // :197-200
    const double s2 = (1.0 - frac2) * b2 + frac2 * b3;
    pitched[g] = f * s1 + (1.0 - f) * s2;
}

__global__ void __launch_bounds__(kEchoBlock)
k_reverse_echo_echo(float *out, double *echo_a, double *echo_b, const Header *header, const Segment *table,
                    const double *pitched, const float *fb_stream, double fb_scalar, int channels) {
    const int c = blockIdx.x;
    const int64_t segments = header->segments;
    for (int64_t k = 0; k < segments; ++k) {
        const Segment seg = table[k];
        double *current = seg.current_is_a ? echo_a : echo_b;
        const double *previous = seg.current_is_a ? echo_b : echo_a;
        const double span = seg.prev_len > 1 ? (double)seg.prev_len - 1.0 : 1.0;
        for (int64_t i = threadIdx.x; i < seg.count; i += kEchoBlock) {
            const int64_t t = seg.first + i, w = seg.write_idx + i;
            double wet = 0.0;                             // :134-146
            if (w < seg.prev_len) {
                const int64_t idx = seg.reverse ? seg.prev_len - 1 - w : w;
                const double pos = seg.prev_len > 1 ? (double)w / span : 0.0;
                const double window = 0.5 - 0.5 * cos(2.0 * M_PI * pos);
                wet = previous[idx * channels + c] * window;
            }
            double fb = control(fb_stream, fb_scalar, t);  // :149-155
            if (!isfinite(fb)) fb = 0.0;
            if (fb > kMaxFeedback) fb = kMaxFeedback;
            if (fb < -kMaxFeedback) fb = -kMaxFeedback;
            current[w * channels + c] = pitched[t * channels + c] + wet * fb;
            out[t * channels + c] = (float)wet;
        }
        __syncthreads();                                  // block k's writes before block k + 1's reads
    }
}

}  // namespace

extern "C" {

size_t pgx_reverse_echo_workspace_bytes(int64_t n, int channels) {
    if (n < 1 || channels < 1) return 0;
    return layout(n, channels).total;
}

int pgx_reverse_echo(float *out, const float *in, int64_t n, int channels, double sample_rate, double block_seconds,
                     const float *block_stream, double pitch_ratio, const float *pitch_stream, double feedback,
                     const float *feedback_stream, double alternate, const float *alternate_stream,
                     int64_t smoothing_samples, pgx_reverse_echo_state *state, double *echo_a, double *echo_b,
                     int64_t rows, double *pitch_history, int64_t pitch_len, void *workspace) {
    // arguments first: a bad call is refused whether or not a device is up
    PGX_CHECK_ARG(n >= 0 && channels >= 1 && rows > kMinBlock && pitch_len >= 2 && smoothing_samples >= 1 &&
                      sample_rate > 0.0 && sample_rate <= 1e9,
                  "pgx_reverse_echo: bad argument");
    PGX_CHECK_ARG(state && echo_a && echo_b && pitch_history && (n == 0 || (out && in && workspace)),
                  "pgx_reverse_echo: null pointer");
    PGX_REQUIRE_INIT();
    if (n == 0) return PGX_OK;
    const Layout l = layout(n, channels);
    char *ws = static_cast<char *>(workspace);
    Header *header = reinterpret_cast<Header *>(ws);
    Segment *table = reinterpret_cast<Segment *>(ws + l.table);
    double *smoothed_ws = reinterpret_cast<double *>(ws + l.smoothed);
    double *read_pos_ws = reinterpret_cast<double *>(ws + l.read_pos);
    double *pitched = reinterpret_cast<double *>(ws + l.pitched);
    hipLaunchKernelGGL(k_reverse_echo_plan, dim3(1), dim3(kPlanBlock), 0, pgx::stream(), state, header, table, l.capacity,
                       smoothed_ws, read_pos_ws, block_stream, block_seconds, pitch_stream, pitch_ratio, alternate_stream,
                       alternate, n, sample_rate, rows, pitch_len, 1.0 / (double)smoothing_samples);
    PGX_LAUNCH_CHECK("k_reverse_echo_plan");
    const int64_t items = (n > pitch_len ? n : pitch_len) * channels;
    hipLaunchKernelGGL(k_reverse_echo_pitch, dim3((unsigned)pgx::ceil_div(items, kPitchBlock)), dim3(kPitchBlock), 0,
                       pgx::stream(), pitched, pitch_history, (const Header *)header, (const double *)read_pos_ws, in,
                       pitch_stream, pitch_ratio, n, channels, pitch_len);
    PGX_LAUNCH_CHECK("k_reverse_echo_pitch");
    hipLaunchKernelGGL(k_reverse_echo_echo, dim3(channels), dim3(kEchoBlock), 0, pgx::stream(), out, echo_a, echo_b,
                       (const Header *)header, (const Segment *)table, (const double *)pitched, feedback_stream, feedback,
                       channels);
    PGX_LAUNCH_CHECK("k_reverse_echo_echo");
    return PGX_OK;
}

}  // extern "C"
