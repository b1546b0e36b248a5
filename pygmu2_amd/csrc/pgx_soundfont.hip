// pgx_soundfont.hip -- the audio plane of MeltysynthPE: SoundFont voices played from a render table.
//
// The control plane (pygmu2_amd/soundfont/synth.py) runs once per block per voice on the host and emits one table row per
// (block, audible voice).  This unit turns `n_blocks` blocks of such rows into samples in two launches:
//
//   k_soundfont_voices   one wave per voice object, its rows in block order: the oscillator with lanes as frames (a
//                        sample-table gather with linear interpolation, the reference's numpy fill paths), then the
//                        direct-form biquad one frame after another.  Of y = a0*x + a1*x1 + a2*x2 - a3*y1 - a4*y2, summed
//                        left to right, the first three terms depend on the input alone and are summed per lane; lane 0
//                        then walks (s - a3*y1) - a4*y2 through the chunk.  Same operations, same order, same bits.  The
//                        filtered block goes to scratch[row]; the filter state lives in HBM per voice object.
//   k_soundfont_mix      one thread per output frame: dest = 0.0, then dest = dest + g * x for the rows of its block in
//                        table order, g the constant or a + step * t; a skipped row is left out; one rounding to float32.
//
// No index leaves the wave data: a gather at an index outside [0, wave_len) reads 0.0 (the reference would raise).
// The entry reads the integer columns back and refuses a table it cannot play before anything is launched.

#include <vector>

#include "pgx_common.h"

namespace {

constexpr int kIC = PGX_SOUNDFONT_ICOLS, kDC = PGX_SOUNDFONT_DCOLS;
constexpr int I_VOICE = 0, I_FLAGS = 1, I_END = 2, I_START_LOOP = 3, I_END_LOOP = 4, I_MIX_L = 5, I_MIX_R = 6;
constexpr int D_POSITION = 0, D_RATIO = 1, D_A0 = 2, D_MIX_L = 7, D_MIX_R = 9;
constexpr int F_CLEAR = 1, F_LOOP = 2, F_FILTER = 4;
constexpr int MIX_SKIP = 0, MIX_CONST = 1, MIX_SLOPE = 2;

__device__ __forceinline__ double wave_at(const int16_t *wave, int64_t wave_len, int64_t i) {
    return (i >= 0 && i < wave_len) ? (double)wave[i] * (1.0 / 32768.0) : 0.0;
}

__device__ __forceinline__ int64_t index_of(double position) {      // astype(np.intp); out of range (or NaN): no frame
    return (position > -9.0e18 && position < 9.0e18) ? (int64_t)position : (int64_t)-1;
}

// numpy's float remainder (sign of the divisor) over C's fmod
__device__ __forceinline__ double np_mod(double a, double b) {
    double m = fmod(a, b);
    if (b == 0.0) return m;
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

__global__ __launch_bounds__(64) void k_soundfont_voices(double *__restrict__ scratch, double *__restrict__ filter_state,
                                                         const int16_t *__restrict__ wave, int64_t wave_len,
                                                         const int32_t *__restrict__ block_rows,
                                                         const int32_t *__restrict__ rows_i,
                                                         const double *__restrict__ rows_d, int64_t n_blocks,
                                                         int block_size) {
    __shared__ double xs[64 + 2];      // x2, x1, then the chunk's input
    __shared__ double ys[64];
    const int voice = blockIdx.x, lane = threadIdx.x;
    double *state = filter_state + 4 * (int64_t)voice;      // x1, x2, y1, y2
    double y1 = state[2], y2 = state[3];                     // lane 0's are the live ones
    if (lane == 0) {
        xs[0] = state[1];
        xs[1] = state[0];
    }
    __syncthreads();
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int first = block_rows[b], last = block_rows[b + 1];
        int row = -1;
        for (int base = first; base < last; base += 64) {
            const int r = base + lane;
            const bool mine = r < last && rows_i[(int64_t)r * kIC + I_VOICE] == voice;
            const unsigned long long hits = __ballot(mine);
            if (hits) {
                row = base + __ffsll((long long)hits) - 1;
                break;
            }
        }
        if (row < 0) continue;                               // wave-uniform
        const int32_t *ri = rows_i + (int64_t)row * kIC;
        const double *rd = rows_d + (int64_t)row * kDC;
        const int flags = ri[I_FLAGS];
        const int64_t end = ri[I_END], start_loop = ri[I_START_LOOP], end_loop = ri[I_END_LOOP];
        const double position = rd[D_POSITION], ratio = rd[D_RATIO];
        const double a0 = rd[D_A0], a1 = rd[D_A0 + 1], a2 = rd[D_A0 + 2], a3 = rd[D_A0 + 3], a4 = rd[D_A0 + 4];
        const bool looping = flags & F_LOOP, filtering = flags & F_FILTER;
        const double loop_start = (double)start_loop, loop_length = (double)(end_loop - start_loop);
        double *dst = scratch + (int64_t)row * block_size;
        if (flags & F_CLEAR) {
            y1 = y2 = 0.0;
            if (lane == 0) xs[0] = xs[1] = 0.0;
        }
        __syncthreads();
        for (int t0 = 0; t0 < block_size; t0 += 64) {
            const int count = min(64, block_size - t0), t = t0 + lane;
            if (lane < count) {
                const double p = position + (double)t * ratio;
                double x = 0.0;
                if (looping) {
                    const double w = np_mod(p - loop_start, loop_length) + loop_start;
                    const int64_t lo = index_of(w);
                    const double frac = w - (double)lo;
                    int64_t hi = lo + 1;
                    if (hi >= end_loop) hi = start_loop;
                    x = (1.0 - frac) * wave_at(wave, wave_len, lo) + frac * wave_at(wave, wave_len, hi);
                } else if (p < (double)end) {
                    const int64_t lo = index_of(p);
                    const double frac = p - (double)lo;
                    x = (1.0 - frac) * wave_at(wave, wave_len, lo) + frac * wave_at(wave, wave_len, lo + 1);
                }
                xs[2 + lane] = x;
            }
            __syncthreads();
            if (filtering) {
                if (lane < count) ys[lane] = a0 * xs[2 + lane] + a1 * xs[1 + lane] + a2 * xs[lane];
                __syncthreads();
                if (lane == 0) {
                    for (int i = 0; i < count; ++i) {
                        const double y = ys[i] - a3 * y1 - a4 * y2;
                        y2 = y1;
                        y1 = y;
                        ys[i] = y;
                    }
                }
                __syncthreads();
                if (lane < count) dst[t] = ys[lane];
            } else if (lane < count) {
                dst[t] = xs[2 + lane];
            }
            __syncthreads();
            if (lane == 0) {                                 // the chunk's last two inputs are the next one's x2, x1
                const double nx2 = xs[count], nx1 = xs[count + 1];
                xs[0] = nx2;
                xs[1] = nx1;
            }
            __syncthreads();
        }
        if (!filtering) {                                    // an inactive filter loads its state from the block's end
            y2 = xs[0];
            y1 = xs[1];
        }
    }
    if (lane == 0) {
        state[0] = xs[1];
        state[1] = xs[0];
        state[2] = y1;
        state[3] = y2;
    }
}

__device__ __forceinline__ double mix_add(double dest, int mode, double a, double step, int t, double x) {
    if (mode == MIX_CONST) return dest + a * x;
    if (mode == MIX_SLOPE) return dest + (a + step * (double)t) * x;
    return dest;
}

__global__ __launch_bounds__(256) void k_soundfont_mix(float *__restrict__ out, float *__restrict__ carry,
                                                       const double *__restrict__ scratch,
                                                       const int32_t *__restrict__ block_rows,
                                                       const int32_t *__restrict__ rows_i,
                                                       const double *__restrict__ rows_d, int64_t n_blocks,
                                                       int block_size, int64_t n_frames) {
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_blocks * block_size) return;
    const int64_t b = f / block_size;
    const int t = (int)(f - b * block_size);
    double left = 0.0, right = 0.0;
    for (int r = block_rows[b]; r < block_rows[b + 1]; ++r) {
        const int32_t *ri = rows_i + (int64_t)r * kIC;
        const double *rd = rows_d + (int64_t)r * kDC;
        const int ml = ri[I_MIX_L], mr = ri[I_MIX_R];
        if (ml == MIX_SKIP && mr == MIX_SKIP) continue;
        const double x = scratch[(int64_t)r * block_size + t];
        left = mix_add(left, ml, rd[D_MIX_L], rd[D_MIX_L + 1], t, x);
        right = mix_add(right, mr, rd[D_MIX_R], rd[D_MIX_R + 1], t, x);
    }
    float *dst = f < n_frames ? out + 2 * f : carry + 2 * (f - n_frames);
    dst[0] = (float)left;
    dst[1] = (float)right;
}

}  // namespace

extern "C" int pgx_soundfont_render(float *out, int64_t n_frames, float *carry, const int16_t *wave, int64_t wave_len,
                                    const int32_t *block_rows, const int32_t *rows_i, const double *rows_d,
                                    int64_t n_rows, int64_t n_blocks, int block_size, double *filter_state,
                                    int polyphony, double *scratch) {
    // arguments first: a bad call is refused whether or not a device is up
    PGX_CHECK_ARG(block_size >= 8 && block_size <= 1024, "pgx_soundfont_render: block_size outside 8 .. 1024");
    PGX_CHECK_ARG(polyphony >= 1 && polyphony <= 256, "pgx_soundfont_render: polyphony outside 1 .. 256");
    PGX_CHECK_ARG(n_blocks >= 0 && n_blocks < (1 << 20) && n_rows >= 0 && n_rows <= n_blocks * polyphony &&
                      wave_len >= 0,
                  "pgx_soundfont_render: bad count");
    PGX_CHECK_ARG(n_frames >= 0 && n_frames <= n_blocks * block_size && n_blocks * block_size - n_frames <= block_size,
                  "pgx_soundfont_render: n_frames does not end in the last block");
    PGX_CHECK_ARG(out && carry && wave && block_rows && rows_i && rows_d && filter_state && scratch,
                  "pgx_soundfont_render: null pointer");
    PGX_REQUIRE_INIT();
    if (n_blocks == 0) return PGX_OK;

    // the integer columns come back to the host: nothing is launched over a table that cannot be played
    std::vector<int32_t> offsets((size_t)n_blocks + 1), cols((size_t)n_rows * kIC);
    PGX_HIP(hipMemcpyAsync(offsets.data(), block_rows, offsets.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                           pgx::stream()));
    if (n_rows)
        PGX_HIP(hipMemcpyAsync(cols.data(), rows_i, cols.size() * sizeof(int32_t), hipMemcpyDeviceToHost,
                               pgx::stream()));
    PGX_HIP(hipStreamSynchronize(pgx::stream()));
    PGX_CHECK_ARG(offsets[0] == 0 && offsets[(size_t)n_blocks] == n_rows, "pgx_soundfont_render: block_rows does not span the rows");
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t first = offsets[(size_t)b], last = offsets[(size_t)b + 1];
        PGX_CHECK_ARG(first <= last && last - first <= polyphony && last <= n_rows,
                      "pgx_soundfont_render: a block has more rows than voices");
        bool seen[256] = {};
        for (int64_t r = first; r < last; ++r) {
            const int32_t *ri = cols.data() + r * kIC;
            PGX_CHECK_ARG(ri[I_VOICE] >= 0 && ri[I_VOICE] < polyphony, "pgx_soundfont_render: voice id outside the polyphony");
            PGX_CHECK_ARG(!seen[ri[I_VOICE]], "pgx_soundfont_render: a voice appears twice in one block");
            seen[ri[I_VOICE]] = true;
            PGX_CHECK_ARG(ri[I_MIX_L] >= MIX_SKIP && ri[I_MIX_L] <= MIX_SLOPE && ri[I_MIX_R] >= MIX_SKIP &&
                              ri[I_MIX_R] <= MIX_SLOPE,
                          "pgx_soundfont_render: unknown mix mode");
        }
    }

    if (n_rows) {
        hipLaunchKernelGGL(k_soundfont_voices, dim3(polyphony), dim3(64), 0, pgx::stream(), scratch, filter_state, wave,
                           wave_len, block_rows, rows_i, rows_d, n_blocks, block_size);
        PGX_LAUNCH_CHECK("k_soundfont_voices");
    }
    const int64_t frames = n_blocks * block_size;
    hipLaunchKernelGGL(k_soundfont_mix, dim3((unsigned)pgx::ceil_div(frames, 256)), dim3(256), 0, pgx::stream(), out, carry,
                       (const double *)scratch, block_rows, rows_i, rows_d, n_blocks, block_size, n_frames);
    PGX_LAUNCH_CHECK("k_soundfont_mix");
    return PGX_OK;
}
