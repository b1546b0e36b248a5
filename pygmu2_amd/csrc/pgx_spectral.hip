// pgx_spectral.hip -- arbitrary-length float64 DFT (pgx_dft_*) and TralfamPE's whole-extent pipeline (pgx_tralfam).
//
// (a) Power-of-two complex FFT, M = 2^m, m = 0..22, batch B, forward or inverse, natural order in and out.
//     One kernel, k_fft_pass: a workgroup holds a tile of 2048 complex points in LDS -- 2^(11-l) sequences of length
//     2^l -- and transforms them with an in-place Stockham radix-4 (+ one radix-2) FFT: every stage reads its operands
//     into registers, barrier, writes its results to the same image, barrier.  The tile's twiddles W_L^p sit in a
//     second LDS table (32 KB + 32 KB = the 64 KB a kernel gets without asking).
//       m <= 11: one launch; the sequences of a tile are batch items.
//       m >= 12: the four-step decomposition  i = i1*N2 + i2,  k = k1 + N1*k2,  N1 = 2^floor(m/2), N2 = M / N1:
//                pass 1  length-N1 FFTs down the columns i2, times W_M^(i2*k1)      in[i1][i2]   -> tmp[k1][i2]
//                pass 2  length-N2 FFTs along the rows k1, written transposed       tmp[k1][i2]  -> out[k1 + N1*k2]
//     A tile is 2048/N1 adjacent columns resp. 2048/N2 adjacent rows; global accesses run along whichever index is
//     contiguous in memory (16 lanes x 16 B at m = 14, one lane at m = 22: the long transforms pay for the natural
//     output order with narrow accesses -- DESIGN.md section 7).  HBM traffic: 32 B per point and pass.
//     Every twiddle is evaluated, never recurred: the index is reduced in integers to an eighth of a turn (p / 2^l is
//     exact), then the float64 polynomials of pgx_common.h on |angle| <= pi/4.
//     The inverse is conj -> forward -> conj, folded into the first load and the last store.
// (b) Any other length N <= 2^21 by Bluestein's chirp-z on top of (a):  M = 2^ceil(log2(2N-1)),
//     b_k = exp(i*pi*(k^2 mod 2N)/N) with k^2 mod 2N in 64-bit integers, reduced to an eighth of a turn in integers
//     before the polynomials;  X = conj(b) . IFFT_M(FFT_M(x . conj(b), zero padded) . FFT_M(b wrapped)).
//     The chirp and its spectrum depend on N alone: pgx_dft_plan makes them once.
// (c) TralfamPE (tralfam_pe.py:70-105): float32 (N, C) -> C complex sequences -> DFT -> |X| . exp(i*phi), phi from draw
//     k*C + c of the seeded PCG64 stream as rng.random((N, C)) * 2.0 * pi -> inverse DFT -> real part as float32 (N, C)
//     with the max |y| of the float32 result reduced on the way -> optional in-place scale by
//     float32(normalize_peak) / peak.  The peak never leaves the device.

#include "pgx_pcg.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileLog2 = 11;
constexpr int kTile = 1 << kTileLog2;
constexpr int kPerThread = kTile / kBlock;                 // 8 points of the tile per thread
constexpr int kMaxLog2 = 22;                               // largest power-of-two transform
constexpr int64_t kMaxLength = (int64_t)1 << 21;           // largest N: Bluestein needs M >= 2N - 1
constexpr size_t kHeadBytes = 256;                         // front of a workspace: the peak word of pgx_tralfam
constexpr int kDrawRun = 4;                                // consecutive draws per lane of k_tralfam_phase
constexpr double kHalfPi = 1.5707963267948966;

struct alignas(16) cplx {
    double x, y;
};
// explicit FMAs: the transforms are bound to float64 accuracy, not to a reference operation order
__device__ __forceinline__ cplx cmul(const cplx &a, const cplx &b) {
    return cplx{__builtin_fma(a.x, b.x, -(a.y * b.y)), __builtin_fma(a.x, b.y, a.y * b.x)};
}
__device__ __forceinline__ cplx cadd(const cplx &a, const cplx &b) { return cplx{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cplx csub(const cplx &a, const cplx &b) { return cplx{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cplx cconj(const cplx &a) { return cplx{a.x, -a.y}; }
__device__ __forceinline__ cplx mul_neg_i(const cplx &a) { return cplx{a.y, -a.x}; }      // a * (-i)

// exp(i * (q * pi/2 + frac * pi/2)), |frac| <= 1/2: the polynomials on |angle| <= pi/4, then the quarter turns
__device__ __forceinline__ cplx cis_quarters(int q, double frac) {
    const double a = frac * kHalfPi;
    const double s = pgx::pgx_sin_poly(a), c = pgx::pgx_cos_poly(a);
    switch (q & 3) {
        case 0: return cplx{c, s};
        case 1: return cplx{-s, c};
        case 2: return cplx{-c, -s};
        default: return cplx{s, -c};
    }
}

// W = exp(-2*pi*i * p / 2^l), 0 <= p < 2^l: p = q * 2^l/4 + rem/4 with |rem| <= 2^l/2 in integers, rem / 2^l exact
__device__ __forceinline__ cplx root_pow2(int64_t p, int l) {
    const int64_t den = (int64_t)1 << l;
    const int64_t q = (8 * p + den) >> (l + 1);
    const int64_t rem = 4 * p - q * den;
    const double inv_den = __hiloint2double((1023 - l) << 20, 0);       // 2^-l
    return cconj(cis_quarters((int)q, (double)rem * inv_den));
}

// b_k = exp(i*pi*k^2/N) = exp(2*pi*i * (k^2 mod 2N) / 2N), k < 2^21: k^2 < 2^42 stays an integer throughout
__device__ __forceinline__ cplx chirp_at(int64_t k, int64_t n) {
    const int64_t den = 2 * n;
    const int64_t num = (k * k) % den;
    const int64_t q = (8 * num + den) / (2 * den);
    const int64_t rem = 4 * num - q * den;
    return cis_quarters((int)q, (double)rem / (double)den);
}

// In-place FFT of the tile's 2^(11-l) sequences (sequence s at img[s << l], natural order in and out), forward sign.
// tw[p] = W_L^p.  The tile must be visible on entry; it is visible to every thread on return.
__device__ __forceinline__ void tile_fft(cplx *img, const cplx *tw, int l) {
    const int tid = threadIdx.x;
    for (int lns = 0; lns < l;) {
        const int Ns = 1 << lns;
        if (l - lns >= 2) {
            constexpr int U = kTile / 4 / kBlock;
            const int lq = l - 2, q = 1 << lq, sh = l - 2 - lns;
            cplx r[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = tid + u * kBlock;
                const int s = w >> lq, j = w & (q - 1), k = j & (Ns - 1);
                const cplx *bi = img + (s << l);
                const cplx x0 = bi[j];
                const cplx c1 = cmul(bi[j + q], tw[k << sh]);
                const cplx c2 = cmul(bi[j + 2 * q], tw[(2 * k) << sh]);
                const cplx c3 = cmul(bi[j + 3 * q], tw[(3 * k) << sh]);
                const cplx s0 = cadd(x0, c2), s1 = csub(x0, c2), s2 = cadd(c1, c3), s3 = mul_neg_i(csub(c1, c3));
                r[u][0] = cadd(s0, s2);
                r[u][1] = cadd(s1, s3);
                r[u][2] = csub(s0, s2);
                r[u][3] = csub(s1, s3);
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = tid + u * kBlock;
                const int s = w >> lq, j = w & (q - 1), k = j & (Ns - 1);
                cplx *bo = img + (s << l) + (j - k) * 4 + k;
                bo[0] = r[u][0];
                bo[Ns] = r[u][1];
                bo[2 * Ns] = r[u][2];
                bo[3 * Ns] = r[u][3];
            }
            lns += 2;
        } else {                                               // the last stage of an odd l: Ns = L/2, k = j
            constexpr int U = kTile / 2 / kBlock;
            const int lq = l - 1, q = 1 << lq;
            cplx r[U][2];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = tid + u * kBlock;
                const int s = w >> lq, j = w & (q - 1);
                const cplx *bi = img + (s << l);
                const cplx x0 = bi[j];
                const cplx c1 = cmul(bi[j + q], tw[j]);
                r[u][0] = cadd(x0, c1);
                r[u][1] = csub(x0, c1);
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = tid + u * kBlock;
                const int s = w >> lq, j = w & (q - 1);
                cplx *bo = img + (s << l);
                bo[j] = r[u][0];
                bo[j + q] = r[u][1];
            }
            lns += 1;
        }
        __syncthreads();
    }
}

// One pass: `nseq` sequences of length 2^l per batch item (blockIdx.y); element i of sequence s is read from
// in[y*in_batch + s*in_ss + i*in_es] and result k goes to out[y*out_batch + s*out_ss + k*out_es].  Of (ss, es) one is 1:
// the lanes of a wave run along that index.
struct FftPass {
    const cplx *in;
    cplx *out;
    const cplx *mul;                  // optional: the result at offset o (without the batch part) times mul[o & mul_mask]
    int64_t nseq, in_ss, in_es, out_ss, out_es, in_batch, out_batch, mul_mask;
    double scale;
    int l;
    int tw_lm;                        // > 0: result k of sequence s times W_(2^tw_lm)^(s*k) (the four-step twiddle)
    int conj_in, conj_out;
};

__global__ __launch_bounds__(kBlock) void k_fft_pass(FftPass p) {
    __shared__ cplx img[kTile];
    __shared__ cplx tw[kTile];
    const int tid = threadIdx.x, l = p.l, lw = kTileLog2 - l, L = 1 << l, W = 1 << lw;
    const int64_t s0 = (int64_t)blockIdx.x << lw;
    const cplx *src = p.in + (int64_t)blockIdx.y * p.in_batch;
    cplx *dst = p.out + (int64_t)blockIdx.y * p.out_batch;
    cplx v[kPerThread];
    const bool in_rows = p.in_es == 1;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {                     // all loads first: one memory latency, not eight
        const int e = tid + u * kBlock;
        const int s = in_rows ? e >> l : e & (W - 1), i = in_rows ? e & (L - 1) : e >> lw;
        const bool ok = s0 + s < p.nseq;
        v[u] = src[ok ? (s0 + s) * p.in_ss + (int64_t)i * p.in_es : 0];
        if (!ok) v[u] = cplx{0.0, 0.0};
    }
    for (int e = tid; e < L; e += kBlock) tw[e] = root_pow2(e, l);
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int e = tid + u * kBlock;
        const int s = in_rows ? e >> l : e & (W - 1), i = in_rows ? e & (L - 1) : e >> lw;
        img[(s << l) + i] = p.conj_in ? cconj(v[u]) : v[u];
    }
    __syncthreads();
    tile_fft(img, tw, l);
    const bool out_rows = p.out_es == 1;
    const int64_t tw_mask = ((int64_t)1 << p.tw_lm) - 1;
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int e = tid + u * kBlock;
        const int s = out_rows ? e >> l : e & (W - 1), k = out_rows ? e & (L - 1) : e >> lw;
        if (s0 + s >= p.nseq) continue;
        cplx r = img[(s << l) + k];
        if (p.tw_lm > 0) r = cmul(r, root_pow2(((s0 + s) * k) & tw_mask, p.tw_lm));
        const int64_t o = (s0 + s) * p.out_ss + (int64_t)k * p.out_es;
        if (p.mul) r = cmul(r, p.mul[o & p.mul_mask]);
        if (p.conj_out) r = cconj(r);
        dst[o] = cplx{r.x * p.scale, r.y * p.scale};
    }
}

// chirp[k] = b_k, k < n;  wrapped[j] = b_j (j < n), b_(M-j) (j > M - n), 0 between: the length-M kernel of the convolution
__global__ __launch_bounds__(kBlock) void k_chirp(cplx *chirp, cplx *wrapped, int64_t n, int64_t M) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < M; j += stride) {
        const int64_t k = j < n ? j : M - j;
        cplx b{0.0, 0.0};
        if (k < n) b = chirp_at(k, n);
        wrapped[j] = b;
        if (j < n) chirp[j] = b;
    }
}

// a[y][k] = x[y][k] . conj(b_k), k < n; 0 up to M
__global__ __launch_bounds__(kBlock) void k_bluestein_pre(cplx *a, const cplx *x, const cplx *chirp, int64_t n, int64_t M,
                                                          int conj_in) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const cplx *xs = x + (int64_t)blockIdx.y * n;
    cplx *as = a + (int64_t)blockIdx.y * M;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < M; k += stride) {
        cplx r{0.0, 0.0};
        if (k < n) {
            const cplx v = xs[k];
            r = cmul(conj_in ? cconj(v) : v, cconj(chirp[k]));
        }
        as[k] = r;
    }
}

// out[y][k] = conj(b_k) . a[y][k] . scale, k < n
__global__ __launch_bounds__(kBlock) void k_bluestein_post(cplx *out, const cplx *a, const cplx *chirp, int64_t n, int64_t M,
                                                           double scale, int conj_out) {
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const cplx *as = a + (int64_t)blockIdx.y * M;
    cplx *os = out + (int64_t)blockIdx.y * n;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += stride) {
        cplx r = cmul(as[k], cconj(chirp[k]));
        if (conj_out) r = cconj(r);
        os[k] = cplx{r.x * scale, r.y * scale};
    }
}

// float32 (n, C) interleaved -> C complex sequences
__global__ __launch_bounds__(kBlock) void k_tralfam_load(cplx *z, const float *x, int64_t n, int channels) {
    const int64_t total = n * channels, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < total; f += stride) {
        const int64_t k = f / channels;
        const int c = (int)(f - k * channels);
        z[(int64_t)c * n + k] = cplx{(double)x[f], 0.0};
    }
}

// z[c][k] <- |z[c][k]| . exp(i*phi), phi = (u * 2.0) * pi, u = (raw >> 11) * 2^-53 of draw k*C + c (tralfam_pe.py:93-97).
// A lane owns kDrawRun consecutive draws: one skip-ahead, then one LCG step per draw.
__global__ __launch_bounds__(kBlock) void k_tralfam_phase(cplx *z, int64_t n, int channels, const pgx_noise_params *rng,
                                                          const pgx::SkipTable *skip) {
    const int64_t total = n * channels, stride = (int64_t)gridDim.x * kBlock * kDrawRun;
    const pgx_noise_params p = rng[0];
    const pgx::u128 inc = pgx::make128(p.inc_hi, p.inc_lo);
    for (int64_t f0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kDrawRun; f0 < total; f0 += stride) {
        // the state BEFORE draw f0: draw f comes from the state after consumed + f + 1 steps
        pgx::u128 s = pgx::pcg_skip_with(*skip, pgx::make128(p.state_hi, p.state_lo), inc,
                                         (uint64_t)p.consumed + (uint64_t)f0);
#pragma unroll
        for (int j = 0; j < kDrawRun; ++j) {
            s = s * pgx::kPcgMult + inc;
            const int64_t f = f0 + j;
            if (f >= total) break;
            const double u = (double)(pgx::pcg_output(s) >> 11) * 0x1p-53;
            const double phi = (u * 2.0) * 3.141592653589793;
            double sn, cs;
            pgx::pgx_sincos_bounded(phi, sn, cs);
            const int64_t k = f / channels;
            const int c = (int)(f - k * channels);
            cplx *at = z + (int64_t)c * n + k;
            const cplx v = *at;
            const double mag = sqrt(__builtin_fma(v.x, v.x, v.y * v.y));
            *at = cplx{mag * cs, mag * sn};
        }
    }
}

// out[k][c] = float32(Re z[c][k]); *peak_bits = max |out| (a non-negative float orders like its bit pattern)
__global__ __launch_bounds__(kBlock) void k_tralfam_store(float *out, const cplx *z, int64_t n, int channels,
                                                          unsigned *peak_bits) {
    const int64_t total = n * channels, stride = (int64_t)gridDim.x * kBlock;
    unsigned top = 0;
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < total; f += stride) {
        const int64_t k = f / channels;
        const int c = (int)(f - k * channels);
        const float y = (float)z[(int64_t)c * n + k].x;
        out[f] = y;
        const unsigned bits = __float_as_uint(fabsf(y));
        top = bits > top ? bits : top;
    }
    if (!peak_bits) return;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)top, d, 64);
        top = o > top ? o : top;
    }
    if ((threadIdx.x & 63) == 0 && top != 0) atomicMax(peak_bits, top);
}

// out *= float32(normalize_peak) / peak, a float32 division and a float32 product; nothing for peak == 0 (or NaN)
__global__ __launch_bounds__(kBlock) void k_tralfam_scale(float *out, int64_t total, float normalize_peak,
                                                          const unsigned *peak_bits) {
    const float peak = __uint_as_float(*peak_bits);
    if (!(peak > 0.0f)) return;
    const float g = normalize_peak / peak;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x; f < total; f += stride) out[f] = out[f] * g;
}

// ---------------------------------------------------------------------------------------------------------- host side

inline bool is_pow2(int64_t n) { return (n & (n - 1)) == 0; }
inline int log2_ceil(int64_t n) {
    int m = 0;
    while (((int64_t)1 << m) < n) ++m;
    return m;
}
// log2 of the power-of-two transform behind length n: n itself, or Bluestein's M >= 2n - 1
inline int fft_log2(int64_t n) { return is_pow2(n) ? log2_ceil(n) : log2_ceil(2 * n - 1); }
inline bool two_pass(int m) { return m > kTileLog2; }
inline bool length_ok(int64_t n) { return n >= 1 && n <= kMaxLength; }

// Forward FFT of `batch` sequences of 2^m points, `seq_stride` apart in both buffers (in == out allowed), result times
// `scale`; `inverse`: conj -> forward -> conj.  `tmp`: batch * 2^m points when two_pass(m).
int fft_pow2(cplx *out, const cplx *in, int m, int64_t batch, bool inverse, double scale, const cplx *mul, cplx *tmp) {
    const int64_t M = (int64_t)1 << m;
    hipStream_t st = pgx::stream();
    FftPass p{};
    p.mul_mask = M - 1;
    if (!two_pass(m)) {
        const int64_t per_tile = kTile >> m;
        p.in = in; p.out = out; p.mul = mul;
        p.nseq = batch; p.in_ss = M; p.in_es = 1; p.out_ss = M; p.out_es = 1;
        p.scale = scale; p.l = m; p.conj_in = inverse; p.conj_out = inverse;
        hipLaunchKernelGGL(k_fft_pass, dim3((unsigned)pgx::ceil_div(batch, per_tile)), dim3(kBlock), 0, st, p);
        PGX_LAUNCH_CHECK("k_fft_pass");
        return PGX_OK;
    }
    const int l1 = m / 2, l2 = m - l1;
    const int64_t N1 = (int64_t)1 << l1, N2 = (int64_t)1 << l2;
    p.in = in; p.out = tmp;
    p.nseq = N2; p.in_ss = 1; p.in_es = N2; p.out_ss = 1; p.out_es = N2; p.in_batch = M; p.out_batch = M;
    p.scale = 1.0; p.l = l1; p.tw_lm = m; p.conj_in = inverse;
    hipLaunchKernelGGL(k_fft_pass, dim3((unsigned)(N2 >> (kTileLog2 - l1)), (unsigned)batch), dim3(kBlock), 0, st, p);
    PGX_LAUNCH_CHECK("k_fft_pass<columns>");
    p = FftPass{};
    p.mul_mask = M - 1;
    p.in = tmp; p.out = out; p.mul = mul;
    p.nseq = N1; p.in_ss = N2; p.in_es = 1; p.out_ss = 1; p.out_es = N1; p.in_batch = M; p.out_batch = M;
    p.scale = scale; p.l = l2; p.conj_out = inverse;
    hipLaunchKernelGGL(k_fft_pass, dim3((unsigned)pgx::ceil_div(N1, (int64_t)1 << (kTileLog2 - l2)), (unsigned)batch),
                       dim3(kBlock), 0, st, p);
    PGX_LAUNCH_CHECK("k_fft_pass<rows>");
    return PGX_OK;
}

// plan of a length that is not a power of two: chirp[n] | chirp spectrum[M] | scratch[M when two_pass]
struct Plan {
    cplx *chirp, *spectrum, *scratch;
};
inline Plan plan_of(void *plan, int64_t n, int64_t M) {
    cplx *base = (cplx *)plan;
    return Plan{base, base + n, base + n + M};
}
inline size_t plan_bytes(int64_t n) {
    if (is_pow2(n)) return sizeof(cplx);
    const int m = fft_log2(n);
    const int64_t M = (int64_t)1 << m;
    return (size_t)(n + M + (two_pass(m) ? M : 0)) * sizeof(cplx);
}
// scratch of one DFT behind the head: Bluestein's padded sequences, then the column pass's output
inline size_t dft_scratch_bytes(int64_t n, int64_t batch) {
    const int m = fft_log2(n);
    const int64_t M = (int64_t)1 << m;
    const int64_t images = (is_pow2(n) ? 0 : 1) + (two_pass(m) ? 1 : 0);
    return (size_t)images * batch * M * sizeof(cplx);
}

// DFT of `batch` sequences of n points, n apart (in == out allowed); inverse scaled 1/n.  `scratch`: dft_scratch_bytes.
int dft_run(cplx *out, const cplx *in, int64_t n, int64_t batch, bool inverse, const void *plan, void *scratch) {
    const int m = fft_log2(n);
    const int64_t M = (int64_t)1 << m;
    if (is_pow2(n)) return fft_pow2(out, in, m, batch, inverse, inverse ? 1.0 / (double)n : 1.0, nullptr, (cplx *)scratch);
    hipStream_t st = pgx::stream();
    const Plan pl = plan_of(const_cast<void *>(plan), n, M);
    cplx *a = (cplx *)scratch, *tmp = a + batch * M;
    const dim3 grid_m((unsigned)pgx::grid_for(M, kBlock), (unsigned)batch), grid_n((unsigned)pgx::grid_for(n, kBlock), (unsigned)batch);
    hipLaunchKernelGGL(k_bluestein_pre, grid_m, dim3(kBlock), 0, st, a, in, (const cplx *)pl.chirp, n, M, inverse ? 1 : 0);
    PGX_LAUNCH_CHECK("k_bluestein_pre");
    if (int rc = fft_pow2(a, a, m, batch, false, 1.0, pl.spectrum, tmp)) return rc;
    if (int rc = fft_pow2(a, a, m, batch, true, 1.0, nullptr, tmp)) return rc;
    const double scale = (1.0 / (double)M) * (inverse ? 1.0 / (double)n : 1.0);
    hipLaunchKernelGGL(k_bluestein_post, grid_n, dim3(kBlock), 0, st, out, (const cplx *)a, (const cplx *)pl.chirp, n, M,
                       scale, inverse ? 1 : 0);
    PGX_LAUNCH_CHECK("k_bluestein_post");
    return PGX_OK;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int64_t pgx_dft_max_length(void) { return kMaxLength; }

size_t pgx_dft_plan_bytes(int64_t n) { return length_ok(n) ? plan_bytes(n) : 0; }

size_t pgx_dft_workspace_bytes(int64_t n, int batch) {
    if (!length_ok(n) || batch < 1 || batch > 65535) return 0;
    return kHeadBytes + dft_scratch_bytes(n, batch);
}

size_t pgx_tralfam_workspace_bytes(int64_t n, int channels) {
    if (!length_ok(n) || channels < 1 || channels > 65535) return 0;
    return kHeadBytes + align256((size_t)n * channels * sizeof(cplx)) + dft_scratch_bytes(n, channels);
}

int pgx_dft_plan(void *plan, int64_t n) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(n >= 1, "pgx_dft_plan: n must be >= 1");
    PGX_CHECK_ARG(n <= kMaxLength, "pgx_dft_plan: n exceeds the maximum length of 2097152 (2^21) points");
    PGX_CHECK_ARG(plan, "pgx_dft_plan: null plan");
    if (is_pow2(n)) return PGX_OK;
    const int m = fft_log2(n);
    const int64_t M = (int64_t)1 << m;
    const Plan pl = plan_of(plan, n, M);
    hipLaunchKernelGGL(k_chirp, dim3((unsigned)pgx::grid_for(M, kBlock)), dim3(kBlock), 0, pgx::stream(), pl.chirp,
                       pl.spectrum, n, M);
    PGX_LAUNCH_CHECK("k_chirp");
    return fft_pow2(pl.spectrum, pl.spectrum, m, 1, false, 1.0, nullptr, pl.scratch);
}

int pgx_dft_c2c(void *out, const void *in, int64_t n, int batch, int inverse, const void *plan, void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || batch <= 0) return PGX_OK;
    PGX_CHECK_ARG(n <= kMaxLength, "pgx_dft_c2c: n exceeds the maximum length of 2097152 (2^21) points");
    PGX_CHECK_ARG(out && in && plan && workspace && batch <= 65535, "pgx_dft_c2c: bad argument");
    return dft_run((cplx *)out, (const cplx *)in, n, batch, inverse != 0, plan, (char *)workspace + kHeadBytes);
}

int pgx_tralfam(float *out, const float *x, int64_t n, int channels, const pgx_noise_params *rng, double normalize_peak,
                const void *plan, void *workspace) {
    PGX_REQUIRE_INIT();
    if (n <= 0 || channels <= 0) return PGX_OK;
    PGX_CHECK_ARG(n <= kMaxLength, "pgx_tralfam: n exceeds the maximum length of 2097152 (2^21) frames");
    PGX_CHECK_ARG(out && x && rng && plan && workspace && channels <= 65535, "pgx_tralfam: bad argument");
    const pgx::SkipTable *skip = pgx::pcg_skip_table_device();
    if (!skip) return PGX_ERR_RUNTIME;
    hipStream_t st = pgx::stream();
    unsigned *peak = (unsigned *)workspace;
    cplx *z = (cplx *)((char *)workspace + kHeadBytes);
    void *scratch = (char *)z + align256((size_t)n * channels * sizeof(cplx));
    const int64_t total = n * channels;
    const dim3 grid((unsigned)pgx::grid_for(total, kBlock));
    const bool normalize = normalize_peak > 0.0;
    if (normalize) PGX_HIP(hipMemsetAsync(peak, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_tralfam_load, grid, dim3(kBlock), 0, st, z, x, n, channels);
    PGX_LAUNCH_CHECK("k_tralfam_load");
    if (int rc = dft_run(z, z, n, channels, false, plan, scratch)) return rc;
    hipLaunchKernelGGL(k_tralfam_phase, dim3((unsigned)pgx::grid_for(pgx::ceil_div(total, kDrawRun), kBlock)), dim3(kBlock),
                       0, st, z, n, channels, rng, skip);
    PGX_LAUNCH_CHECK("k_tralfam_phase");
    if (int rc = dft_run(z, z, n, channels, true, plan, scratch)) return rc;
    hipLaunchKernelGGL(k_tralfam_store, grid, dim3(kBlock), 0, st, out, (const cplx *)z, n, channels,
                       normalize ? peak : (unsigned *)nullptr);
    PGX_LAUNCH_CHECK("k_tralfam_store");
    if (normalize) {
        hipLaunchKernelGGL(k_tralfam_scale, grid, dim3(kBlock), 0, st, out, total, (float)normalize_peak,
                           (const unsigned *)peak);
        PGX_LAUNCH_CHECK("k_tralfam_scale");
    }
    return PGX_OK;
}

}  // extern "C"
