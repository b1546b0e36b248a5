/*
 * pygmu_hip.h -- C ABI of libpygmu_hip.so, the MI355X (gfx950) render library behind
 * pygmu2's `ProcessingElement._render(start, duration) -> Snippet` hot path.
 *
 * The reference (rdpoor/pygmu2) is pure Python/numpy: it has no FFI.  The drop-in
 * boundary is therefore the body of each PE's `_render`; every entry
 * point below replaces the numpy/scipy/numba arithmetic of one reference function,
 * cited as `file:line` relative to /root/reference/src/pygmu2/.  The Python binding a
 * maintainer would add is shown in INTEGRATION.md (ctypes; pygmu2_amd/device.py is
 * that binding for this repository's own PE classes).
 *
 * Conventions
 *  - Plain C types only.  `float*` / `double*` / `void*` arguments are DEVICE pointers
 *    obtained from pgx_malloc unless the name ends in `_host`.
 *  - Audio buffers are (frames, channels) row-major float32, exactly the reference's
 *    Snippet payload (snippet.py:37-45).  Batched entry points take `batch` independent
 *    instances ("voices"); instance i's buffer starts `*_stride` ELEMENTS after
 *    instance i-1's, its parameter block is params[i], its state is state[i].
 *  - Parameter blocks and state blobs live in device memory and are owned by the caller
 *    (the PE object).  A zero-filled state blob is the reset state unless noted.
 *  - Every call is asynchronous on the library stream (pgx_stream_handle) unless
 *    documented as synchronous.  No entry point allocates or synchronises unless noted,
 *    so sequences of calls can be captured into a HIP graph.
 *  - Return value: 0 on success, negative pgx_status otherwise; the message of the last
 *    failure on the calling thread is available from pgx_last_error().  No C++
 *    exception crosses this boundary.
 */
#ifndef PYGMU_HIP_H
#define PYGMU_HIP_H

#include <stddef.h>
#include <stdint.h>

/* PGX_HOST marks a pointer parameter that the call itself dereferences on the host. */
#define PGX_HOST

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    PGX_OK = 0,
    PGX_ERR_INVALID = -1,   /* bad argument (maps to Python ValueError)            */
    PGX_ERR_RUNTIME = -2,   /* HIP runtime failure (maps to Python RuntimeError)   */
    PGX_ERR_NOT_INIT = -3,  /* pgx_init not called / no device                      */
    PGX_ERR_NOMEM = -4
} pgx_status;

/* ------------------------------------------------------------------ runtime */
int pgx_abi_version(void);
const char *pgx_last_error(void);
int pgx_device_count(PGX_HOST int *count);
int pgx_init(int device);                 /* select device, create stream + pool; idempotent */
int pgx_shutdown(void);                   /* sync, release pool, destroy stream              */
int pgx_device_name(PGX_HOST char *buf, size_t len);
void *pgx_stream_handle(void);            /* hipStream_t of the library stream               */
int pgx_stream_sync(void);
/* Two independent sub-graphs of one block may overlap on the device:
 *   pgx_stream_fork()      a side stream starts behind everything enqueued so far; calls go to it
 *   pgx_stream_select(s)   while forked: s != 0 -> side stream, 0 -> main stream
 *   pgx_stream_join()      main stream waits for the side stream; calls go to the main stream again
 * Between fork and join pgx_free() parks blocks (they are re-pooled at the join): "freed = reusable"
 * is only true in single-stream order.  The caller keeps the two call sequences data-independent. */
int pgx_stream_fork(void);
int pgx_stream_select(int side);
int pgx_stream_join(void);
int pgx_stream_is_forked(void);           /* 1 between fork and join */
/* A fork whose side work the main stream does not need yet (the next block's envelopes, rendered one block ahead):
 *   pgx_stream_detach()         ends the fork without waiting: the side stream keeps running what it was given, calls go
 *                               to the main stream again; blocks freed during the fork stay parked
 *   pgx_stream_wait_detached()  the main stream waits for that work (no-op when nothing is detached)
 * A new fork waits for detached work first (there is one side stream); pgx_stream_sync covers it. */
int pgx_stream_detach(void);
/* pgx_stream_fork_after(event): a fork whose side stream starts behind `event` -- recorded earlier on the main stream
 * with pgx_event_record -- instead of behind the main stream's current tail (NULL: behind nothing).  For side work that
 * depends on nothing the main stream is doing and writes only buffers whose last main-stream reader the event covers. */
int pgx_stream_fork_after(void *event);
int pgx_stream_wait_detached(void);
int pgx_stream_is_detached(void);

int pgx_malloc(PGX_HOST void **dptr, size_t bytes);      /* pooled (size-class free lists)           */
int pgx_free(void *dptr);                       /* returns the block to the pool            */
int pgx_pool_trim(void);                        /* hipFree every cached block               */
int pgx_memset(void *dptr, int byte_value, size_t bytes);
int pgx_memcpy_h2d(void *dst, const void *src_host, size_t bytes);  /* synchronous */
int pgx_memcpy_d2h(void *dst_host, const void *src, size_t bytes);  /* synchronous */
int pgx_memcpy_d2d(void *dst, const void *src, size_t bytes);

/* Root Snippets leaving the device (the caller of render() reads `.data`: benchmark_pes.py:176-185 hands host
 * arrays to its caller).  Pinned host blocks are pooled like device blocks.
 *   pgx_d2h_begin   asynchronous copy on the library's copy stream, ordered behind everything enqueued on
 *                   the library stream so far -- the next block renders while this one crosses PCIe
 *   pgx_d2h_wait    the host blocks until that copy has landed
 *   pgx_d2h_fence   the library stream waits for it instead (before `src` is recycled unread) */
int pgx_host_malloc(PGX_HOST void **hptr, size_t bytes);
int pgx_host_free(void *hptr);
int pgx_d2h_begin(void *dst_host, const void *src, size_t bytes, PGX_HOST int64_t *ticket);
int pgx_d2h_wait(int64_t ticket);
int pgx_d2h_query(int64_t ticket, PGX_HOST int *done);   /* *done = 1 once that copy has landed; never blocks */
int pgx_d2h_fence(int64_t ticket);

int pgx_event_create(PGX_HOST void **event);
int pgx_event_destroy(void *event);
int pgx_event_record(void *event);              /* on the library stream */
int pgx_event_elapsed_ms(void *start, void *stop, PGX_HOST float *ms);   /* synchronises on stop */

/* Diagnostics: evaluate the library's float64 sine / cosine (the routine every oscillator and
 * coefficient kernel uses in place of np.sin / np.cos) on n device doubles. */
int pgx_selftest_sincos(double *out_sin, double *out_cos, const double *x, int64_t n);
/* the library's own float64 tanh (LadderPE's feedback nonlinearity), for the accuracy test */
int pgx_selftest_tanh(double *out, const double *x, int64_t n);

/* ------------------------------------------------------------------ sources / copies
 * ConstantPE._render (constant_pe.py:51-63), IdentityPE._render (identity_pe.py:43-60),
 * DiracPE._render (dirac_pe.py:48-67), ArrayPE._render (array_pe.py:74-129) and the
 * copy/hold part of _ExtentWindowPE._render (extent_window_pe.py:88-157).  Bit-exact.
 */
int pgx_fill(float *out, int64_t n_elems, float value);
/* IdentityPE: out[i, :] = first + float(i) * delta in float32, where the host passes
 * first = float32(start), delta = float32(start + 1) - first (numpy's arange fill rule). */
int pgx_ramp(float *out, float first, float delta, int64_t n, int channels);
/* IdentityPE over a window of consecutive blocks of `period` frames (n frames from `start`): every block is the
 * reference's np.arange(block start, ..., dtype=float32) -- first and delta taken at the block's own start, which is
 * what the fill depends on beyond 2^24 (identity_pe.py:54). */
int pgx_ramp_blocks(float *out, int64_t start, int64_t n, int channels, int64_t period);
int pgx_dirac(float *out, int64_t start, int64_t n, int channels);
/* out[f, :] = src[start + f - src_start, :] where start+f lies in [src_start, src_start+src_len),
 * else src[0] if (before && hold_first), src[src_len-1] if (after && hold_last), else 0. */
int pgx_window_copy(float *out, int64_t start, int64_t n, int channels,
                    const float *src, int64_t src_start, int64_t src_len,
                    int hold_first, int hold_last);

/* out[f] = in[f, ch]: channel selection of a control stream, as _scalar_or_pe_values does
 * for a multi-channel parameter PE (processing_element.py:346-352). */
int pgx_extract_channel(float *out, const float *in, int64_t n, int channels, int ch);

/* ------------------------------------------------------------------ SinePE
 * Pure path: SinePE._render + _compute_phase_pure (sine_pe.py:119-175).
 *   phase = phase0 + w * (double(n) / sr),  out = float(amp * sin(phase)),  w = (2*pi)*f
 *   computed on the host exactly as the reference does.  float64 throughout.
 */
typedef struct {
    double w;        /* (2.0 * pi) * frequency */
    double amp;
    double phase0;
} pgx_sine_params;
int pgx_sine_render(float *out, int64_t out_stride, int batch, int64_t start, int64_t n,
                    int channels, double sample_rate, const pgx_sine_params *params);
/* GainPE(SinePE(scalars), gain=<scalar>) in one launch: float32(float32(amp*sin) * float32 gain),
 * the same two roundings as pgx_sine_render followed by pgx_gain_const (gain_pe.py:121-123). */
int pgx_sine_gain_render(float *out, int64_t out_stride, int batch, int64_t start, int64_t n,
                         int channels, double sample_rate, const pgx_sine_params *params, float gain);

/* Stateful path: _compute_phase_stateful (sine_pe.py:177-232).  freq/amp/phase_mod are
 * optional per-sample float32 control streams (frames, 1); NULL -> the scalar in params.
 * state[instance] = { accumulated_phase, initialised flag }.  The phase term is added to
 * every sample and is included in the carried phase, as in the reference. */
typedef struct {
    double freq;
    double amp;
    double phase;          /* scalar phase (used as initial phase and as per-sample term) */
    int32_t phase_is_stream;
    int32_t pad;
} pgx_sine_stateful_params;
int pgx_sine_stateful(float *out, int64_t n, int channels, double sample_rate,
                      const pgx_sine_stateful_params *params,
                      const float *freq, const float *amp, const float *phase_mod,
                      double *state /* [2] */);

/* A bank of stateful sines (voice_bank.py: FM / AM / PM voices).  Voice v writes n * channels float32 at out + v *
 * out_stride, reads params[v] and its (n, 1) streams at freq + v * freq_stride, amp + v * amp_stride, phase_mod + v *
 * phase_stride (NULL: the scalar of params[v], as above), and carries state[v] = { accumulated_phase, initialised flag }.
 * workspace: pgx_sine_stateful_bank_workspace_bytes(n, batch) bytes, or NULL.  Without one, or for blocks of one or two
 * tiles of 2 048 frames (or more than 2^22), one workgroup per voice walks its row in ONE launch; with one, a workgroup per
 * tile and voice in two launches (the tiles' totals; their left fold in tile order and the frames).  Either way row v holds the float32
 * samples and state[v] the final { phase, 1.0 } that pgx_sine_stateful(row v, params[v], voice v's streams, state[v]) gives,
 * bit for bit.
 * n <= 0 or batch <= 0: PGX_OK, nothing launched.  batch > 65535, channels < 1, sample_rate <= 0, a stride below its row,
 * a null out / params / state: PGX_ERR_INVALID, nothing launched. */
size_t pgx_sine_stateful_bank_workspace_bytes(int64_t n, int batch);
int pgx_sine_stateful_bank(float *out, int64_t out_stride, int batch, int64_t n, int channels, double sample_rate,
                           const pgx_sine_stateful_params *params /* device [batch] */,
                           const float *freq, int64_t freq_stride, const float *amp, int64_t amp_stride,
                           const float *phase_mod, int64_t phase_stride,
                           double *state /* [batch][2] */, void *workspace /* or NULL */);

/* ------------------------------------------------------------------ GainPE / MixPE
 * GainPE._render (gain_pe.py:92-127): one float32 multiply -> bit-exact.
 * MixPE._render (mix_pe.py:91-94): float32 adds in input order -> bit-exact. */
int pgx_gain_const(float *out, const float *in, int64_t n_elems, float gain);
int pgx_gain_vec(float *out, const float *in, const float *gain, int64_t n, int channels,
                 int gain_channels /* 1 (broadcast) or == channels */);
/* ins_host: HOST array of k device pointers, each n_elems floats. */
int pgx_mix_n(float *out, PGX_HOST const float *const *ins_host, int k, int64_t n_elems);
/* Sum of `batch` equally shaped voices stored [batch][n_elems] (stride in elements),
 * accumulated in float32 in voice order 0..batch-1 (== MixPE over the voices). */
int pgx_mix_batch(float *out, const float *in, int64_t in_stride, int batch, int64_t n_elems);
/* MixPE over voices that each end in GainPE(voice, gain=<PE>): out = sum_b float32(in_b * gain_b),
 * products rounded to float32, added in voice order -- identical to pgx_gain_vec + pgx_mix_batch. */
int pgx_gain_mix_batch(float *out, const float *in, int64_t in_stride, const float *gain,
                       int64_t gain_stride, int batch, int64_t n, int channels, int gain_channels);

/* ------------------------------------------------------------------ BiquadPE
 * Constant coefficients: BiquadPE._filter_constant_coeffs (biquad_pe.py:383-404), i.e.
 * scipy.signal.lfilter's direct-form-II-transposed section in float64:
 *     y = z0 + b0*x;  z0 = (z1 + b1*x) - a1*y;  z1 = b2*x - a2*y
 * evaluated by a parallel scan over affine state maps; each thread re-runs its chunk in
 * exactly this operation order from its scanned carry-in.
 * coef[instance] = {b0,b1,b2,a1,a2} (host computes them, biquad_pe.py:217-335);
 * state[instance][channel] = {z0,z1}.  workspace: device scratch of at least
 * pgx_biquad_workspace_bytes(batch, n, channels, settle_frames) bytes (may be NULL when that is 0).
 * settle_frames: 0, or a frame count W for which every entry of A^W (A = [[-a1,1],[-a2,0]], all
 * instances) is below 2^-90, evaluated by the host from the coefficients it computed.  With W > 0 a
 * long chain is rendered in one launch: each workgroup rebuilds its carry-in from the W frames before
 * its range, which is exact to far below one float64 ulp; W = 0 (or a W above 65536) uses the
 * reduce + apply launch pair, exact for any section.
 * tables: NULL, or [batch][pgx_biquad_table_doubles()] doubles filled once per coefficient set by
 * pgx_biquad_tables (the powers of A the scan uses); saves the single-launch path its prologue. */
size_t pgx_biquad_workspace_bytes(int batch, int64_t n, int channels, int64_t settle_frames);
size_t pgx_biquad_table_doubles(void);
int pgx_biquad_tables(double *tables, const double *coef /* [batch][5] */, int batch);
int pgx_biquad_const(float *out, int64_t out_stride, const float *in, int64_t in_stride,
                     int batch, int64_t n, int channels,
                     const double *coef /* [batch][5] */, const double *tables, int64_t settle_frames,
                     double *state /* [batch][channels][2] */, void *workspace);

/* BiquadPE(SinePE) with scalar parameters, mono (biquad_pe.py:383-404 over sine_pe.py:159-175): the sine is made
 * in registers inside the single-launch filter kernel, so the chain writes 4 B per frame and reads nothing.
 * w = (2 pi) f, amp, phase0 as in pgx_sine_params; start = first frame of the render.  Only where
 * pgx_biquad_sine_supported(n, settle_frames) (the settled single-launch plan applies) and the phase stays below
 * 2e9 rad; the caller renders the two PEs separately otherwise.  A thread's first frame is k_sine's sample bit for
 * bit, its next 15 are that (sin, cos) pair turned by w / sr: within the rounding noise of the reference's phase. */
int pgx_biquad_sine_supported(int64_t n, int64_t settle_frames);
int pgx_biquad_sine(float *out, int64_t start, int64_t n, double sample_rate, double w, double amp, double phase0,
                    const double *coef /* [5] */, const double *tables, int64_t settle_frames,
                    double *state /* [2] */,
                    double *state_backup /* [2] or NULL: receives the state on entry (a window's snapshot) */);
/* Blocks long enough that every wave of one resident round gets a run of at least min_chunks 1024-frame chunks are
 * rendered by the wave-run kernel (k_biquad_sine_runs), shorter ones by the single-launch filter kernel.  0 turns
 * the wave runs off (environment: PGX_SB_SINE_RUNS), a negative value restores the default.  Returns the previous
 * value.  pgx_biquad_sine_supported answers the same either way. */
int pgx_biquad_sine_set_runs(int min_chunks);
/* The wave-run plan pgx_biquad_sine would render a block of n frames by, in 1024-frame chunks: out = {run, head, tail,
 * warm, waves}.  Wave 0 renders the chunks [0, head) and the last `tail` ones, wave g >= 1 the `run` chunks from
 * head + (g - 1) * run, each after `warm` chunks of warm-up.  Returns 1, or 0 (out untouched) when the single-launch
 * filter kernel would render the block; follows pgx_biquad_sine_set_runs.  Needs pgx_init (the plan is sized by the
 * device's resident waves). */
int pgx_biquad_sine_runs_plan(int64_t n, int64_t settle_frames, PGX_HOST int out[5]);
/* Deadline pacing of the wave-run kernel: every wave sets its issue priority once per chunk by how far it is behind
 * the schedule the previous window's duration gives it (read on the device, no synchronisation), so that the waves of
 * a SIMD end together.  It changes no sample.  A window is paced only when the runs-launch before it had the same plan
 * and no other pgx_biquad_sine render lies between them: the first window of a stream, a window after a change of
 * size and a window after a seek's render run unpaced.  0 off, 1 on (environment: PGX_SB_SINE_PACING), a negative
 * value restores the default.  Returns the previous value. */
int pgx_biquad_sine_set_pacing(int mode);
/* What the last wave-run launch rendered with pacing on left on the device, after a synchronise of the library's
 * stream (done here): out = {its launch id, the longest duration among its recording waves (one in 61) in ticks of
 * 10 ns, the ticks per chunk (tau) it was given: 0 = it ran unpaced}; three zeros before the first such launch.  out is
 * host memory. */
int pgx_biquad_sine_pacing_info(int64_t out[3]);

/* The same chain over window-sized blocks in closed form (pgx_tone.hip): once the filter's transient has died the
 * output of a constant section driven by a pure tone is that tone scaled by |H(e^jw/sr)| and shifted by arg H, so
 * out[i] = float32(amp |H| sin(phase0 + arg H + w (start + i) / sr)) with no recurrence, no warm-up and no state
 * carried from lane to lane.  What the closed form leaves out is the filter's answer to the float32 rounding of the
 * input samples, at most 2^-25 sum|h| / |H| of the output's peak.
 * pgx_biquad_tone_supported: 1 when settle_frames > 0, n >= 2 settle_frames, |w| n / sr stays in the fast sine's
 * range and sum|h| / |H| <= 4 (h: the first settle_frames samples of the impulse response; H in long double) -- the
 * omitted rounding noise then stays below 1.2e-7 of the peak.  A host computation: no device is needed.
 * pgx_biquad_tone_gain / pgx_biquad_tone_l1: the |H| and the sum|h| that test uses.
 * pgx_biquad_tone: coefficients by value; tables, state and state_backup as for pgx_biquad_sine.  The carried state
 * enters as the zero-input response of (state - the steady solution's state at start - 1) over the first
 * settle_frames frames; state_backup (or NULL) receives the incoming state bit for bit; state leaves as the steady
 * solution's DF-II-T state at the last frame (x taken as the float32-rounded tone). */
int pgx_biquad_tone_supported(int64_t n, int64_t settle_frames, double w, double sample_rate, double b0, double b1,
                              double b2, double a1, double a2);
double pgx_biquad_tone_gain(double w, double sample_rate, double b0, double b1, double b2, double a1, double a2);
double pgx_biquad_tone_l1(int64_t settle_frames, double b0, double b1, double b2, double a1, double a2);
int pgx_biquad_tone(float *out, int64_t start, int64_t n, double sample_rate, double w, double amp, double phase0,
                    double b0, double b1, double b2, double a1, double a2, const double *tables,
                    int64_t settle_frames, double *state /* [2] */, double *state_backup /* [2] or NULL */);
/* The window kernel is bound by its stores, so the size of a stream's windows is its business: the frames per look-ahead
 * window at which the one live float32 mono window of a stream (its last block lives in a buffer of its own,
 * pgx_biquad_tone_window_split below, so the next window rewrites the same buffer) is still stored at the memory-side
 * cache's rate, not HBM's, and the host's cost of opening a window is spread over as many frames as that allows.
 * 0: no preference.
 * PGX_TONE_WINDOW_FRAMES replaces the built-in figure (read once).  A host computation: no device is needed. */
int64_t pgx_biquad_tone_window_frames(void);
/* A stream opens a window every few microseconds of host time: pgx_biquad_tone_plan evaluates once what
 * pgx_biquad_tone evaluates per call from its twelve chain constants (the gate, |H|, arg H, the rotation constants) and
 * returns a handle (NULL: pgx_biquad_tone_supported declines the chain at every block length), which the caller frees
 * with pgx_biquad_tone_plan_free; tables must outlive it.  pgx_biquad_tone_window(plan, ...) is pgx_biquad_tone with
 * those constants: the same launch, the same bits in out, state and state_backup. */
void *pgx_biquad_tone_plan(double sample_rate, double w, double amp, double phase0, double b0, double b1, double b2,
                           double a1, double a2, const double *tables, int64_t settle_frames);
int pgx_biquad_tone_plan_free(void *plan);
int pgx_biquad_tone_window(const void *plan, float *out, int64_t start, int64_t n, double *state /* [2] */,
                           double *state_backup /* [2] or NULL */);
/* A stream whose caller keeps the last block it pulled keeps that block's buffer alive.  pgx_biquad_tone_window_split
 * stores frames [0, n - tail_frames) to out and frames [n - tail_frames, n) to out_tail[0 ...]: with a window's last
 * block in a small buffer of its own the big one is free the moment the window is used up, and a stream rewrites one
 * resident buffer instead of two in turn.  Every frame is made by the same thread from the same anchor with the same
 * arithmetic as in pgx_biquad_tone_window: out | out_tail, state and state_backup hold the same bits.  tail_frames == 0
 * is pgx_biquad_tone_window; tail_frames == n leaves out untouched.  16-byte stores into the tail need out_tail on a
 * 16-byte boundary and n - tail_frames a multiple of 4 (else four 4-byte stores).  PGX_ERR_INVALID for tail_frames < 0,
 * tail_frames > n and tail_frames > 0 without out_tail.
 * pgx_biquad_tone_split_tail: 1 when streams should render their windows that way, 0 with PGX_TONE_SPLIT_TAIL=0 (read
 * once), which keeps the two alternating buffers.  A host computation: no device is needed. */
int pgx_biquad_tone_window_split(const void *plan, float *out, float *out_tail, int64_t tail_frames, int64_t start,
                                 int64_t n, double *state /* [2] */, double *state_backup /* [2] or NULL */);
int pgx_biquad_tone_split_tail(void);

/* Time-varying coefficients: _compute_coefficients per sample (biquad_pe.py:217-335) +
 * the direct-form-I recurrence of _biquad_varying_numba (biquad_pe.py:35-62).
 * freq/q: per-sample float32 control streams (frames,1) or NULL -> scalar.
 * state[channel] = {x1,x2,y1,y2}.  mode: 0 lowpass,1 highpass,2 bandpass,3 notch,
 * 4 allpass,5 peaking,6 lowshelf,7 highshelf. */
typedef struct {
    double freq;
    double q;
    double gain_db;
    int32_t mode;
    int32_t pad;
} pgx_biquad_var_params;
/* gain_a = 10^(gain_db/40) and gain_sqrt_a = sqrt(gain_a), computed by the host exactly as the
 * reference does (biquad_pe.py:250,290).
 * workspace: pgx_scan2_workspace_bytes(n, channels) bytes, or NULL.  With a workspace a long block is cut
 * into segments: a reduce launch composes each segment's affine state map, the apply launch folds the
 * earlier maps onto the carried state and renders (2 launches x up to 128 workgroups per channel);
 * without one (or for blocks of one or two tiles) a single workgroup walks the block. */
size_t pgx_scan2_workspace_bytes(int64_t n, int channels);
int pgx_biquad_varying(float *out, const float *in, int64_t n, int channels, double sample_rate,
                       const pgx_biquad_var_params *params, const float *freq, const float *q,
                       double gain_a, double gain_sqrt_a, double *state /* [channels][4] */,
                       void *workspace);
/* Bank of BiquadPEs with PE-driven frequency and / or Q (voice_bank.py): pgx_biquad_varying with the voice in the grid.
 * in / out: `batch` rows of n * channels float32, in_stride / out_stride elements apart (each >= n * channels);
 * freq / q: NULL (voice v takes params[v].freq / params[v].q) or `batch` rows of n float32, freq_stride / q_stride apart (>= n);
 * params: device [batch] (mode and the scalars are per voice);  gains: device [batch][2] = {A, sqrt(A)}, the two numbers the
 *         host passes pgx_biquad_varying by value, per voice;  state: [batch][channels][4];
 * workspace: batch * pgx_scan2_workspace_bytes(n, channels) bytes (voice v's slice starts at v times that), or NULL.
 * With a workspace every voice is rendered by pgx_biquad_varying's own plan (scan2_plan(n): the reduce and the apply launch,
 * grid (segments, channels, batch)); without one, or for blocks of one or two tiles, one workgroup per (voice, channel) walks
 * the block in ONE launch.  Either way row v holds the float32 samples and the final state that
 * pgx_biquad_varying(row v, ..., the same choice of workspace) gives, bit for bit.
 * n <= 0 or batch <= 0: PGX_OK, nothing launched.  batch > 65535, a stride below its row, a null out / in / params / gains /
 * state: PGX_ERR_INVALID, nothing launched. */
int pgx_biquad_varying_bank(float *out, int64_t out_stride, const float *in, int64_t in_stride, int batch, int64_t n,
                            int channels, double sample_rate, const pgx_biquad_var_params *params, const double *gains,
                            const float *freq, int64_t freq_stride, const float *q, int64_t q_stride,
                            double *state, void *workspace);

/* ------------------------------------------------------------------ SVFilterPE / EnvelopePE / TransformPE
 * (the PEs of benchmarks/profile_biquad_vs_svfilter.py)
 * SVFilterPE: _svf_coefficients_batch_numba + _svf_varying_numba (svfilter_pe.py:65-205).
 * params reuses pgx_biquad_var_params; mode: 0 lowpass,1 highpass,2 bandpass,3 notch,4 peaking,
 * 5 lowshelf,6 highshelf.  gain_a = 10^(gain_db/40).  state[channel] = {s0, s1}. */
int pgx_svf(float *out, const float *in, int64_t n, int channels, double sample_rate,
            const pgx_biquad_var_params *params, const float *freq, const float *q, double gain_a,
            const double *coef /* NULL, or {a00,a01,a10,a11,b0,b1,c0,c1,c2} evaluated by the host
                                  (constant frequency and q; freq and q must then be NULL) */,
            double *state /* [channels][2] */, void *workspace /* as for pgx_biquad_varying */);
/* Bank of SVFilterPEs (voice_bank.py): pgx_svf with the voice in the grid.
 * in / out: `batch` rows of n * channels float32, in_stride / out_stride elements apart (each >= n * channels);
 * freq / q: NULL (voice v takes params[v].freq / params[v].q) or `batch` rows of n float32, freq_stride / q_stride apart (>= n);
 * params: device [batch] (mode and the scalars are per voice);  gains: device [batch], A = 10^(gain_db/40), the number the host
 *         passes pgx_svf by value, per voice;  coef: NULL, or device [batch][9], voice v's host-evaluated constants as pgx_svf
 *         takes them (freq and q must then be NULL);  state: [batch][channels][2];
 * workspace: batch * pgx_scan2_workspace_bytes(n, channels) bytes (voice v's slice starts at v times that), or NULL.
 * With a workspace every voice is rendered by pgx_svf's own plan (the reduce and the apply launch, grid (segments, channels,
 * batch)); without one, or for blocks of one or two tiles, one workgroup per (voice, channel) walks the block in ONE launch.
 * Either way row v holds the float32 samples and the final {s0, s1} that pgx_svf(row v, ..., the same choice of workspace)
 * gives, bit for bit.
 * n <= 0 or batch <= 0: PGX_OK, nothing launched.  batch > 65535, a stride below its row, a null out / in / params / gains /
 * state, coef together with freq or q: PGX_ERR_INVALID, nothing launched. */
int pgx_svf_bank(float *out, int64_t out_stride, const float *in, int64_t in_stride, int batch, int64_t n, int channels,
                 double sample_rate, const pgx_biquad_var_params *params, const double *gains,
                 const float *freq, int64_t freq_stride, const float *q, int64_t q_stride, const double *coef,
                 double *state, void *workspace);

/* EnvelopePE._render (envelope_pe.py:128-206) on the (already look-ahead shifted) source block.
 * one_pole != 0: attack == release, scipy lfilter one-pole as a scan; else the attack/release
 * switch of _envelope_ar_numba (envelope_pe.py:259-271), one lane per channel.
 * rms_window > 0 selects DetectionMode.RMS (block-local uniform_filter1d, mode='nearest'); rms_period > 0: the
 * n frames are several of the caller's blocks of rms_period frames rendered at once, and the detector restarts
 * at every one of their edges (0: one block).
 * state[channel] = envelope; scratch: pgx_envelope_scratch_bytes (detector output + 64-frame block sums, and
 * the pieces / entries of the all-windows form used from 131 072 frames on). */
size_t pgx_envelope_scratch_bytes(int64_t n, int channels);
int pgx_envelope(float *out, const float *in, int64_t n, int channels, double attack_coeff,
                 double release_coeff, int one_pole, int rms_window, int64_t rms_period, double *state,
                 double *scratch);

/* TransformPE._render (transform_pe.py:96-152) for chains of named element-wise operations:
 * float32 -> float64 -> ops in order -> float32.
 * code: 0 affine (p1 + p0*x), 1 clip [p0,p1], 2 sqrt, 3 square, 4 abs, 5 tanh, 6 one_minus. */
typedef struct {
    int32_t code;
    int32_t pad;
    double p0;
    double p1;
} pgx_transform_op;
int pgx_transform(float *out, const float *in, int64_t n_elems, const pgx_transform_op *ops, int nops);
/* A bank of `batch` such chains with the same steps and per-voice parameters (voice_bank.py): voice i runs
 * ops[i * nops .. (i + 1) * nops) over the per_voice elements at in + i * per_voice -- the same arithmetic, one launch
 * (the voice is blockIdx.y; batch <= 65535). */
int pgx_transform_bank(float *out, const float *in, int64_t per_voice, int batch, const pgx_transform_op *ops,
                       int nops);

/* TransformPE chains that hold a tuning step (pygmu2_amd/transforms.py: PitchToFreq, FreqToPitch, SemitonesToRatio,
 * RatioToSemitones over temperament.py's EqualTemperament / JustIntonation): float32 -> float64 -> ops in order ->
 * float32, one launch and one rounding for the whole chain.
 * code 0-6: as pgx_transform, the same arithmetic.  Codes 7-10 read record tunings[op.tuning]:
 *    7  equal, pitch -> freq   reference_freq * 2^((x - reference_pitch) / divisions)
 *    8  equal, freq -> pitch   reference_pitch + divisions * log2(max(x, 1e-10) / reference_freq)
 *    9  just,  pitch -> freq   temperament.py JustIntonation.pitch_to_freq: octave / scale-degree split, linear
 *                              interpolation of the log2 table, exp2, * 2^octave, * reference_freq
 *   10  just,  freq -> pitch   JustIntonation.freq_to_pitch: the nearest table entry (first minimum) in the octave
 * (interval <-> ratio are the same codes with reference_pitch 0 and reference_freq 1.)
 * A just record (num_notes = N >= 2) owns 2N + 1 doubles of `tables` from table_offset: log2(ratios[0..N-1]),
 * log2(ratios[0] * 2.0) -- the upper neighbour of the last entry, across the octave -- and ratios[0..N-1];
 * reference_pitch is the pitch of ratios[0] and reference_freq its frequency.  An equal record has num_notes 0. */
typedef struct {
    int32_t code;
    int32_t tuning;                 /* codes 7-10: index into `tunings` */
    double p0;
    double p1;
} pgx_tuning_op;
typedef struct {
    double reference_pitch;
    double reference_freq;
    double divisions;               /* equal: divisions per octave; just: (double)num_notes */
    int64_t table_offset;
    int32_t num_notes;
    int32_t pad;
} pgx_tuning_record;
/* ops, tunings and tables are device memory that the caller built together (transform_pe.py): op.tuning and
 * table_offset + 2 * num_notes are trusted as the other parameter blocks of this header are; the kernel only reads them. */
int pgx_tuning(float *out, const float *in, int64_t n_elems, const pgx_tuning_op *ops, int nops,
               const pgx_tuning_record *tunings, const double *tables);
/* the same device functions float64 in, float64 out: one op (code 7-10) over one record, for the accuracy test */
int pgx_selftest_tuning(double *out, const double *in, int64_t n, int code, const pgx_tuning_record *tunings,
                        const double *tables);

/* ------------------------------------------------------------------ DelayPE / PiecewisePE / WAV formats
 * (the callers and data formats either side of the path)
 * DelayPE's float / PE delay: interpolated_lookup (interpolated_lookup.py:28-130) over the rendered
 * source window [window_start, window_start + window_len): index = float64(start + i) - delay,
 * linear or Catmull-Rom ("cubic"), neighbours clipped to the window; with bounded != 0 indices
 * outside [extent_start, extent_end) give 0 (delay_pe.py:199-205).  delay: NULL -> delay_scalar. */
int pgx_interp_lookup(float *out, const float *window, int64_t window_start, int64_t window_len,
                      int channels, int64_t start, int64_t n, double delay_scalar, const float *delay,
                      int cubic, int bounded, double extent_start, double extent_end);
/* result_dev[0..1] = min, max of float64(start + i) - delay[i]  (np.min / np.max of the indices,
 * interpolated_lookup.py:111-112): the host sizes the source window from them.  A NaN anywhere in the stream gives
 * (NaN, NaN). */
int pgx_index_range(double *result_dev, const float *delay, int64_t start, int64_t n);
/* ------------------------------------------------------------------ WavetablePE / TimeWarpPE
 * The two other callers of interpolated_lookup, through the same device function as pgx_interp_lookup.
 *
 * WavetablePE._render (wavetable_pe.py:117-169) in one launch: index = float64(indexer[i]) put through the
 * out-of-bounds rule (:146-159), then linear / Catmull-Rom interpolation over the rendered table window
 * [window_start, window_start + window_len), neighbours clipped to it.  oob_mode 0 zero, 1 clamp, 2 wrap; with
 * finite == 0 (a table without a finite extent) the index stays raw in every mode and nothing is masked.
 *   wrap : ((raw - wt_start) % wt_len) + wt_start with numpy's float remainder (fmod, + wt_len if negative);
 *          an index in (wt_end - 1, wt_end) interpolates towards the frame at wt_end, as the reference does
 *   clamp: clip to [wt_start, wt_end - 1]
 *   zero : raw index; 0 where raw < wt_start or raw >= wt_end
 * A window of at most 2560 floats is staged in LDS once per workgroup and the gathers are served from there. */
int pgx_wavetable(float *out, const float *indexer, int64_t n, const float *window, int64_t window_start,
                  int64_t window_len, int channels, int cubic, int oob_mode, int finite, double wt_start,
                  double wt_end);
/* out[0] = 1 if pgx_wavetable would stage the window in LDS for these arguments (PGX_WT_LDS_FLOATS included), out[1] = its
 * grid.  The window is staged when window_len * channels is at most 2560 floats (PGX_WT_LDS_FLOATS: another limit, at
 * most 16384; 0: never) and the n frames make at least as many gathers as that (2 per channel linear, 4 cubic).  Host
 * arithmetic only: needs no device and no pgx_init.  n <= 0: PGX_OK and out = {0, 0}, as pgx_wavetable launches nothing.
 * out is host memory, handed over as a plain address (a ctypes array of two ints, or NULL). */
int pgx_wavetable_plan(int64_t n, int64_t window_len, int channels, int cubic, int out[2]);
/* result_dev[0..1] = min, max of those processed indices (np.min / np.max, interpolated_lookup.py:126-127) for a
 * table whose window is not kept on the device: the host sizes the table render from them.  A NaN anywhere in the
 * stream gives (NaN, NaN). */
int pgx_wavetable_range(double *result_dev, const float *indexer, int64_t n, int oob_mode, int finite,
                        double wt_start, double wt_end);
/* TimeWarpPE._render with a PE rate, index side (timewarp_pe.py:150-163): positions[i] = state[0] +
 * sum(rate[0..i)) (np.cumsum; here a float64 scan over workgroup segments), range_dev[0..1] = min, max of the
 * positions ((NaN, NaN) if any position is NaN), then state[0] += sum(rate).  workspace:
 * PGX_TIMEWARP_WORKSPACE_DOUBLES doubles of scratch. */
#define PGX_TIMEWARP_WORKSPACE_DOUBLES 768
int pgx_timewarp_scan(double *positions, double *range_dev, double *state, double *workspace, const float *rate,
                      int64_t n);
/* TimeWarpPE._render, lookup side (timewarp_pe.py:165-184): interpolation at positions[i], or at
 * pos0 + i * rate when positions is NULL (a scalar rate needs no stream and no scan); 0 where the position is
 * below extent_start (has_start) or at / beyond extent_end (has_end). */
int pgx_timewarp(float *out, int64_t n, const double *positions, double pos0, double rate, const float *window,
                 int64_t window_start, int64_t window_len, int channels, int cubic, int has_start,
                 double extent_start, int has_end, double extent_end);
/* partials_dev[2 p + {0, 1}] = (min, max) of workgroup p's share of the mono stream x[0..n), p < parts <= 1024
 * ((NaN, NaN) if it met a NaN anywhere in its share; (+inf, -inf) if its share is empty): the host folds the pairs,
 * so a NaN anywhere in the stream gives (NaN, NaN).  LadderPE with a PE-driven cutoff / resonance sizes the warm-up
 * of its time segments from the block's lowest cutoff and highest resonance (ladder_pe.py:84-113 clamps). */
int pgx_stream_range(double *partials_dev, int parts, const float *x, int64_t n);
/* PiecewisePE._render (piecewise_pe.py:164-229); times sorted int64, values float64 (device).
 * transition: 0 step, 1 linear, 2 exponential, 3 sigmoid, 4 constant_power. */
int pgx_piecewise(float *out, int64_t start, int64_t n, int channels, const int64_t *times,
                  const double *values, int count, int transition, int hold_first, int hold_last);
/* PortamentoPE._render (portamento_pe.py:154-254 as its docstring states it): `batch` glide lines in one launch on a grid
 * of (tiles, lines); line b writes n frames of `channels` equal samples at out + b * out_stride (>= n * channels).
 * Line b's ramps are entries offsets[b] .. offsets[b + 1] - 1 of the four device arrays, ramp_at non-decreasing within
 * a line.  Ramp i owns the frames [ramp_at[i], ramp_at[i + 1]), the line's last ramp every frame from its ramp_at on, its
 * first also every frame before; two ramps with one ramp_at: the earlier owns nothing.  At frame s of ramp i, x = s -
 * ramp_at[i]: x <= 0 gives ramp_from[i], x >= ramp_len[i] gives ramp_to[i], else ramp_from + (ramp_to - ramp_from) *
 * ((double)x / (double)ramp_len) in float64 (pgx_piecewise's linear transition), rounded once to float32.
 * A line of one held value is one ramp with ramp_from == ramp_to (any ramp_at, ramp_len >= 1); a line without ramps
 * (offsets[b + 1] <= offsets[b]) is silent.  A line's table is read from LDS up to 512 ramps, from global memory
 * beyond.  No workspace.
 * n <= 0 or batch <= 0: PGX_OK, nothing launched.  A null pointer, channels < 1, out_stride < n * channels,
 * batch > 65535: PGX_ERR_INVALID, nothing launched. */
int pgx_portamento(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                   const int64_t *ramp_at, const int64_t *ramp_len, const double *ramp_from,
                   const double *ramp_to, const int32_t *offsets /* [batch + 1] into the ramp arrays */);
/* WavWriterPE / WavReaderPE sample conversion on the device (half the PCIe bytes of float32):
 * libsndfile's PCM_16 rules as python-soundfile configures them (clipping on; the reference's default
 * subtype, wav_writer_pe.py:67): s = x * 32768 saturated to [-32768, 32767], else lrintf; x = s / 32768. */
int pgx_f32_to_pcm16(int16_t *out, const float *in, int64_t n_elems);
int pgx_pcm16_to_f32(float *out, const int16_t *in, int64_t n_elems);

/* ------------------------------------------------------------------ SpatialPE (section 8f rank 2)
 * SpatialAdapter.render (spatial_pe.py:94-144): M -> N channels.
 * The three entry points below average channels as np.mean does a float32 row: fewer than 8 terms one after the
 * other, 8 .. 128 terms on eight running sums joined pairwise; more than 128 source channels are refused. */
int pgx_channel_adapt(float *out, const float *in, int64_t n, int src_channels, int out_channels);
/* SpatialLinear / SpatialConstantPower.render (spatial_pe.py:179-214, 250-286): mono mix of the source
 * panned to stereo; azimuth in degrees, clipped to +-90; azimuth_stream: per-frame float32 or NULL. */
int pgx_pan(float *out, const float *in, int64_t n, int src_channels, float azimuth,
            const float *azimuth_stream, int constant_power);
/* Panned voices of a bank (voice_bank.py).  One device function evaluates a pan gain for pgx_pan and the three entries below.
 * pgx_pan_gains: gains[v] = {lg, rg} of azimuth[v] (device [batch], degrees) as pgx_pan evaluates them for a scalar
 * azimuth -- once, when a bank is built.  batch <= 0: PGX_OK, nothing launched.  A null pointer: PGX_ERR_INVALID. */
int pgx_pan_gains(float *gains /* [batch][2] */, const float *azimuth /* [batch] */, int batch, int constant_power);
/* pgx_pan with the voice in the grid.  in: `batch` rows of n * src_channels float32, in_stride elements apart (>= n *
 * src_channels);  out: `batch` rows of n * 2, out_stride apart (>= n * 2).  Exactly one of gains (device [batch][2] from
 * pgx_pan_gains: scalar azimuths) and azimuth_stream (`batch` rows of n float32, az_stride elements apart, >= n) is non-null.
 * Row v holds what pgx_pan(row v, azimuth v / stream row v) gives, bit for bit.
 * n <= 0 or batch <= 0: PGX_OK, nothing launched.  A null out / in, src_channels outside 1 .. 128, a stride below its row,
 * both or neither of gains / azimuth_stream, batch > 65535: PGX_ERR_INVALID, nothing launched. */
int pgx_pan_bank(float *out, int64_t out_stride, const float *in, int64_t in_stride, int batch, int64_t n,
                 int src_channels, const float *gains, const float *azimuth_stream, int64_t az_stride,
                 int constant_power);
/* out (n, 2) = sum over the voices of pgx_pan(voice): out[f][c] = sum_b float32(mono_b[f] * g_b,c[f]), mono the float32
 * mean of the frame's src_channels, products rounded to float32, added in float32 in voice order starting from voice 0's
 * product -- identical to pgx_pan per voice + pgx_mix_batch, without the [batch][n][2] layer.  in, in_stride (rows of a
 * window allowed), gains, azimuth_stream, az_stride as for pgx_pan_bank; the voice is not in the grid: any batch.
 * n <= 0 or batch <= 0: PGX_OK, nothing launched.  A null out / in, src_channels outside 1 .. 128, a stride below its row,
 * both or neither of gains / azimuth_stream: PGX_ERR_INVALID, nothing launched. */
int pgx_pan_mix_batch(float *out /* [n][2] */, const float *in, int64_t in_stride, int batch, int64_t n, int src_channels,
                      const float *gains, const float *azimuth_stream, int64_t az_stride, int constant_power);
/* out[i] = float32 mean of frame i's channels (the mono mix SpatialHRTF convolves, spatial_pe.py:483) */
int pgx_mono_mean(float *out, const float *in, int64_t n, int src_channels);

/* ------------------------------------------------------------------ LoopPE / WindowPE / DynamicsPE
 * (the remaining configurations of benchmarks/benchmark_pes.py:309-350)
 * LoopPE._render (loop_pe.py:159-232): out[i] = loop[(start + i) mod loop_len] (numpy's non-negative modulo),
 * silence from total_len on (count * loop_len; < 0 = endless); the last `crossfade` frames of the loop blend
 * into its first ones with the reference's float64 weights.  `loop` = the source rendered over the loop region
 * (loop_len, channels).  Bit-exact. */
int pgx_loop(float *out, const float *loop, int64_t start, int64_t n, int channels, int64_t loop_len,
             int64_t total_len, int64_t crossfade);
/* WindowPE._render (window_pe.py:118-254): centred window of 2*half_window + 1 frames; `padded` = the source
 * rendered over [start - half_window, start + n + half_window).  mode 0 max, 1 min, 2 mean, 3 rms;
 * rectify: |x| first.  max / min are exact, mean / rms sum the window directly (the reference differences a
 * cumulative sum).  workspace: pgx_window_workspace_bytes (64-frame block statistics, float64). */
size_t pgx_window_workspace_bytes(int64_t n, int channels, int64_t half_window);
int pgx_window(float *out, const float *padded, int64_t n, int channels, int64_t half_window, int mode,
               int rectify, void *workspace);
/* DynamicsPE._render (dynamics_pe.py:190-372): out = audio * 10**((gain_db(20 log10(max(env, 1e-10))) +
 * makeup) / 20) with numpy's float32 typing of every step.  The host rounds the Python scalars the way numpy's
 * weak-scalar promotion does (pygmu2_amd/dynamics_pe.py). */
typedef struct {
    int mode;              /* 0 compress, 1 limit (ratio = inf), 2 expand, 3 gate */
    int soft;              /* knee > 0 */
    int stereo_link;
    int wide_makeup;       /* the make-up gain is a numpy float64 scalar (automatic value): float64 from its addition on */
    float threshold;       /* float32(threshold) */
    float slope;           /* float32(1/ratio - 1) (compress), float32(ratio - 1) (expand) */
    float neg_slope;       /* float32(-(ratio - 1)) */
    float half_knee;       /* float32(knee / 2) */
    float two_knee;        /* float32(2 * knee) */
    float knee;            /* float32(knee) */
    float knee_lo;         /* float32(threshold - knee/2) */
    float knee_hi;         /* float32(threshold + knee/2) */
    float gate_range;      /* float32(gate_range) */
    float makeup;          /* float32(makeup_gain_db) */
    double gate_range_d;   /* the hard-knee gate is float64 in numpy */
    double makeup_d;
} pgx_dynamics_params;
int pgx_dynamics(float *out, const float *audio, const float *envelope, int64_t n, int channels,
                 int env_channels, const pgx_dynamics_params *params);

/* ------------------------------------------------------------------ BlitSawPE / SuperSawPE
 * BlitSawPE._render (blit_saw_pe.py:150-264): phase cumsum -> mod 1 -> Dirichlet kernel
 * -> leaky integrator -> *2 *amp -> float32.  state[instance] = {phase, integrator}.
 * The caller applies the reset-on-discontinuity rule (blit_saw_pe.py:182-185) by
 * re-initialising state to {initial_phase, 0} before the call.
 * freq/amp/m streams: optional per-sample float32 (frames,1), stride in elements between
 * instances (0 = shared). */
typedef struct {
    double freq;
    double amp;
    double leak;
    double m;              /* <= 0: automatic (largest odd M below Nyquist) */
} pgx_blitsaw_params;
int pgx_blitsaw(float *out, int64_t out_stride, int batch, int64_t n, int channels,
                double sample_rate, const pgx_blitsaw_params *params,
                const float *freq, int64_t freq_stride,
                const float *amp, int64_t amp_stride,
                const float *m, int64_t m_stride,
                double *state /* [batch][2] */,
                void *workspace /* pgx_blitsaw_workspace_bytes, or NULL: one workgroup per instance */,
                double *state_backup /* NULL, or [batch][2]: receives the state on entry -- the snapshot of a caller
                                        that renders a block ahead of its stream and may have to take it back */);
/* A long stream of a few scalar-parameter oscillators is rendered by several workgroups per oscillator
 * (two passes that replay the single workgroup's carry chains: same bits).  0 = not applicable. */
size_t pgx_blitsaw_workspace_bytes(int batch, int64_t n, int streams /* any of freq/amp/m is a stream */);

/* SuperSawPE._render (super_saw_pe.py:287-318): out = float(amp * sum_v double(voice_v))
 * where voice_v is the float32 output of BlitSaw v.  `voices` = [batch*nvoices] float32
 * buffers laid out [instance][voice][frames]; amp stream optional. */
int pgx_supersaw_sum(float *out, int64_t out_stride, int batch, int nvoices, int64_t n,
                     int channels, const float *voices, const double *amp_scalar /* [batch] */,
                     const float *amp, int64_t amp_stride);

/* A bank of mono BiquadPE(BlitSawPE) voices with scalar parameters in one launch: the oscillator's float32
 * samples go through the constant-coefficient section (scipy's DF-II-T order, pgx_biquad_const) without leaving
 * the chip.  params / saw_state as for pgx_blitsaw; coef = [batch][5] {b0,b1,b2,a1,a2}; biquad_state = [batch][2].
 * One workgroup per voice: for banks of >= 128 voices. */
int pgx_blitsaw_biquad_bank(float *out, int64_t out_stride, int batch, int64_t n, double sample_rate,
                            const pgx_blitsaw_params *params, double *saw_state /* [batch][2] */,
                            const double *coef, double *biquad_state /* [batch][2] */);

/* The same chain with sixteen frames per thread: pgx_supersaw_wide's oscillator (under its conditions, which the
 * CALLER checks; saw_tables from pgx_supersaw_wide_tables with one voice per instance) and
 * the settled biquad's filter section on the tables of pgx_biquad_tables.  Agrees with pgx_blitsaw_biquad_bank to a
 * float32 ulp or two (<= 1e-6 of peak asserted), not to the bit. */
int pgx_blitsaw_biquad_wide(float *out, int64_t out_stride, int batch, int64_t n,
                            const double *saw_tables /* [batch] pgx_supersaw_wide_tables(nvoices = 1) */,
                            double *saw_state /* [batch][2] */, const double *coef /* [batch][5] */,
                            const double *biquad_tables /* [batch] pgx_biquad_tables */,
                            double *biquad_state /* [batch][2] */,
                            const float *gain /* NULL, or [batch][gain_stride]: out = float32(voice * gain), GainPE's product */,
                            int64_t gain_stride);
/* The same chain in concurrent time segments for banks of up to 256 voices (a rank's share of a sharded mix), so that a
 * few voices fill the chip with ONE launch: workgroup (voice, s) renders the 4096-frame tiles of segment s.  On entering
 * a segment the oscillator's phase is a product and its integrator level a closed form (the harmonics' steady state plus
 * the decayed remainder of the carried level); the filter has no closed form but forgets: the segment starts
 * ceil(settle_frames / 4096) tiles early from a zero filter state and emits nothing there (settle_frames: the caller's
 * bound for "every entry of A^W below 2^-90", the largest of the bank, > 0).  States are read from the *_in buffers and
 * written to the *_out buffers (two different buffers each).  <= 1e-6 of peak from pgx_blitsaw_biquad_wide. */
int pgx_blitsaw_biquad_wide_segments(int batch, int64_t n, int64_t settle_frames);
int pgx_blitsaw_biquad_wide_seg(float *out, int64_t out_stride, int batch, int64_t n, const double *saw_tables,
                                const double *saw_state_in, double *saw_state_out, const double *coef,
                                const double *biquad_tables, const double *biquad_state_in, double *biquad_state_out,
                                const float *gain, int64_t gain_stride, int64_t settle_frames);

/* MixPE over a bank of such voices -- MixPE(*[GainPE(BiquadPE(BlitSawPE), gain=<envelope>)]) or without the GainPE
 * (mix_pe.py:91-94 over gain_pe.py:104-119, biquad_pe.py:383-404, blit_saw_pe.py:150-264) -- MIXED ON CHIP: out[n] is the
 * mix's block, the [voices][frames] layer between the voices and the mix is never written.  The work is cut into
 * independent (voice, 4096-frame tile) pairs: a workgroup renders a group of voices over the same tile and adds them in a
 * float64 accumulator per frame; the groups' rows of partial sums are then added in group order (a fixed order).  A pair
 * enters with the oscillator's phase (a product), its integrator level (closed form, as pgx_blitsaw_biquad_wide_seg) and a
 * filter started from rest warm_frames before the first frame it emits (warm_frames: a multiple of 16 with every entry of
 * A^warm_frames below 2^-90 for every voice, <= pgx_voice_tiles_max_warm()).  tables: pgx_voice_tiles_tables packs each
 * voice's constants (saw_tables / coef / biquad_tables as for pgx_blitsaw_biquad_wide, plus the per-thread turns of the
 * oscillator's anchor) into one 12 KB block that a workgroup brings into LDS by LDS-DMA, one voice ahead of its use
 * (pgx_voice_tiles_table_bytes(nvoices) bytes).  States are read from the *_in buffers and written to the *_out buffers.
 * The oscillator's sample enters the filter unrounded (BlitSawPE's float32 rounding: 6e-8 of a voice's level); each voice's
 * float32 sample and its float32 product with the gain are the two-PE chain's; the sum is taken in float64 and rounded once (the reference adds float32 in voice
 * order): <= 1e-6 of peak from pgx_blitsaw_biquad_wide + pgx_gain_mix_batch. */
int64_t pgx_voice_tiles_max_warm(void);
size_t pgx_voice_tiles_table_bytes(int nvoices);
int pgx_voice_tiles_tables(double *tables, const double *saw_tables, const double *coef /* [nvoices][5] */,
                           const double *biquad_tables, int nvoices);
size_t pgx_voice_tiles_workspace_bytes(int nvoices, int64_t n, int64_t warm_frames);
/* What the tiles of a block enter with (integrator levels' closed-form terms, first anchors) depends on the oscillators'
 * phases only: pgx_voice_tiles_entries makes it for the block that begins advance_frames after the block saw_state is the
 * start of -- 0: that block itself; n: the next block of a stream, while this one is still being rendered (another
 * stream) -- into set `slot` (0 / 1) of the workspace; pgx_voice_tiles then takes entries_slot = that set, or -1 to make
 * them itself first. */
int pgx_voice_tiles_entries(void *workspace, int slot, int nvoices, int64_t n, const double *tables,
                            const double *saw_state /* [nvoices][2] */, int64_t advance_frames, int64_t warm_frames);
int pgx_voice_tiles(float *out /* [n] */, int nvoices, int64_t n, const double *tables,
                    const double *saw_state_in, double *saw_state_out /* [nvoices][2] */,
                    const double *biquad_state_in, double *biquad_state_out /* [nvoices][2] */,
                    const float *gain /* NULL, or [nvoices][gain_stride] */, int64_t gain_stride, int64_t warm_frames,
                    void *workspace /* pgx_voice_tiles_workspace_bytes(nvoices, n, warm_frames) */, int entries_slot,
                    int next_entries_slot /* -1, or the other set: the entries of the block that follows this one in the
                                             stream are made in the launch that adds the rows (from saw_state_out) */);

/* A bank of scalar-parameter SuperSawPEs in one launch, voices summed on chip: the same samples as
 * pgx_blitsaw over batch*nvoices oscillators followed by pgx_supersaw_sum, bit for bit, without the
 * [batch*nvoices][frames] intermediate (one workgroup per instance, one wave per oscillator; nvoices <= 16).
 * params / state are [batch*nvoices] as for pgx_blitsaw, laid out [instance][voice]. */
int pgx_supersaw_bank(float *out, int64_t out_stride, int batch, int nvoices, int64_t n, int channels,
                      double sample_rate, const pgx_blitsaw_params *params, double *state /* [batch*nvoices][2] */,
                      const double *amp_scalar /* [batch] */);
/* The same bank when a few instances have to fill the chip (a rank's share of a sharded mix): every instance is cut
 * into pgx_supersaw_bank_segments(batch, n) time segments rendered by concurrent workgroups of one launch.  A later
 * segment takes its oscillators' phase sums by replaying the per-tile additions and their integrator levels from
 * the closed form of the leaky integrator's response to the BLIT's harmonics (blit_saw_pe.py:196-235:
 * y = yss(phase) + leak^frames * (y0 - yss(phase0))); needs scalar frequencies, the automatic (odd) M and
 * leak < 1.  Agreement with the sequential recurrence ~1e-14 (float64), i.e. the same float32 samples up to a
 * rounding flip in ~1e-7 of them.  state_in is read, state_out (another buffer) receives the new states. */
int pgx_supersaw_bank_segments(int batch, int64_t n);
int pgx_supersaw_bank_seg(float *out, int64_t out_stride, int batch, int nvoices, int64_t n, int channels,
                          double sample_rate, const pgx_blitsaw_params *params,
                          const double *state_in, double *state_out, const double *amp_scalar /* [batch] */,
                          const double *tables /* pgx_supersaw_bank_tables, or NULL: made by every workgroup */);
/* What the bank's workgroups need per voice and what depends on the parameters only (Dirichlet constants, rotation
 * sines, powers of the leak, per-thread prefix offsets, per-lane scan powers): made once per bank, loaded by every
 * later launch.  The same operations as the in-kernel preparation, hence the same samples. */
size_t pgx_supersaw_bank_table_bytes(int batch, int nvoices);
int pgx_supersaw_bank_tables(double *tables, int batch, int nvoices, double sample_rate,
                             const pgx_blitsaw_params *params);
/* The bank with sixteen frames per thread: the per-thread part of the work (anchor sines, the voice's constants,
 * the integrator scan) is paid half as often -- the bank is bound by instruction issue.  Scalar frequencies >= 1 Hz
 * with the automatic (odd) M and |sin(M pi f/sr)| >= 0.05 only (always true below Nyquist): the CALLER checks that
 * (the rotation / recurrence form of the Dirichlet kernel is the only one here).  Frame phases are frac(phase0 + (i+1) * inc), not k_blitsaw's running sums: the output
 * agrees with pgx_supersaw_bank to ~1e-9 of peak, not to the bit.  Time segments (pgx_supersaw_wide_segments) as in
 * pgx_supersaw_bank_seg; tables from pgx_supersaw_wide_tables (their own layout); state_in != state_out. */
size_t pgx_supersaw_wide_table_bytes(int batch, int nvoices);
int pgx_supersaw_wide_tables(double *tables, int batch, int nvoices, double sample_rate,
                             const pgx_blitsaw_params *params);
int pgx_supersaw_wide_segments(int batch, int nvoices, int64_t n);
int pgx_supersaw_wide(float *out, int64_t out_stride, int batch, int nvoices, int64_t n, int channels,
                      const double *state_in, double *state_out, const double *amp_scalar /* [batch] */,
                      const double *tables);

/* ------------------------------------------------------------------ LadderPE
 * _ladder_process_numba (ladder_pe.py:31-203), the reference's float64 operation order.
 * state[instance][channel] = {z0[4], z1[4], old_input}.
 * settle_frames = 0: one lane per (instance, channel) chain, strictly sequential.
 * settle_frames = W > 0 (host estimate of how many samples the filter needs to forget its state: from the
 * small-signal loop below self-oscillation, a TRIAL value at and above it -- a driven, saturating ladder usually
 * locks to its input although the linearised loop does not decay; the caller reads the counters below and moves to
 * a longer warm-up or to W = 0 when chains fall back): the block is cut into segments that each start W samples
 * early from a zero state; the library verifies every segment against its left neighbour's final
 * state (1e-8 relative) and REPAIRS what disagrees -- the segment behind a bad boundary is rendered again from its
 * neighbour's exit state, sample by sample in the reference's operation order, and so are its successors until the
 * repaired trajectory meets a segment's own entry state again (a chain that disagrees from its first boundary on is
 * the sequential render, bit for bit) -- so W affects speed, never results beyond that bound.  accurate_frames = A (0 < A < W): only the last A warm-up samples
 * of a segment evaluate tanh in float64; the W - A before them, which merely have to forget the zero start,
 * use the float32 exponential unit (state error ~1e-7, contracted by the accurate tail; 0 or >= W: all of the
 * warm-up is accurate).  Warm-ups run on fused multiply-adds; emitted samples keep the reference's operation
 * order.  workspace: pgx_ladder_workspace_bytes(...) bytes
 * (NULL when 0).  Its first 16 bytes are counters, cumulative since the caller zeroed them: int32[0] chains with a
 * repair, int32[1] segmented launches, int64[1] samples repaired (the position does not depend on n). */
typedef struct {
    double freq;
    double resonance;
    double drive;
    double passband_gain;
    int32_t oversample;
    int32_t mode;          /* 0 lp24,1 lp12,2 bp24,3 bp12,4 hp24,5 hp12 */
} pgx_ladder_params;
int pgx_ladder(float *out, int64_t out_stride, const float *in, int64_t in_stride,
               int batch, int64_t n, int channels, double sample_rate,
               const pgx_ladder_params *params,
               const float *freq, const float *resonance, const float *drive, /* batch==1 only */
               double *state /* [batch][channels][9] */, int64_t settle_frames, int64_t accurate_frames,
               void *workspace);
size_t pgx_ladder_workspace_bytes(int batch, int64_t n, int channels, int64_t settle_frames);

/* ------------------------------------------------------------------ CombPE
 * _comb_process_numba (comb_pe.py:26-113): y[n] = x[n] + fb[n] * y[n - D[n]].
 * ring = [batch][2][ring_rows][channels] float64, zero at reset: the last buffer_len outputs, double buffered --
 * a render reads half `parity` and leaves the other half current; the write position on entering a render is
 * total_frames mod buffer_len (total_frames = frames rendered since the reset, kept by the caller).
 *  - scalar frequency (freq == NULL; any batch): params[v].delay = clip(rint(sr / max(max(f, min_f), 1)), 1,
 *    buffer_len - 1) (comb_pe.py:70-77 on the settled smoother), delay_min / delay_max = its range over the batch.
 *    fb (batch == 1) optionally streams the feedback.  Up to 1024 * delay frames the render is the reference's loop
 *    operation for operation; beyond, time segments run concurrently (carries through a float64 affine fold).
 *  - freq != NULL (batch == 1): the smoothed frequency is carried in state[0] (-1 = unset); delays come from a
 *    time-parallel evaluation of the one-pole (comb_pe.py:61-77), the ring runs in LDS.  ring_rows = buffer_len.
 *    The delays are index work: a sample whose sr / f lies within 1e-9 of a rounding tie (where the time-parallel
 *    level and the reference's chain, ~1e-14 apart, could round differently) raises a flag, and the block's delays
 *    are then made again by the reference's loop itself on one lane -- always the reference's integers.
 *    state = double[4]: {smoothed frequency, level on entering the last block, tie flag (int32), blocks redone by the
 *    literal loop (int64)}; the caller sets {-1, 0, 0, 0} at reset. */
typedef struct {
    double feedback;       /* scalar feedback (clamped to +-0.995 by the kernels, non-finite -> 0) */
    int32_t delay;         /* scalar-frequency delay in frames (unused with a frequency stream) */
    int32_t buffer_len;    /* ceil(sr / min_frequency) + 1 rows (comb_pe.py:216-218) */
} pgx_comb_params;
int pgx_comb(float *out, int64_t out_stride, const float *in, int64_t in_stride, int batch, int64_t n,
             int channels, double sample_rate, const pgx_comb_params *params /* device [batch] */,
             int delay_min, int delay_max, const float *freq, const float *fb /* batch == 1 */,
             double min_frequency, int64_t smoothing_samples,
             double *ring, int64_t ring_rows, int64_t total_frames, int parity,
             double *state /* [4], frequency stream only */, void *workspace);
size_t pgx_comb_workspace_bytes(int batch, int64_t n, int channels, int delay_max, int freq_stream);

/* ------------------------------------------------------------------ envelopes / gates
 * PeriodicGate (periodic_gate.py:63-67 over function_gen_pe.py:157-193, scalar params):
 *   gate = (mod(mod(double(n)*dt,1)+phase,1) < duty) ? 1 : 0.  Bit-exact.
 * PeriodicTrigger (periodic_trigger.py:49-58): amp where (n+phase_samples) % period == 0. */
typedef struct {
    double dt;             /* frequency / sample_rate */
    double phase;
    double duty;           /* already clipped to [0,1] */
} pgx_gate_params;
int pgx_periodic_gate(float *out, int64_t out_stride, int batch, int64_t start, int64_t n,
                      const pgx_gate_params *params);
int pgx_periodic_trigger(float *out, int64_t start, int64_t n, int64_t period,
                         int64_t phase_samples, float amplitude);
/* K PeriodicTriggers in one launch (voice_bank.py): row v of `out` (n float32, out_stride elements apart, >= n) holds what
 * pgx_periodic_trigger(start, n, periods[v], phase_samples[v], amplitudes[v]) writes, bit for bit -- the same integer
 * test, the same rule for negative frames.  periods / phase_samples / amplitudes: device [batch] each, every period > 0 (a
 * row whose period is not stays silent).  n <= 0 or batch <= 0: PGX_OK, nothing launched; batch > 65535, a stride below n
 * (batch > 1), a null pointer: PGX_ERR_INVALID. */
int pgx_periodic_trigger_bank(float *out, int64_t out_stride, int batch, int64_t start, int64_t n,
                              const int64_t *periods, const int64_t *phase_samples, const float *amplitudes);
/* PeriodicGate with PE-driven parameters: FunctionGenPE's stateful rectangle path (function_gen_pe.py:169-186).
 * A stream pointer overrides its scalar; state = { carried phase in cycles } (the host zeroes it when a
 * render is not contiguous with the previous one, function_gen_pe.py:170-171). */
int pgx_gate_stateful(float *out, int64_t n, double sample_rate, double freq, double duty, double phase,
                      const float *freq_stream, const float *duty_stream, const float *phase_stream,
                      double *state);

/* ---- control-signal PEs (pgx_control.hip) ------------------------------------------------------------------
 * SampleHoldPE._render (sample_hold_pe.py:73-85) / TrackHoldPE._render (track_hold_pe.py:73-85):
 *   out[i] = src[j][0], j = the last frame <= i with control[j][0] > threshold (0.0 / 0.5, compared in float32);
 *   (float)state[0] where this render has had none yet.  A max-scan over frame indices and a gather: bit-exact.
 * Only channel 0 of src / control is read, in place (the *_channels are the strides).  state = { held value }: the
 * float64 initial value until the first latch, a widened float32 sample afterwards.
 * workspace: PGX_CONTROL_WORKSPACE_DOUBLES * 8 bytes of device scratch (the segments' last passing indices and a
 * copy of the carried value). */
#define PGX_CONTROL_WORKSPACE_DOUBLES 1040
int pgx_hold(float *out, const float *src, int src_channels, const float *control, int control_channels, int64_t n,
             float threshold, double *state, void *workspace);
/* SlewLimiterPE._render (slew_limiter_pe.py:103-135), channel 0 of `in`.  mode 0 LINEAR (:116-124): up / down =
 * rise_rate / sr, fall_rate / sr; mode 1 EXPONENTIAL (:125-132): up / down = min(rate / sr, 1).  Solved time-parallel
 * (Newton rounds over affine pieces; from 131 072 frames on all 8192-frame windows together, with a sequential
 * kernel armed if those rounds run out): samples within ~1e-13 relative of the sequential loop's float64 values.
 * state = { current }; scratch: pgx_slew_scratch_bytes(n).  stats (NULL, or 4 device ints that are added to):
 * inner Newton rounds, windows solved, window-level rounds, fallbacks to the sequential kernel. */
size_t pgx_slew_scratch_bytes(int64_t n);
int pgx_slew(float *out, const float *in, int in_channels, int64_t n, int mode, double up, double down,
             double *state, double *scratch, int *stats);
/* FunctionGenPE._render, every parameter a scalar (function_gen_pe.py:166-168, :180-193): phase =
 * mod(mod((start + i) * dt, 1) + phase, 1); rectangle +-1 (:186) or _piecewise_linear (:121-155); `channels`
 * copies of the column.  duty is clipped to [0, 1] here (:184).  Bit-exact. */
int pgx_function_gen_pure(float *out, int64_t start, int64_t n, int channels, int sawtooth, double dt, double phase,
                          double duty);
/* `batch` pure FunctionGenPEs of one waveform and channel count in one launch (voice_bank.py; function_gen_pe.py:166-168,
 * :180-193 per instance): instance v writes n frames of `channels` interleaved copies at out + v * out_stride, the
 * samples of pgx_function_gen_pure(start, n, channels, sawtooth, params[v].dt, params[v].phase, params[v].duty) -- the
 * same per-sample device function, the instance in the grid.  Bit-exact.  dt = freq / sample_rate as the PE forms it.
 * n <= 0 or batch <= 0: nothing is launched.  A null pointer, channels < 1, out_stride < n * channels (batch > 1),
 * batch > 65535: PGX_ERR_INVALID.
 * pgx_function_gen_params is { double dt; double phase; double duty; } -- pgx_gate_params' record under the name of
 * this PE (the gate is this generator's rectangle, periodic_gate.py:63-67); duty is clipped in the kernel here. */
typedef pgx_gate_params pgx_function_gen_params;
int pgx_function_gen_bank(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                          int sawtooth, const pgx_function_gen_params *params);
/* FunctionGenPE._render with any PE parameter (function_gen_pe.py:169-177): base = mod(state[0] + [0,
 * cumsum(f / sr)[:-1]], 1), then state[0] = mod(state[0] + sum(f / sr), 1); the float64 prefix sum runs over
 * workgroup segments.  A stream pointer (mono, n floats) overrides its scalar; the host zeroes the state when a
 * render does not continue the previous one (:170-171).  workspace: PGX_CONTROL_WORKSPACE_DOUBLES doubles. */
int pgx_function_gen_stateful(float *out, int64_t n, int channels, int sawtooth, double sample_rate, double freq,
                              double duty, double phase, const float *freq_stream, const float *duty_stream,
                              const float *phase_stream, double *state, double *workspace);

/* AdsrGatedPE._render (adsr_pe.py:124-196) / AdsrTriggeredPE._render (adsr_pe.py:279-335):
 * the reference's sequential float64 accumulation reproduced bit for bit (binade-linear runs, see
 * pgx_adsr.hip).  state[instance] = {state enum, env, prev_gate | sustain_ends_at}.
 * workspace: >= pgx_adsr_workspace_bytes(batch, n) bytes of device scratch (edge masks).
 * A lone gated envelope (batch == 1) over 196 608 frames or more -- a look-ahead window -- is walked with its 65 536-frame
 * chunks as one batch, in rounds (every chunk from the carried state, then from its left neighbour's exit; settled when
 * two rounds' exits agree bit for bit -- every completed attack pins the state, so two rounds settle any envelope
 * whose chunks each hold one); this one case WAITS for the device once per call to read the verdict, and a render
 * that has not settled after three rounds is walked chunk after chunk.  Same samples either way. */
typedef struct {
    double attack_dvdt;
    double decay_dvdt;
    double release_dvdt;
    double sustain_level;
    int64_t sustain_samples;   /* triggered variant only */
} pgx_adsr_params;
size_t pgx_adsr_workspace_bytes(int batch, int64_t n);
int pgx_adsr_gated(float *out, int64_t out_stride, const float *gate, int64_t gate_stride,
                   int batch, int64_t n, const pgx_adsr_params *params, double *state, void *workspace);
/* AdsrGatedPE(PeriodicGate(scalar params)): the gate of pgx_periodic_gate is evaluated inside the
 * envelope kernels, sample for sample the same values, without materialising the gate buffer.
 * detach_walk != 0: after the (parallel) edge search the library forks (pgx_stream_fork), enqueues the
 * envelope walk -- one latency-bound wave per envelope -- on the side stream and selects the main
 * stream again; the caller enqueues independent work and must call pgx_stream_join() before any call
 * that reads `out` or touches `state`.  Not allowed while already forked. */
int pgx_adsr_gated_periodic(float *out, int64_t out_stride, int batch, int64_t start, int64_t n,
                            const pgx_gate_params *gates, const pgx_adsr_params *params, double *state,
                            void *workspace, int detach_walk);
/* The same block with the carried state read from one buffer and written to another (a block rendered ahead of the
 * caller's stream -- voice_bank.py: the states it started from stay where they are, a pull that turns out not to be
 * this block costs nothing to undo).  detach_walk = 0: everything on the current stream; != 0: as above -- the edge search on
 * the current stream, then the fork and the walk on the side stream (the caller joins or detaches). */
int pgx_adsr_gated_periodic_to(float *out, int64_t out_stride, int batch, int64_t start, int64_t n,
                               const pgx_gate_params *gates, const pgx_adsr_params *params,
                               const double *state_in, double *state_out, void *workspace, int detach_walk);
int pgx_adsr_triggered(float *out, int64_t out_stride, const float *trig, int64_t trig_stride,
                       int batch, int64_t start, int64_t n, const pgx_adsr_params *params,
                       double *state, void *workspace);

/* ------------------------------------------------------------------ ConvolvePE
 * ConvolvePE._render (convolve_pe.py:250-342): y = x * h (linear, streaming).  The
 * reference evaluates it by float64 FFT overlap-save; this library evaluates the same sum
 * directly as a Toeplitz(h) x Hankel(x) matrix product on the f32 MFMA units with
 * float64 accumulation across K-slabs.
 *   x:     (n, src_ch) float32 current block
 *   hist:  (L-1, out_ch) float32 previous inputs (fanned out), updated in place
 *   h:     (L, fir_ch) float32
 *   out:   (n, out_ch) float32
 * workspace >= pgx_convolve_workspace_bytes(n, L, out_ch). */
size_t pgx_convolve_workspace_bytes(int64_t n, int64_t fir_len, int out_channels);
int pgx_convolve(float *out, const float *x, int64_t n, int src_channels,
                 const float *h, int64_t fir_len, int fir_channels, int out_channels,
                 float *hist, void *workspace);

/* Long filters: the same convolution by float64 FFT overlap-save, hand-written (four-step N1 x N2
 * decomposition, Stockham radix-4 FFTs of 4096 points per workgroup in LDS, spectrum kept in the
 * order the forward pass produces it, two real blocks packed per complex transform).
 *   fft_size = pgx_convolve_fft_size(L): power of two >= 2L in [4096, 262144], 0 if L is too long
 *   spectrum: pgx_convolve_fft_spectrum_bytes(...) bytes, filled once per filter by _prepare
 *   workspace >= pgx_convolve_fft_workspace_bytes(n, L, out_ch, fft_size)
 * x, hist, out as for pgx_convolve; hist is updated in place. */
int64_t pgx_convolve_fft_size(int64_t fir_len);
size_t pgx_convolve_fft_spectrum_bytes(int64_t fft_size, int fir_channels);
size_t pgx_convolve_fft_workspace_bytes(int64_t n, int64_t fir_len, int out_channels, int64_t fft_size);
int pgx_convolve_fft_prepare(void *spectrum, const float *h, int64_t fir_len, int fir_channels,
                             int64_t fft_size);
int pgx_convolve_fft(float *out, const float *x, int64_t n, int src_channels, const void *spectrum,
                     int64_t fir_len, int fir_channels, int out_channels, int64_t fft_size,
                     float *hist, void *workspace,
                     int hist_is_zero /* fresh stream: the history counts as zeros and is only written */);

/* ------------------------------------------------------------------ multi-GPU exchange (RCCL over xGMI)
 * The one exchange step of the path: the partial mixes of a MixPE whose inputs are dealt i mod world over
 * the ranks are summed (mix_pe.py:91-94 is the sum being distributed).  One process
 * per GPU.  librccl is loaded on demand by these entry points only.
 *   pgx_comm_unique_id   rank 0 creates the 128-byte rendezvous id; the host hands it to every rank
 *                        (any channel: a file, MPI, torch.distributed's store ...)
 *   pgx_comm_init        collective: every rank calls it with the same id, after pgx_init(device)
 *   pgx_allreduce_sum    out[i] = sum over ranks of in[i] (float32, n elements; out may equal in).  Runs on
 *                        the library's collective stream, ordered behind everything enqueued on the library
 *                        stream so far; asynchronous.  `in` and `out` must stay allocated until the ticket
 *                        has been waited for.  The call records the ordering event and queues the job; a thread
 *                        of the library's own hands the jobs to RCCL in call order (PGX_COMM_THREAD=0: the
 *                        caller does, 16-18 us of host time per call).  Calls must come from one thread.
 *   pgx_allreduce_wait   orders the library stream behind the collective of `ticket` (stream-level wait:
 *                        the host blocks only until that collective has been handed to RCCL -- normally long
 *                        ago), after which `out` may be read and `in` released
 *   pgx_allreduce_scalar_host   synchronous sum (op 0) / max (op 1) of one host double over the ranks
 *   pgx_comm_fold_check  every rank must issue the same sequence of collectives with the same counts.  The first 8
 *                        tickets and every 16th after them (PGX_COMM_CHECK_FIRST / _EVERY) are preceded by a 32-byte
 *                        all-reduce(max) of {n, -n, h, -h}: n this collective's count, h a running hash of every count
 *                        so far and of every word folded in here (the caller's shared facts: window or block, rows,
 *                        switches).  Ranks that disagree get PGX_ERR_RUNTIME ("ranks out of step ...") from the
 *                        next call on the communicator instead of a hang or a corrupted sum; a check that does not
 *                        complete within PGX_COMM_CHECK_TIMEOUT_MS (60 s) fails the same way.
 *   pgx_comm_stats       tickets issued, agreement checks completed, current sequence hash (any pointer may be NULL)
 *   pgx_comm_quiesce     PGX_OK once everything handed to the communicator has completed, PGX_ERR_RUNTIME after
 *                        `timeout_ms` (a peer that died mid-collective never completes ours).  pgx_comm_destroy /
 *                        pgx_shutdown use it with PGX_COMM_EXIT_TIMEOUT_MS (10 s): past the deadline the communicator
 *                        is ABANDONED -- nothing of it is joined, synchronised or destroyed -- both return
 *                        PGX_ERR_RUNTIME and pgx_comm_abandoned() says 1: the process should exit non-zero. */
size_t pgx_comm_unique_id_bytes(void);
int pgx_comm_unique_id(void *id_host, size_t len);
int pgx_comm_init(int rank, int world, const void *id_host, size_t len);
int pgx_comm_info(PGX_HOST int *rank, PGX_HOST int *world);        /* world == 0: no communicator */
int pgx_comm_destroy(void);
int pgx_comm_quiesce(int timeout_ms);
int pgx_comm_abandoned(void);
int pgx_comm_fold_check(int64_t word);
int pgx_comm_stats(PGX_HOST int64_t *issued, PGX_HOST int64_t *checks, PGX_HOST int64_t *hash);
int pgx_allreduce_sum(float *out, const float *in, size_t n, PGX_HOST int64_t *ticket);
int pgx_allreduce_wait(int64_t ticket);
int pgx_allreduce_scalar_host(PGX_HOST double *value_host, int op);

/* ------------------------------------------------------------------ KarplusStrongPE / AnalogOscPE (pgx_sources.hip)
 * KarplusStrongPE._render (karplus_strong_pe.py:137-213): a one-period circular line of float32 noise (drawn and
 * uploaded by the caller at the first render after a reset; state zeroed), fed back through the two-point average
 * times rho and a first-order allpass, in the reference's float32 operation order: bit-exact.  `batch` strings, each
 * with its own params[i], line (lines + params[i].line_offset, params[i].n floats) and state[i]; string i writes n
 * frames of `channels` identical copies at out + i * out_stride.  start = absolute index of the first generated frame
 * (>= 0: the caller zero-fills frames before 0), which the two-phase switch is compared with.  max_line >= every
 * params[i].n: lines of a workgroup's strings that fit in 64 KiB are staged in LDS for the render. */
typedef struct {
    int64_t line_offset;   /* floats from `lines` to this string's line */
    int32_t n;             /* N = max(2, floor(sr / f)) */
    int32_t two_phase;     /* duration and rho_damping both given */
    int64_t switch_at;     /* absolute frame from which rho_damping applies */
    float rho;             /* float32(rho), float32(rho_damping), float32(allpass c) */
    float rho_damping;
    float c;
    float pad;
} pgx_ks_params;
typedef struct {
    int32_t r;             /* read position */
    float ap_in;           /* allpass input / output of the previous frame */
    float ap_out;
    int32_t pad;
} pgx_ks_state;
int pgx_karplus_strong(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                       const pgx_ks_params *params, float *lines, pgx_ks_state *state, int max_line);
/* The plucks of a score in one launch (MixPE over DelayPE / CropPE of KarplusStrongPE, sequence_pe.py / mix_pe.py:69-96):
 * `count` strings, each with its own parameter block, line (line + params->line_offset), state, first frame in its own
 * time (>= 0), frame count (>= 0) and destination out + dst (floats; frames * channels of them, disjoint from every
 * other string's).  The same arithmetic as pgx_karplus_strong, string by string: bit-exact.  notes[] is device memory.
 * `group` strings (1..64) share a workgroup; a workgroup whose lines fit in 64 KiB stages them in LDS, any other reads
 * its lines in global memory.  max_line >= every params->n >= 2 (a workgroup holding a line outside that renders
 * nothing).  Lanes of one workgroup
 * run until the longest of them is done: the caller orders notes[] by frame count.  notes_on_host != 0: notes[] is
 * HOST memory with count <= PGX_SCORE_INLINE entries, which travel in the kernel arguments (nothing is uploaded; the
 * array may be reused as soon as the call returns). */
typedef struct {
    const pgx_ks_params *params;
    float *line;
    pgx_ks_state *state;
    int64_t start;
    int64_t frames;
    int64_t dst;
} pgx_ks_note;
#define PGX_SCORE_INLINE 16
int pgx_karplus_score(float *out, int channels, const pgx_ks_note *notes, int count, int group, int max_line,
                      int notes_on_host);

/* AnalogOscPE._render (analog_osc_pe.py:203-267), float64 inside, float32 out, `channels` identical copies.
 * waveform 0 = "rectangle", 1 = "sawtooth".  Pure form (scalar parameters): phase = mod(index * f / sr, 1)
 * (:185-187); the sawtooth integrates its corrected derivative from y0 = _piecewise_linear_value(phase[0]) within
 * this render (:253-256).  Stateful form: freq_stream / duty_stream are optional float32 (frames, 1) streams
 * overriding the scalar; state = { carried phase, carried saw value } (:189-193, :262-263); restart != 0 (a render not
 * contiguous with the previous one) starts from phase 0 / saw -1.  workspace: pgx_analog_osc_workspace_bytes(n)
 * bytes of device scratch (the pure rectangle needs none). */
size_t pgx_analog_osc_workspace_bytes(int64_t n);
int pgx_analog_osc_pure(float *out, int64_t start, int64_t n, int channels, double sample_rate, int waveform,
                        double freq, double duty, void *workspace);
int pgx_analog_osc_stateful(float *out, int64_t n, int channels, double sample_rate, int waveform, double freq,
                            double duty, const float *freq_stream, const float *duty_stream, int restart,
                            double *state /* [2] */, void *workspace);

/* A bank of `batch` AnalogOscPEs of one waveform and channel count (voice_bank.py): the same kernels with the voice in
 * blockIdx.y (the single entry points above are batch = 1), so a bank takes as many launches as one PE -- 1 (pure
 * rectangle), 3 (pure sawtooth, stateful rectangle), 5 (stateful sawtooth) -- and voice i gets, operation for
 * operation, the samples of pgx_analog_osc_pure / pgx_analog_osc_stateful for that voice alone.  Voice i writes n
 * frames at out + i * out_stride, reads params[i] (device memory), its (n, 1) streams at freq_streams + i * freq_stride
 * / duty_streams + i * duty_stride (NULL: the scalar of params[i]), carries state[i] and scans in its own
 * pgx_analog_osc_workspace_bytes(n) slice of `workspace`.  stateful == 0: the pure form -- both streams must be NULL,
 * `state` is unused, `start` is the first frame's index; the rectangle needs no workspace.  stateful != 0: the carried
 * form (`start` is unused), restart as above for every voice.  batch <= 65535. */
typedef struct {
    double freq;
    double duty;
} pgx_osc_params;
size_t pgx_analog_osc_bank_workspace_bytes(int64_t n, int batch);
int pgx_analog_osc_bank(float *out, int64_t out_stride, int batch, int64_t start, int64_t n, int channels,
                        double sample_rate, int waveform, const pgx_osc_params *params /* [batch] */,
                        const float *freq_streams, int64_t freq_stride, const float *duty_streams,
                        int64_t duty_stride, int stateful, int restart, double *state /* [batch][2] */,
                        void *workspace);

/* ------------------------------------------------------------------ NoisePE (pgx_noise.hip)
 * NoisePE._render (noise_pe.py:111-165): np.random.default_rng(seed).uniform(-1, 1, n).astype(float32) drawn on the
 * device (numpy's PCG64: a 128-bit LCG with the XSL-RR output, reached at any draw number by a table skip-ahead), then
 * white as drawn, Paul Kellet's pink filter, or the clamped brown walk, in the reference's float32 operation order:
 * bit-exact, however a stream is cut into renders.  `batch` independent instances; instance i writes n frames at
 * out + i * out_stride, reads params[i] and carries state[i] (pink and brown).  An instance's first frame is draw number
 * params[i].consumed + draws of its stream (modulo 2^64); the caller adds n to `draws` after every render.  White is
 * one launch of many workgroups; pink and brown are one launch of a workgroup per instance that steps the recurrence
 * literally.
 * pgx_noise_skip_table: the 64 pairs (M^(2^k), S_(2^k)) the skip-ahead uses, as {a_hi, a_lo, c_hi, c_lo} per k
 * (256 words); needs no device. */
typedef struct {
    uint64_t state_hi, state_lo;   /* PCG64 state and increment as numpy reports them for the seed */
    uint64_t inc_hi, inc_lo;
    int64_t consumed;              /* draws taken from the stream before `draws` started counting */
    int32_t scaled;                /* 0: (min_value, max_value) == (-1, 1), the draw passes untouched */
    float span;                    /* float32(max_value - min_value) */
    float min_value;               /* float32(min_value) */
    int32_t pad;
} pgx_noise_params;
typedef struct {
    float pink[7];                 /* b0..b6 */
    float brown;                   /* the level */
} pgx_noise_state;
int pgx_noise_skip_table(uint64_t *table /* [256] */);
int pgx_noise_white(float *out, int64_t out_stride, int batch, int64_t n, uint64_t draws,
                    const pgx_noise_params *params);
int pgx_noise_pink(float *out, int64_t out_stride, int batch, int64_t n, uint64_t draws,
                   const pgx_noise_params *params, pgx_noise_state *state);
int pgx_noise_brown(float *out, int64_t out_stride, int batch, int64_t n, uint64_t draws,
                    const pgx_noise_params *params, pgx_noise_state *state);

/* ------------------------------------------------------------------ arbitrary-length DFT, TralfamPE (pgx_spectral.hip)
 * Complex float64 DFT of any length 1 <= n <= pgx_dft_max_length() = 2^21, `batch` sequences of n {double re, im}
 * points lying n apart; numpy's convention: forward unnormalised, inverse scaled 1/n.  A power of two is a Stockham
 * FFT held in LDS (n <= 2048: one launch) or the four-step decomposition (two launches); every other length is
 * Bluestein's chirp-z over M = 2^ceil(log2(2n - 1)) points with the chirp phase k^2 mod 2n reduced in 64-bit
 * integers.  Every twiddle is evaluated in float64 from an exactly reduced index, never recurred.
 *   pgx_dft_plan_bytes / pgx_dft_plan   what depends on n alone (the chirp and its spectrum; for a power of two the
 *                                       plan is empty but must still be a valid 16-byte block), made once per length.
 *                                       Layout, in {double re, im} points, M as above:
 *                                         chirp[n]     b_k = exp(i*pi*k^2/n), k < n
 *                                         spectrum[M]  the forward DFT of b wrapped to M points: b_j for j < n,
 *                                                      b_(M-j) for j > M - n, 0 between
 *                                         scratch[M]   only when M > 2048: the column pass of that DFT; not read again
 *   pgx_dft_workspace_bytes             scratch of one call; 0 for an unsupported n or batch
 *   pgx_dft_c2c                         out == in is allowed; out, in, plan and workspace are device memory
 * The three *_bytes helpers and pgx_dft_max_length are pure planning helpers: they need no device.  A longer n is
 * PGX_ERR_INVALID.
 *
 * pgx_tralfam: TralfamPE._mogrify (tralfam_pe.py:88-105) for x = float32 (n, channels) interleaved: per channel the
 * DFT of the whole extent, magnitudes kept, every phase replaced by rng.random((n, channels)) * 2.0 * pi -- draw
 * k * channels + c of the PCG64 stream that rng[0] describes (state, inc, consumed; the other fields are not read), as
 * u = (raw >> 11) * 2^-53 -- inverse DFT, real part rounded to float32 into out (n, channels).  normalize_peak > 0:
 * then the max |out| over all channels is reduced on the device and out is scaled in place by
 * float32(normalize_peak) / peak (float32 division and product; nothing when the peak is 0).  plan: pgx_dft_plan of n;
 * workspace: pgx_tralfam_workspace_bytes(n, channels). */
int64_t pgx_dft_max_length(void);
size_t pgx_dft_plan_bytes(int64_t n);
size_t pgx_dft_workspace_bytes(int64_t n, int batch);
int pgx_dft_plan(void *plan, int64_t n);
int pgx_dft_c2c(void *out, const void *in, int64_t n, int batch, int inverse, const void *plan, void *workspace);
size_t pgx_tralfam_workspace_bytes(int64_t n, int channels);
int pgx_tralfam(float *out, const float *x, int64_t n, int channels, const pgx_noise_params *rng,
                double normalize_peak /* <= 0: none */, const void *plan, void *workspace);

/* ------------------------------------------------------------------ score mix (pgx_score.hip)
 * MixPE._render (mix_pe.py:69-96) over inputs that each occupy part of the block: out[f] = the float32 sum, in list
 * order, one rounding per add, of the segments that cover frame f; 0 where none does.  A segment is `frames` frames of
 * `channels` interleaved floats at `data`, the first of them frame `first` of the block (0 <= first,
 * first + frames <= the block's frames).  The block is cut into tiles of tile_frames frames; tile t adds the segments
 * tile_list[tile_offsets[t] .. tile_offsets[t + 1]) (indices into segs[], in the order they are to be added; the
 * caller lists every segment that touches the tile, a listed segment that does not is harmless).  One workgroup per
 * tile.  segs, tile_offsets (tiles + 1 entries) and tile_list are device memory; n_segs == 0 zero-fills.
 * tile_list == NULL: segs is HOST memory with n_segs <= PGX_SCORE_INLINE entries, which travel in the kernel arguments
 * (nothing is uploaded), and every tile walks all of them in order; tile_offsets is not read. */
typedef struct {
    const float *data;
    int64_t first;
    int64_t frames;
} pgx_score_seg;
int pgx_score_mix(float *out, int64_t frames, int channels, const pgx_score_seg *segs, int64_t n_segs,
                  const int32_t *tile_offsets, const int32_t *tile_list, int64_t tile_frames);

/* ------------------------------------------------------------------ restart bank (pgx_restart.hip)
 * TriggerRestartPE._render (trigger_restart_pe.py:72-98) and RandomSelectPE (random_select_pe.py:79-95) over sources
 * whose samples depend on the frame index alone: a scan of the trigger block plus a gather from "takes" -- stretches of
 * the sources rendered once -- instead of one render and one copy per event.  An event is a trigger sample > 0 (NaN
 * and negative samples are none, +2 is one); only channel 0 of the trigger is read (trigger_stride floats per frame).
 * The block is cut into tiles of PGX_RESTART_TILE frames and at most PGX_RESTART_MAX_SEGMENTS segments of whole tiles,
 * one workgroup each; all arithmetic on indices is integer, so no result depends on that cut.
 *
 * pgx_restart_plan: summary_dev[0..4) = {events, index of the first (n: none), index of the last (-1: none), frames of
 * the longest stretch [event, next event or n) (0: none)}.  workspace: PGX_RESTART_WORKSPACE_INT64 int64 of device
 * scratch; it keeps the segments' partial results for pgx_restart_gather over the same trigger block.
 *
 * pgx_restart_gather: for frame t, ordinal = events at positions <= t and local = t - the last of them (ordinal 0:
 * local = carry_local + t, the local time of frame 0 on the clock that runs in from earlier blocks; carry_local < 0:
 * nothing has ever started).  slot = sel_dev[ordinal]; sel_dev has n_sel entries, entry 0 names the take of the
 * running stretch, entry k that of the block's k-th event.  out[t, c] = takes[slot].ptr[(local - first) * channels + c]
 * where first <= local < first + len, else 0; also 0 for a slot outside [0, n_takes), an ordinal outside [0, n_sel)
 * and for ordinal 0 with carry_local < 0.  local is 64-bit throughout.  Nothing but `out` is written. */
#define PGX_RESTART_TILE 2048
#define PGX_RESTART_MAX_SEGMENTS 1024
#define PGX_RESTART_WORKSPACE_INT64 (4 * PGX_RESTART_MAX_SEGMENTS)
typedef struct {
    const float *ptr;      /* len frames of `channels` interleaved floats: the source at local times first .. */
    int64_t first;
    int64_t len;
} pgx_restart_take;
int pgx_restart_plan(int64_t *summary_dev, void *workspace, const float *trigger, int trigger_stride, int64_t n);
int pgx_restart_gather(float *out, int64_t n, int channels, const float *trigger, int trigger_stride,
                       const void *workspace, int64_t carry_local, const int32_t *sel_dev, int64_t n_sel,
                       const pgx_restart_take *takes_dev, int n_takes);

/* ------------------------------------------------------------------ ReversePitchEchoPE (pgx_reverse_echo.hip)
 * ReversePitchEchoPE._render through _reverse_pitch_echo_numba (reverse_pitch_echo_pe.py:30-265): the block-size
 * one-pole, the two-head pitch shifter and the double-buffered reversed echo.  float32 in (n frames of `channels`
 * interleaved), float32 out (the windowed playback alone), float64 inside.  Each of block_seconds / pitch_ratio /
 * feedback / alternate is the scalar, or a float32 (n, 1) stream that overrides it (widened to float64 on load).
 *
 * Everything carried from one render to the next lives on the device: the record below, the two echo buffers
 * (rows * channels float64 each, row-major; rows = max(65, int(10 * sample_rate))) and the pitch history
 * (2 * pitch_len * channels float64; pitch_len = max(2, int(sample_rate / 60))).  The pitch history is the reference's
 * circular buffer in time order: row j of half `pitch_parity` is the input pitch_len - j frames before the next one;
 * each render writes the other half.  A new stream starts from zeroed buffers and a record of {smoothed = the
 * clamped, rounded initial size, current_is_a = 1, reverse = 1, everything else 0}.
 *
 * Three launches: a one-workgroup plan (float64 scans of the smoothed size and of the read position, re-associated;
 * one lane walks the echo-block boundaries, one step per echo block of >= PGX_REVERSE_ECHO_MIN_BLOCK frames), a
 * grid-wide pitch stage and an echo stage of one workgroup per channel; no workgroup reads what another wrote in the
 * same launch.  A pitch ratio is taken as >= PGX_REVERSE_ECHO_MIN_RATIO (NaN too) and is expected to stay below
 * pitch_len, where the reference's read position stays inside its buffer.
 * workspace: pgx_reverse_echo_workspace_bytes(n, channels) bytes of device scratch (0 for n < 1).
 * PGX_ERR_INVALID, whether or not the library is initialised: a null state / buffer pointer (out / in / workspace may
 * be null for n == 0 only), channels < 1, n < 0, rows <= PGX_REVERSE_ECHO_MIN_BLOCK, pitch_len < 2,
 * smoothing_samples < 1, a sample rate that is not positive.  n == 0: success, nothing is launched. */
#define PGX_REVERSE_ECHO_MIN_BLOCK 64
#define PGX_REVERSE_ECHO_MAX_FEEDBACK 0.995
#define PGX_REVERSE_ECHO_MIN_RATIO 0.001
#define PGX_REVERSE_ECHO_UNITY_BAND 1e-4
typedef struct {
    double smoothed;          /* _smoothed_block_samples */
    double read_pos;          /* _pitch_read_pos, in [0, pitch_len) */
    int64_t write_idx;        /* _write_idx */
    int64_t read_idx;         /* _read_idx: moves with write_idx */
    int64_t current_block;    /* _current_block_samples: locked at write_idx == 0 */
    int64_t prev_len;         /* _previous_block_samples */
    int64_t pitch_write_pos;  /* _pitch_write_pos */
    int32_t reverse;          /* _playback_reverse */
    int32_t current_is_a;     /* _current_is_a */
    int32_t pitch_parity;     /* the half of the pitch history the next render reads */
    int32_t pad;
} pgx_reverse_echo_state;
size_t pgx_reverse_echo_workspace_bytes(int64_t n, int channels);
int pgx_reverse_echo(float *out, const float *in, int64_t n, int channels, double sample_rate, double block_seconds,
                     const float *block_stream, double pitch_ratio, const float *pitch_stream, double feedback,
                     const float *feedback_stream, double alternate, const float *alternate_stream,
                     int64_t smoothing_samples, pgx_reverse_echo_state *state, double *echo_a, double *echo_b,
                     int64_t rows, double *pitch_history, int64_t pitch_len, void *workspace);

/* ------------------------------------------------------------------ MeltysynthPE: SoundFont voices (pgx_soundfont.hip)
 * The audio plane of the reference's meltysynth port: Oscillator._fill_block_no_loop_np / _fill_block_continuous_np,
 * BiQuadFilter.process and Synthesizer._write_block, played from a render table that the host's control plane
 * (pygmu2_amd/soundfont/synth.py) emits: one row per (block, audible voice), blocks in order, the rows of block b at
 * block_rows[b] .. block_rows[b + 1] (n_blocks + 1 int32, block_rows[0] = 0, block_rows[n_blocks] = n_rows) in the order
 * they are mixed.  A row is PGX_SOUNDFONT_ICOLS int32 of rows_i and PGX_SOUNDFONT_DCOLS float64 of rows_d, row-major:
 *   rows_i  0 voice       id of the voice object, 0 <= id < polyphony, at most once per block; it owns the filter state
 *           1 flags       1: zero the filter state before this block; 2: looping oscillator; 4: the low-pass is active
 *           2 end, 3 start_loop, 4 end_loop     sample frames
 *           5 mix_left, 6 mix_right             0 skip, 1 constant gain, 2 slope;  7 unused
 *   rows_d  0 position at the block's first frame, 1 pitch ratio: frame t reads at position + t * ratio
 *           2..6 a0 a1 a2 a3 a4: y = a0*x + a1*x1 + a2*x2 - a3*y1 - a4*y2, float64, summed left to right
 *           7, 8 left: {gain, -} for a constant, {gain at frame 0, step per frame} for a slope;  9, 10 right
 * wave: wave_len int16 samples, s * (1 / 32768) in float64 on load.  No index leaves it: a gather outside
 * [0, wave_len) reads 0.0.  Not looping: frames with position < end interpolate wave[lo], wave[lo + 1], the others are
 * 0.  Looping: the position is wrapped as start_loop + numpy_mod(position - start_loop, end_loop - start_loop), and
 * lo + 1 is start_loop once it reaches end_loop.  An inactive filter passes the block through and takes its state from
 * the block's last two frames.  filter_state: 4 * polyphony float64 {x1, x2, y1, y2} per voice object, carried across
 * blocks and calls; zeroed by the caller at the start of a stream.
 * Mix: per frame dest = 0.0, then dest = dest + g * x per row in table order, one rounding to float32, interleaved
 * stereo.  Frame f of the n_blocks * block_size rendered goes to out[f] for f < n_frames and to carry[f - n_frames]
 * otherwise; (n_blocks - 1) * block_size <= n_frames <= n_blocks * block_size, carry holds block_size frames.
 * scratch: n_rows * block_size float64 of device memory (at least one).  Everything but the counts is device memory.
 * Two launches (one when n_rows == 0), whatever the number of voices and blocks.  The integer columns are read back
 * first: PGX_ERR_INVALID with nothing launched and nothing written for a null pointer, block_size outside 8 .. 1024,
 * polyphony outside 1 .. 256, a negative count, n_frames outside the last block, offsets that do not span the rows, a
 * voice id outside the polyphony or twice in a block, an unknown mix mode.  n_blocks == 0: PGX_OK, nothing launched. */
#define PGX_SOUNDFONT_ICOLS 8
#define PGX_SOUNDFONT_DCOLS 11
int pgx_soundfont_render(float *out, int64_t n_frames, float *carry, const int16_t *wave, int64_t wave_len,
                         const int32_t *block_rows, const int32_t *rows_i, const double *rows_d, int64_t n_rows,
                         int64_t n_blocks, int block_size, double *filter_state, int polyphony, double *scratch);

#ifdef __cplusplus
}
#endif
#endif /* PYGMU_HIP_H */
