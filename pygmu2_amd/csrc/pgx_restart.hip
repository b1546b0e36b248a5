// pgx_restart.hip -- TriggerRestartPE / RandomSelectPE over sources whose samples depend on the frame index alone
// (pgx_restart_plan / pgx_restart_gather).
//
// The reference walks the trigger block on the host and renders the source once per event (trigger_restart_pe.py:72-98).
// Here a block is a scan plus a gather, the scheme of pgx_hold (pgx_control.hip):
//   * plan:   per segment of whole tiles the events' count, first index, last index and the longest gap between two
//             consecutive events inside the segment; a one-workgroup second launch folds the segments into the four
//             integers the host needs (count, first, last, longest stretch) -- 32 bytes, not the trigger block;
//   * gather: per tile an inclusive max-scan of event indices ("the last event <= t") and an inclusive count of events
//             ("which event that was"), carried in from the segments' partials; every frame then reads the take its
//             event's selection names at the local time t - last event.
// Integers only: the result does not depend on how the block is cut into workgroups.  float32 in, float32 out.
// An event is a sample > 0 (NaN and negatives are none, +2 is one).

#include "pgx_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kT = 8;                                   // frames per thread
constexpr int kTile = kBlock * kT;
constexpr int kMaxSeg = PGX_RESTART_MAX_SEGMENTS;
static_assert(kTile == PGX_RESTART_TILE, "PGX_RESTART_TILE");
constexpr long long kNone = 0x7fffffffffffffffLL;       // "no first event yet" under a min

__host__ __device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// segments of whole tiles, one workgroup each: a tile per segment until there are kMaxSeg of them
struct SegPlan {
    int64_t seg_frames;
    int nseg;
};
inline SegPlan seg_plan(int64_t n) {
    const int64_t tiles = pgx::ceil_div(n, kTile);
    const int64_t per = pgx::ceil_div(tiles, kMaxSeg);
    return SegPlan{per * kTile, (int)pgx::ceil_div(tiles, per)};
}

// workspace: four int64 per segment
enum { kCount = 0, kFirst = 1, kLast = 2, kGap = 3, kPerSeg = 4 };

// VEC: a mono trigger, 16-byte aligned -- a thread's 8 frames are two float4
template <bool VEC>
__device__ __forceinline__ void trig_load(float (&c)[kT], const float *trig, int stride, int64_t f0, int64_t end) {
    if (VEC && f0 + kT <= end) {
        const float4 a = *reinterpret_cast<const float4 *>(trig + f0);
        const float4 b = *reinterpret_cast<const float4 *>(trig + f0 + 4);
        c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w;
        c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < kT; ++j) c[j] = (f0 + j < end) ? trig[(f0 + j) * stride] : 0.0f;   // never an event
    }
}

// Over the workgroup, in thread order: the max of `last` and the sum of `count` over the threads BEFORE this one, folded
// onto the carried (carry_last, carry_count); the carries leave as the totals.  `lds`: 2 * kWaves values; two barriers.
__device__ __forceinline__ void block_scan(long long last, long long count, long long &carry_last, long long &carry_count,
                                           long long &before_last, long long &before_count, long long *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc_l = last, inc_c = count;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long ol = __shfl_up(inc_l, d, 64), oc = __shfl_up(inc_c, d, 64);
        if (lane >= d) {
            inc_l = ol > inc_l ? ol : inc_l;
            inc_c = inc_c + oc;
        }
    }
    if (lane == 63) {
        lds[wave] = inc_l;
        lds[kWaves + wave] = inc_c;
    }
    __syncthreads();
    long long bl = carry_last, bc = carry_count, tl = carry_last, tc = carry_count;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const long long wl = lds[w], wc = lds[kWaves + w];
        if (w < wave) {
            bl = wl > bl ? wl : bl;
            bc = bc + wc;
        }
        tl = wl > tl ? wl : tl;
        tc = tc + wc;
    }
    __syncthreads();
    long long el = __shfl_up(inc_l, 1, 64), ec = __shfl_up(inc_c, 1, 64);
    if (lane == 0) {
        el = -1;
        ec = 0;
    }
    before_last = el > bl ? el : bl;
    before_count = bc + ec;
    carry_last = tl;
    carry_count = tc;
}

// (sum of count, min of first, max of last, max of gap) over the workgroup, in every thread.  `lds`: 4 * kWaves values.
__device__ __forceinline__ void block_fold(long long &count, long long &first, long long &last, long long &gap,
                                           long long *lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long oc = __shfl_xor(count, d, 64), of = __shfl_xor(first, d, 64);
        const long long ol = __shfl_xor(last, d, 64), og = __shfl_xor(gap, d, 64);
        count = count + oc;
        first = of < first ? of : first;
        last = ol > last ? ol : last;
        gap = og > gap ? og : gap;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[wave] = count;
        lds[kWaves + wave] = first;
        lds[2 * kWaves + wave] = last;
        lds[3 * kWaves + wave] = gap;
    }
    __syncthreads();
    count = lds[0];
    first = lds[kWaves];
    last = lds[2 * kWaves];
    gap = lds[3 * kWaves];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
        count = count + lds[w];
        first = lds[kWaves + w] < first ? lds[kWaves + w] : first;
        last = lds[2 * kWaves + w] > last ? lds[2 * kWaves + w] : last;
        gap = lds[3 * kWaves + w] > gap ? lds[3 * kWaves + w] : gap;
    }
    __syncthreads();
}

// Pass 1 of the plan: one workgroup per segment -> partials[seg] = {count, first (n: none), last (-1: none), longest gap
// between consecutive events of the segment}.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_restart_reduce(long long *partials, const float *trig, int stride, int64_t n, int64_t seg_frames) {
    __shared__ long long lds[4 * kWaves];
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    long long count = 0, lo = kNone, gap = 0;
    long long carry_last = -1, carry_count = 0;           // over the tiles of this segment
    for (int64_t base = first; base < end; base += kTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kT;
        float c[kT];
        trig_load<VEC>(c, trig, stride, f0, end);
        long long run = -1, mine = -1, cnt = 0;
#pragma unroll
        for (int j = 0; j < kT; ++j) {
            if (c[j] > 0.0f) {
                const long long at = f0 + j;
                if (run >= 0) gap = (at - run) > gap ? (at - run) : gap;
                else mine = at;
                run = at;
                ++cnt;
            }
        }
        long long before_last, before_count;
        block_scan(run, cnt, carry_last, carry_count, before_last, before_count, lds);
        if (mine >= 0) {
            if (before_last >= 0) gap = (mine - before_last) > gap ? (mine - before_last) : gap;
            lo = mine < lo ? mine : lo;
        }
        count = count + cnt;
    }
    long long last = carry_last;                          // the same in every thread
    block_fold(count, lo, last, gap, lds);
    if (threadIdx.x == 0) {
        long long *p = partials + (int64_t)blockIdx.x * kPerSeg;
        p[kCount] = count;
        p[kFirst] = lo == kNone ? (long long)n : lo;
        p[kLast] = last;
        p[kGap] = gap;
    }
}

// Pass 2 of the plan: one workgroup folds the segments, a run of them per thread, in order.
// summary = {count, first (n: none), last (-1: none), the longest stretch [event, next event or n), 0: none}.
__global__ void __launch_bounds__(kBlock)
k_restart_combine(long long *summary, const long long *partials, int nseg, int64_t n) {
    __shared__ long long lds[4 * kWaves];
    const int per = (nseg + kBlock - 1) / kBlock;
    const int s0 = (int)threadIdx.x * per, s1 = (s0 + per < nseg) ? s0 + per : nseg;
    long long count = 0, lo = kNone, last = -1, gap = 0;
    for (int s = s0; s < s1; ++s) {
        const long long *p = partials + (int64_t)s * kPerSeg;
        const long long c = p[kCount];
        if (c == 0) continue;
        if (last >= 0) gap = (p[kFirst] - last) > gap ? (p[kFirst] - last) : gap;
        else lo = p[kFirst];
        gap = p[kGap] > gap ? p[kGap] : gap;
        last = p[kLast];
        count = count + c;
    }
    long long carry_last = -1, carry_count = 0, before_last, before_count;
    block_scan(last, count, carry_last, carry_count, before_last, before_count, lds);
    if (count > 0 && before_last >= 0) gap = (lo - before_last) > gap ? (lo - before_last) : gap;
    block_fold(count, lo, last, gap, lds);
    if (threadIdx.x == 0) {
        if (last >= 0) gap = ((long long)n - last) > gap ? ((long long)n - last) : gap;
        summary[0] = count;
        summary[1] = lo == kNone ? (long long)n : lo;
        summary[2] = last;
        summary[3] = gap;
    }
}

// The gather.  ordinal = events at positions <= t; local = t - the last of them, or carry_local + t before the first;
// slot = sel[ordinal] (sel[0]: the take of the stretch that runs in from the previous block).  A frame is silent when
// nothing has ever started (carry_local < 0 before the first event), when its slot is none (< 0, or no entry of sel /
// takes) and where its local time lies outside the take.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_restart_gather(float *out, int64_t n, int channels, const float *trig, int stride, const long long *partials,
                 int64_t seg_frames, long long carry_local, const int32_t *sel, int64_t n_sel, const pgx_restart_take *takes,
                 int n_takes) {
    __shared__ long long lds[4 * kWaves];
    long long carry_last = -1, carry_count = 0, unused = kNone, unused2 = 0;
    for (int s = threadIdx.x; s < (int)blockIdx.x; s += kBlock) {
        const long long *p = partials + (int64_t)s * kPerSeg;
        carry_last = p[kLast] > carry_last ? p[kLast] : carry_last;
        carry_count = carry_count + p[kCount];
    }
    if (gridDim.x > 1) block_fold(carry_count, unused, carry_last, unused2, lds);
    const int64_t first = (int64_t)blockIdx.x * seg_frames;
    const int64_t end = first + seg_frames < n ? first + seg_frames : n;
    for (int64_t base = first; base < end; base += kTile) {
        const int64_t f0 = base + (int64_t)threadIdx.x * kT;
        float c[kT];
        trig_load<VEC>(c, trig, stride, f0, end);
        long long loc[kT];
        int ord[kT];
        long long run = -1;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kT; ++j) {
            if (c[j] > 0.0f) {
                run = f0 + j;
                ++cnt;
            }
            loc[j] = run;
            ord[j] = cnt;
        }
        long long before_last, before_count;
        block_scan(run, cnt, carry_last, carry_count, before_last, before_count, lds);
        float y[kT];
        const bool mono = channels == 1;
#pragma unroll
        for (int j = 0; j < kT; ++j) {
            const int64_t t = f0 + j;
            if (t >= end) break;
            const long long at = loc[j] > before_last ? loc[j] : before_last;
            const long long ordinal = before_count + ord[j];
            const long long local = ordinal == 0 ? carry_local + t : t - at;
            const float *src = nullptr;
            if ((ordinal > 0 || carry_local >= 0) && ordinal < n_sel) {
                const int slot = sel[ordinal];
                if (slot >= 0 && slot < n_takes) {
                    const pgx_restart_take take = takes[slot];
                    const long long rel = local - take.first;
                    if (rel >= 0 && rel < take.len) src = take.ptr + rel * channels;
                }
            }
            if (mono) {
                y[j] = src ? src[0] : 0.0f;
            } else {
                float *dst = out + t * channels;
                for (int ch = 0; ch < channels; ++ch) dst[ch] = src ? src[ch] : 0.0f;
            }
        }
        if (mono) {
            if (VEC && f0 + kT <= end) {
                *reinterpret_cast<float4 *>(out + f0) = make_float4(y[0], y[1], y[2], y[3]);
                *reinterpret_cast<float4 *>(out + f0 + 4) = make_float4(y[4], y[5], y[6], y[7]);
            } else {
#pragma unroll
                for (int j = 0; j < kT; ++j)
                    if (f0 + j < end) out[f0 + j] = y[j];
            }
        }
    }
}

}  // namespace

extern "C" {

int pgx_restart_plan(int64_t *summary_dev, void *workspace, const float *trigger, int trigger_stride, int64_t n) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(summary_dev && workspace && trigger && trigger_stride >= 1 && n >= 1, "pgx_restart_plan: bad argument");
    const SegPlan p = seg_plan(n);
    long long *partials = static_cast<long long *>(workspace);
    if (trigger_stride == 1 && aligned16(trigger))
        hipLaunchKernelGGL(k_restart_reduce<true>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), partials, trigger,
                           trigger_stride, n, p.seg_frames);
    else
        hipLaunchKernelGGL(k_restart_reduce<false>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), partials, trigger,
                           trigger_stride, n, p.seg_frames);
    PGX_LAUNCH_CHECK("k_restart_reduce");
    hipLaunchKernelGGL(k_restart_combine, dim3(1), dim3(kBlock), 0, pgx::stream(),
                       reinterpret_cast<long long *>(summary_dev), (const long long *)partials, p.nseg, n);
    PGX_LAUNCH_CHECK("k_restart_combine");
    return PGX_OK;
}

int pgx_restart_gather(float *out, int64_t n, int channels, const float *trigger, int trigger_stride,
                       const void *workspace, int64_t carry_local, const int32_t *sel_dev, int64_t n_sel,
                       const pgx_restart_take *takes_dev, int n_takes) {
    PGX_REQUIRE_INIT();
    PGX_CHECK_ARG(out && workspace && trigger && sel_dev && trigger_stride >= 1 && n >= 1 && channels >= 1 &&
                      n_sel >= 1 && n_takes >= 0 && (takes_dev || n_takes == 0), "pgx_restart_gather: bad argument");
    const SegPlan p = seg_plan(n);
    const long long *partials = static_cast<const long long *>(workspace);
    // the vector form also stores a mono output as float4; with more channels only the trigger loads are vectors
    const bool vec = trigger_stride == 1 && aligned16(trigger) && (channels > 1 || aligned16(out));
    if (vec)
        hipLaunchKernelGGL(k_restart_gather<true>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), out, n, channels, trigger,
                           trigger_stride, partials, p.seg_frames, (long long)carry_local, sel_dev, n_sel, takes_dev,
                           n_takes);
    else
        hipLaunchKernelGGL(k_restart_gather<false>, dim3(p.nseg), dim3(kBlock), 0, pgx::stream(), out, n, channels,
                           trigger, trigger_stride, partials, p.seg_frames, (long long)carry_local, sel_dev, n_sel,
                           takes_dev, n_takes);
    PGX_LAUNCH_CHECK("k_restart_gather");
    return PGX_OK;
}

}  // extern "C"
