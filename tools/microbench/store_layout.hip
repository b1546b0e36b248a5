// Write ceiling of the layouts a window-sized BiquadPE(SinePE) render can store in.  Pure-store kernels over a 536 MB
// buffer (134 M floats, beyond the 256 MB memory-side cache), HIP events over 100 launches after 30.  A 4 KB chunk is
// what one wave of the filter kernels stores per step: 64 lanes x 16 floats, as four 1 KB float4 rows (stage_store).
//   (a) the fused kernel's current layout: workgroup-contiguous 16 KB tiles, runs of 32 tiles, 1024 workgroups of
//       256 threads (768 resident: the last 256 run as a second round)
//   (b) wave-contiguous runs of 4 KB chunks, one resident round (3 or 4 waves per SIMD)
//   (c) (b) with odd run lengths, and with each wave's start rotated inside its run (staggered)
//   (d) (b) and (c) with __builtin_nontemporal_store
//   (e) (a) and (b) with write-through (sc1) stores: the line leaves L2 with the store, so the kernel ends with no dirty
//       lines for the end-of-kernel write-back
// Every layout is timed at n and at 2n frames (both beyond the cache, the same waves with runs twice as long): the
// per-launch fixed cost is 2 t(n) - t(2n), the rate n * 4 / (t(2n) - t(n)).
//   hipcc --offload-arch=gfx950 -O3 -o store_layout tools/microbench/store_layout.hip && ./store_layout
#include <hip/hip_runtime.h>
#include <cstdio>
#include <string>
typedef float v4f __attribute__((ext_vector_type(4)));

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
enum { PLAIN = 0, NT = 1, SC1 = 2 };

template <int KIND>
__device__ __forceinline__ void put(float *p, v4f v) {
    if (KIND == NT) __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(p));
    else *reinterpret_cast<v4f *>(p) = v;
}

// one 4 KB chunk of a wave: frames [c * 1024, c * 1024 + 1024), clipped to n
template <int KIND>
__device__ __forceinline__ void chunk(float *out, long n, long c, int lane, float v) {
    if (KIND == SC1) {
        // a buffer resource over the chunk's bytes inside [0, n): rows past the end are dropped by the bounds check
        const long left = n - c * 1024;
        if (left <= 0) return;
        const unsigned long p = (unsigned long)(out + c * 1024);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
        const int bytes = __builtin_amdgcn_readfirstlane((int)(left < 1024 ? left : 1024) * 4);
        __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long)hi << 32) | lo), 0, bytes, 0x00020000);
        const unsigned bits = __builtin_bit_cast(unsigned, v);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_buffer_store_b128(v4u{bits, bits, bits, bits}, rsrc, lane * 16, i * 1024, 16 /* sc1 */);
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long e = c * 1024 + i * 256 + lane * 4;
        if (e + 4 <= n) put<KIND>(out + e, v4f{v, v, v, v});
    }
}

// (a) workgroup g writes tiles [g * seg, g * seg + seg) of 4096 floats, wave w the w-th KB row group of each
template <int KIND>
__global__ void __launch_bounds__(256) store_wg_tiles(float *out, long n, int seg, float v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = 0; t < seg; ++t) {
        const long tile = (long)blockIdx.x * seg + t;
        chunk<KIND>(out, n, tile * 4 + wave, lane, v);
    }
}

// (b)-(d) wave g writes chunks [g * run, g * run + run) in order, starting `rot(g)` chunks into its run and wrapping
template <int KIND>
__global__ void __launch_bounds__(256) store_wave_runs(float *out, long n, int run, int stagger, float v) {
    const int lane = threadIdx.x & 63;
    const long g = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int rot = stagger ? (int)((g * stagger) % run) : 0;
    for (int k = 0; k < run; ++k) {
        int c = k + rot;
        if (c >= run) c -= run;
        chunk<KIND>(out, n, g * run + c, lane, v);
    }
}

template <typename F>
static float time_us(F launch) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    for (int i = 0; i < 30; ++i) launch();
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < 100; ++i) launch();
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return ms * 10.0f;
}

// launch(k): the layout over k * n frames, k = 1, 2
template <typename F>
static void timeit(const std::string &name, long bytes, F launch) {
    const float t1 = time_us([&] { launch(1); }), t2 = time_us([&] { launch(2); });
    printf("%-84s %8.2f us  %5.2f TB/s | 2n %8.2f us, fixed %6.2f us, rate %5.2f TB/s\n", name.c_str(), t1,
           bytes / (t1 * 1e-6) / 1e12, t2, 2 * t1 - t2, bytes / ((t2 - t1) * 1e-6) / 1e12);
}

int main() {
    const long n = 134000000, bytes = n * 4, chunks = (n + 1023) / 1024;
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    float *out;
    if (hipMalloc(&out, 2 * bytes) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
    timeit("hipMemsetAsync", bytes, [&](int k) { (void)hipMemsetAsync(out, 0, k * bytes, 0); });
    for (int kind : {PLAIN, SC1}) {
        const int seg = 32;
        const int groups = (int)((chunks / 4 + seg - 1) / seg);
        timeit(std::string(kind == SC1 ? "(e/a)" : "(a)") + " workgroup runs of 32 x 16 KB" + (kind == SC1 ? " sc1, " : ", ") +
                   std::to_string(groups) + " workgroups", bytes, [&](int k) {
                   const int gk = (int)((k * chunks / 4 + seg - 1) / seg);
                   if (kind == SC1) hipLaunchKernelGGL(store_wg_tiles<SC1>, dim3(gk), dim3(256), 0, 0, out, k * n, seg, 0.25f);
                   else hipLaunchKernelGGL(store_wg_tiles<PLAIN>, dim3(gk), dim3(256), 0, 0, out, k * n, seg, 0.25f);
               });
    }
    for (int per_simd : {3, 4}) {
        const long waves = (long)cus * 4 * per_simd;
        const int run = (int)((chunks + waves - 1) / waves);
        const int odd = run | 1;
        for (int kind : {PLAIN, NT, SC1}) {
            auto go = [&](const char *tag, int r, int stagger) {
                const unsigned groups = (unsigned)((chunks + 4L * r - 1) / (4L * r));
                const std::string name = std::string(tag) + (kind == NT ? " NT" : kind == SC1 ? " sc1" : "") + ", " +
                                         std::to_string(per_simd) + " waves/SIMD, runs of " + std::to_string(r) +
                                         " x 4 KB, " + std::to_string(groups) + " workgroups";
                timeit(name, bytes, [&](int k) {
                    if (kind == NT) hipLaunchKernelGGL(store_wave_runs<NT>, dim3(groups), dim3(256), 0, 0, out, k * n, k * r, stagger, 0.25f);
                    else if (kind == SC1) hipLaunchKernelGGL(store_wave_runs<SC1>, dim3(groups), dim3(256), 0, 0, out, k * n, k * r, stagger, 0.25f);
                    else hipLaunchKernelGGL(store_wave_runs<PLAIN>, dim3(groups), dim3(256), 0, 0, out, k * n, k * r, stagger, 0.25f);
                });
            };
            go(kind == NT ? "(d/b) wave runs" : kind == SC1 ? "(e/b) wave runs" : "(b) wave runs", run, 0);
            if (kind == SC1) continue;
            if (odd != run) go(kind == NT ? "(d/c) wave runs, odd length" : "(c) wave runs, odd length", odd, 0);
            go(kind == NT ? "(d/c) wave runs, odd length, staggered" : "(c) wave runs, odd length, staggered", odd, 7);
        }
    }
    (void)hipFree(out);
    return 0;
}
