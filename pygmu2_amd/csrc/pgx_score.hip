// pgx_score.hip -- the mix of a score: MixPE._render (mix_pe.py:69-96) over inputs that each occupy part of the block
// (sequence_pe.py builds such a MixPE; examples 19 and 29 build it by hand).
//
// The reference adds K full-length, mostly zero rows.  Adding a float32 zero changes nothing but the sign of a zero, so
// the sum over the segments that cover a frame, in input order, is the same sample.  The host cuts the block into tiles
// and lists per tile the segments that touch it, in input order (CSR: sum(len_i / tile + 2) entries).  One workgroup
// owns a tile; the walk over the tile's list is the same for every lane, so a descriptor is read once per wave through
// the scalar cache; each lane owns four elements of a 1024-element chunk and adds where the segment covers them.  Loads
// are one dword per lane, consecutive lanes on consecutive addresses: a segment starts at any frame, so wider loads
// would be unaligned.  Work and traffic are O(sum len_i + block + list), never K * block.

#include "pgx_common.h"

namespace {

constexpr int kScoreBlock = 256;
constexpr int kScorePer = 4;                                   // elements per lane and chunk
constexpr int kScoreChunk = kScoreBlock * kScorePer;

// A mix of at most kScoreInline segments carries them in its kernel arguments and every tile walks them all
// (k_score_mix_inline: tile_list == nullptr): a streamed block with a handful of sounding notes uploads nothing.
constexpr int kScoreInline = PGX_SCORE_INLINE;
struct ScoreInline {
    pgx_score_seg s[kScoreInline];
};

__device__ __forceinline__ void score_mix_body(float *out, int64_t frames, int channels, const pgx_score_seg *segs,
                                               int64_t n_segs, const int32_t *tile_offsets,
                                               const int32_t *tile_list, int64_t tile_frames) {
    const int64_t f0 = (int64_t)blockIdx.x * tile_frames;
    const int64_t f1 = (f0 + tile_frames < frames) ? f0 + tile_frames : frames;
    const int64_t e1 = f1 * channels;
    const int lo = tile_list ? tile_offsets[blockIdx.x] : 0;
    const int hi = tile_list ? tile_offsets[blockIdx.x + 1] : (int)n_segs;
    for (int64_t base = f0 * channels; base < e1; base += kScoreChunk) {
        float acc[kScorePer];
#pragma unroll
        for (int j = 0; j < kScorePer; ++j) acc[j] = 0.0f;
        const int64_t mine = base + threadIdx.x;
        for (int i = lo; i < hi; ++i) {
            const int64_t idx = tile_list ? tile_list[i] : i;
            if (idx < 0 || idx >= n_segs) continue;
            const pgx_score_seg s = segs[idx];
            const int64_t s0 = s.first * channels, s1 = s0 + s.frames * channels;
            if (s1 <= base || s0 >= base + kScoreChunk) continue;      // the same in every lane
#pragma unroll
            for (int j = 0; j < kScorePer; ++j) {
                const int64_t e = mine + (int64_t)j * kScoreBlock;
                if (e >= s0 && e < s1) acc[j] = acc[j] + s.data[e - s0];
            }
        }
#pragma unroll
        for (int j = 0; j < kScorePer; ++j) {
            const int64_t e = mine + (int64_t)j * kScoreBlock;
            if (e < e1) out[e] = acc[j];
        }
    }
}

__global__ void __launch_bounds__(kScoreBlock)
k_score_mix(float *out, int64_t frames, int channels, const pgx_score_seg *segs, int64_t n_segs,
            const int32_t *tile_offsets, const int32_t *tile_list, int64_t tile_frames) {
    score_mix_body(out, frames, channels, segs, n_segs, tile_offsets, tile_list, tile_frames);
}

__global__ void __launch_bounds__(kScoreBlock)
k_score_mix_inline(float *out, int64_t frames, int channels, ScoreInline segs, int n_segs, int64_t tile_frames) {
    score_mix_body(out, frames, channels, segs.s, n_segs, nullptr, nullptr, tile_frames);
}

}  // namespace

extern "C" {

int pgx_score_mix(float *out, int64_t frames, int channels, const pgx_score_seg *segs, int64_t n_segs,
                  const int32_t *tile_offsets, const int32_t *tile_list, int64_t tile_frames) {
    PGX_REQUIRE_INIT();
    if (frames <= 0) return PGX_OK;
    PGX_CHECK_ARG(out && channels >= 1 && n_segs >= 0 && tile_frames >= 1, "pgx_score_mix: bad argument");
    if (n_segs == 0) {
        PGX_HIP(hipMemsetAsync(out, 0, (size_t)frames * channels * sizeof(float), pgx::stream()));
        return PGX_OK;
    }
    const int64_t tiles = pgx::ceil_div(frames, tile_frames);
    PGX_CHECK_ARG(tiles < (int64_t)1 << 31, "pgx_score_mix: too many tiles");
    if (!tile_list) {
        PGX_CHECK_ARG(segs && n_segs <= kScoreInline, "pgx_score_mix: too many segments for a mix without tile lists");
        ScoreInline inl = {};
        for (int64_t i = 0; i < n_segs; ++i) inl.s[i] = segs[i];
        hipLaunchKernelGGL(k_score_mix_inline, dim3((unsigned)tiles), dim3(kScoreBlock), 0, pgx::stream(), out, frames,
                           channels, inl, (int)n_segs, tile_frames);
        PGX_LAUNCH_CHECK("k_score_mix_inline");
        return PGX_OK;
    }
    PGX_CHECK_ARG(segs && tile_offsets, "pgx_score_mix: null table");
    hipLaunchKernelGGL(k_score_mix, dim3((unsigned)tiles), dim3(kScoreBlock), 0, pgx::stream(), out, frames, channels,
                       segs, n_segs, tile_offsets, tile_list, tile_frames);
    PGX_LAUNCH_CHECK("k_score_mix");
    return PGX_OK;
}

}  // extern "C"
