// xv_rowplan.hip -- the destination-row plan of the extractor's CMN + VAD mode, made on the MI355X.
//
// Extractor.submit_raw (xvector_amd/engine.py) walks every frame of a window on the host (xv_raw_row_plan of xv_host.cpp) to tell
// xv_cmn_sliding_scatter_f32 where each raw frame goes in the packed batch.  When the MFCC rows and the VAD decisions were made on
// this card (Mfcc.compute_device) they never leave it, and the plan is made here from them:
//     xv_voiced_rank_i32      once per window: rank[p] = number of voiced frames of its utterance before frame p (-1: unvoiced),
//                             voiced_count[u] = what the host needs to plan the window's chunks (4 bytes per utterance come down);
//     xv_chunk_row_plan_i32   once per batch: dst_row[p] from rank[p] and the per-utterance chunk tables, the arithmetic of
//                             xv_raw_row_plan (chunk k = rank / size, row r = rank % size) without its running counters.
//
// Both are integer-only and use no atomics: one fixed order, the same bits on every run.  One wave per utterance, as
// xv_vad_compact_i32: a wave walks its utterance TILE frames at a time (UNROLL independent 64-frame loads in flight), a frame's rank
// is the count carried from the tiles before plus the voiced lanes below it (ballot + popcount over the 64 lanes of the wave).
#include "xv_device.h"

namespace {

constexpr int WAVES = 4;           // utterances per 256-thread block
constexpr int UNROLL = 4;          // 64-frame steps whose loads are issued together
constexpr int TILE = 64 * UNROLL;

// the span of utterance u, or false when it leaves [0, n_frames) (nothing is read or written for such an utterance)
__device__ __forceinline__ bool span_of(const int *utt_start, const int *utt_len, int u, long n_frames, long &base, int &T)
{
    base = utt_start[u];
    T = utt_len[u];
    return base >= 0 && T >= 0 && base + (long)T <= n_frames;
}

__global__ __launch_bounds__(256) void voiced_rank_kernel(const float *__restrict__ vad, const int *__restrict__ utt_start,
                                                          const int *__restrict__ utt_len, int n_utts, long n_frames,
                                                          int *__restrict__ rank, int *__restrict__ voiced_count)
{
    const int u = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (u >= n_utts) return;
    const int lane = threadIdx.x & 63;
    long base;
    int T;
    if (!span_of(utt_start, utt_len, u, n_frames, base, T)) {
        if (lane == 0) voiced_count[u] = 0;
        return;
    }
    if (!vad) {                                              // every frame is voiced
        for (int t = lane; t < T; t += 64) rank[base + t] = t;
        if (lane == 0) voiced_count[u] = T;
        return;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    int count = 0;                                           // voiced frames of the tiles before this one: carried across tiles
    for (int t0 = 0; t0 < T; t0 += TILE) {
        bool v[UNROLL];
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const int t = t0 + 64 * k + lane;
            v[k] = t < T && vad[base + t] != 0.0f;
        }
#pragma unroll
        for (int k = 0; k < UNROLL; ++k) {
            const int t = t0 + 64 * k + lane;
            const unsigned long long m = __ballot(v[k]);
            if (t < T) rank[base + t] = v[k] ? count + __popcll(m & below) : -1;
            count += __popcll(m);
        }
    }
    if (lane == 0) voiced_count[u] = count;
}

__global__ __launch_bounds__(256) void chunk_row_plan_kernel(const int *__restrict__ rank, const int *__restrict__ utt_start,
                                                             const int *__restrict__ utt_len, const int *__restrict__ chunk_size,
                                                             const int *__restrict__ chunks_kept, const int *__restrict__ first_chunk,
                                                             int n_utts, long n_frames, int b0, int b1,
                                                             const int *__restrict__ row_start, int *__restrict__ dst_row)
{
    const int u = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (u >= n_utts) return;
    const int lane = threadIdx.x & 63;
    long base;
    int T;
    if (!span_of(utt_start, utt_len, u, n_frames, base, T)) return;
    const int size = chunk_size[u];
    const int kept = size > 0 ? chunks_kept[u] : 0;
    const long first = first_chunk[u];
    for (int t = lane; t < T; t += 64) {
        const int v = rank[base + t];
        int dst = -1;
        if (v >= 0 && size > 0) {
            const int k = v / size;
            const long cid = first + k;
            // cid - b0 lies in [0, b1 - b0): the entries of row_start the caller brought for this batch
            if (k < kept && cid >= b0 && cid < b1) dst = row_start[cid - b0] + (v - k * size);
        }
        dst_row[base + t] = dst;
    }
}

}  // namespace

extern "C" int xv_voiced_rank_i32(const float *vad, const int32_t *utt_start, const int32_t *utt_len, int n_utts, int64_t n_frames,
                                  int32_t *rank, int32_t *voiced_count, void *stream)
{
    if (n_utts < 0 || n_frames < 0 || !rank || !voiced_count) return fail(XV_ERR_BAD_ARG, "voiced_rank: bad argument");
    if (n_utts == 0) return 0;
    if (!utt_start || !utt_len) return fail(XV_ERR_BAD_ARG, "voiced_rank: bad argument");
    hipLaunchKernelGGL(voiced_rank_kernel, dim3((n_utts + WAVES - 1) / WAVES), dim3(256), 0, (hipStream_t)stream, vad, utt_start,
                       utt_len, n_utts, (long)n_frames, rank, voiced_count);
    return launch_status("voiced_rank_kernel");
}

extern "C" int xv_chunk_row_plan_i32(const int32_t *rank, const int32_t *utt_start, const int32_t *utt_len, const int32_t *chunk_size,
                                     const int32_t *chunks_kept, const int32_t *first_chunk, int n_utts, int64_t n_frames, int32_t b0,
                                     int32_t b1, const int32_t *row_start, int32_t *dst_row, void *stream)
{
    if (n_utts < 0 || n_frames < 0 || !dst_row) return fail(XV_ERR_BAD_ARG, "chunk_row_plan: bad argument");
    if (n_utts == 0) return 0;
    if (!rank || !utt_start || !utt_len || !chunk_size || !chunks_kept || !first_chunk || (b1 > b0 && !row_start))
        return fail(XV_ERR_BAD_ARG, "chunk_row_plan: bad argument");
    hipLaunchKernelGGL(chunk_row_plan_kernel, dim3((n_utts + WAVES - 1) / WAVES), dim3(256), 0, (hipStream_t)stream, rank, utt_start,
                       utt_len, chunk_size, chunks_kept, first_chunk, n_utts, (long)n_frames, (int)b0, (int)b1, row_start, dst_row);
    return launch_status("chunk_row_plan_kernel");
}
