// xv_segment.hip -- speech segments from VAD decisions that lie in device memory.
//
// The rule (this project's own; include/xvector_hip.h states it in full): per utterance of T frames, a frame is voiced iff
// vad != 0; (1) an inner unvoiced run of at most max_gap frames is closed, (2) voiced runs shorter than min_len are dropped, (3) a
// kept run [a, b) is padded to [max(a - pad, 0), min(b + pad, T)), (4) a run of n > max_len frames is split into k = ceil(n / max_len)
// pieces [a + floor(i n / k), a + floor((i + 1) n / k)).  The segments are the pieces in increasing order.
//
// Restated over voiced frames only, every decision looks BACKWARDS: with p(t) the last voiced frame before a voiced frame t, t
// opens a run iff there is no p(t) or t - p(t) - 1 > max_gap, and then the run before it is complete: it is [s, p(t) + 1) with s
// the last opening frame before t.  The last run of an utterance is completed by its end.  So one workgroup walks its utterance in
// tiles of TILE frames (one frame per thread, the next tile's decisions already in flight) and carries three integers across
// tiles: the last voiced frame, the opening frame of the run that is open, and the number of pieces written so far.  Inside a tile
//     p(t), s(t)   are "the highest flagged lane below mine": a ballot and a count of leading zeros per wave, the waves joined
//                  through LDS (a wave that has no flagged lane below takes the last flagged frame of the waves before, else the
//                  carry);
//     the index of a completed run's first piece is the carry plus the exclusive prefix sum of the piece counts of the runs
//                  completed before it in the tile (a shuffle scan per wave, wave totals through LDS).
// The thread of the opening frame writes the pieces of the run it completes (a run that spans many tiles is still written by one
// thread: its pieces are few, n / max_len).  Gaps, runs and pieces that straddle tiles differ from those inside one only in where
// p and s come from.  Integers only, no atomics, one fixed order: the same bits on every run.  No workspace is needed:
// xv_vad_segments_workspace_bytes is 0 and the workspace arguments are there for a scan-based implementation to use.
#include "xv_device.h"

namespace {

constexpr int TILE = XV_SEG_TILE;          // frames per step = threads per workgroup
constexpr int NW = TILE / 64;

struct SegParams {
    int gap, min_len, pad, max_len;
};

// pieces of the completed run of voiced frames [a, b) in an utterance of T frames: (first frame, length, count) after drop and pad
__device__ __forceinline__ int run_pieces(int a, int b, int T, const SegParams &q, int &first, int &n)
{
    if (b - a < q.min_len) return 0;
    first = max(a - q.pad, 0);
    n = (int)min((long)b + q.pad, (long)T) - first;
    return q.max_len > 0 && n > q.max_len ? (n + q.max_len - 1) / q.max_len : 1;
}

// piece i of k of the run (first, n) goes to entry idx of utterance u's table, while it fits the caller's capacity
__device__ __forceinline__ void write_pieces(int first, int n, int k, long idx, long off, int cap, long n_slots,
                                             int *__restrict__ seg_first, int *__restrict__ seg_len)
{
    const long fit = min((long)k, (long)cap - idx);          // entries idx + i < cap
    for (long i = 0; i < fit; ++i) {
        const long slot = off + idx + i;
        if (slot < 0 || slot >= n_slots) continue;
        const int lo = (int)(i * n / k), hi = (int)((i + 1) * n / k);
        seg_first[slot] = first + lo;
        seg_len[slot] = hi - lo;
    }
}

// the highest lane below `lane` whose flag is set, or -1; `all`: the wave's ballot of the flag
__device__ __forceinline__ int flagged_below(unsigned long long all, int lane)
{
    const unsigned long long m = all & ((1ull << lane) - 1ull);
    return m ? 63 - __clzll(m) : -1;
}

__global__ __launch_bounds__(TILE) void vad_segments_kernel(const float *__restrict__ vad, const int *__restrict__ utt_start,
                                                            const int *__restrict__ utt_len, long n_frames, SegParams q,
                                                            const int *__restrict__ seg_off, const int *__restrict__ seg_cap,
                                                            long n_slots, int *__restrict__ seg_count, int *__restrict__ seg_first,
                                                            int *__restrict__ seg_len)
{
    __shared__ int s_voiced[NW], s_open[NW], s_total[NW];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long base = utt_start[u];
    const int T = utt_len[u];
    if (base < 0 || T <= 0 || base + (long)T > n_frames) {      // no frame, or a span outside the buffer: nothing is read
        if (tid == 0) seg_count[u] = 0;
        return;
    }
    const long off = seg_off[u];
    const int cap = seg_cap[u];
    int last_voiced = -1, open_at = -1;          // carried across tiles: the last voiced frame, the opening frame of the open run
    long written = 0;                            // ... and the pieces of the runs completed so far
    bool v_next = tid < T && vad[base + tid] != 0.0f;
    for (long t0 = 0; t0 < T; t0 += TILE) {
        const int t = (int)min(t0 + tid, (long)T);         // (a thread past the end holds no voiced frame: its t is not used)
        const bool v = v_next;
        const long tn = t0 + TILE + tid;
        v_next = tn < T && vad[base + tn] != 0.0f;
        // p: the last voiced frame before t
        const unsigned long long mv = __ballot(v);
        if (lane == 0) s_voiced[w] = mv ? (int)t0 + 64 * w + 63 - __clzll(mv) : -1;
        __syncthreads();
        int before = last_voiced, tile_last = last_voiced;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int x = s_voiced[k];
            if (x >= 0) {
                tile_last = x;
                if (k < w) before = x;
            }
        }
        const int jb = flagged_below(mv, lane);
        const int p = jb >= 0 ? (int)t0 + 64 * w + jb : before;
        const bool opens = v && (p < 0 || t - p - 1 > q.gap);
        // s: the opening frame of the run that ends at p
        const unsigned long long mo = __ballot(opens);
        if (lane == 0) s_open[w] = mo ? (int)t0 + 64 * w + 63 - __clzll(mo) : -1;
        __syncthreads();
        int open_before = open_at, tile_open = open_at;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int x = s_open[k];
            if (x >= 0) {
                tile_open = x;
                if (k < w) open_before = x;
            }
        }
        const int jo = flagged_below(mo, lane);
        const int s = jo >= 0 ? (int)t0 + 64 * w + jo : open_before;
        // the run [s, p + 1) is complete at an opening frame that has a voiced frame before it
        int first = 0, n = 0, k = 0;
        if (opens && p >= 0) k = run_pieces(s, p + 1, T, q, first, n);
        int incl = k;                            // inclusive prefix sum of k over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63) s_total[w] = incl;
        __syncthreads();
        long idx = written + incl - k, tile_total = 0;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int x = s_total[j];
            tile_total += x;
            if (j < w) idx += x;
        }
        if (k > 0) write_pieces(first, n, k, idx, off, cap, n_slots, seg_first, seg_len);
        last_voiced = tile_last;
        open_at = tile_open;
        written += tile_total;
        // (s_voiced is next written behind the third barrier of this tile and was last read before the second; s_open and s_total
        // are next written behind the first and second barriers of the next tile: no array is rewritten while a wave may read it)
    }
    if (tid == 0) {
        if (last_voiced >= 0) {                  // the end of the utterance completes the open run
            int first = 0, n = 0;
            const int k = run_pieces(open_at, last_voiced + 1, T, q, first, n);
            write_pieces(first, n, k, written, off, cap, n_slots, seg_first, seg_len);
            written += k;
        }
        seg_count[u] = (int)written;
    }
}

bool params_ok(int max_gap, int min_len, int pad, int max_len)
{
    return max_gap >= 0 && min_len >= 1 && pad >= 0 && 2L * pad <= max_gap && (max_len == 0 || (max_len > 0 && max_len >= 2L * min_len));
}

}  // namespace

extern "C" size_t xv_vad_segments_workspace_bytes(int64_t n_frames)
{
    (void)n_frames;
    return 0;
}

extern "C" int64_t xv_vad_segments_capacity(int64_t T, int max_gap, int min_len, int max_len)
{
    if (T < 0 || !params_ok(max_gap, min_len, 0, max_len)) return -1;
    return (T + max_gap + 1) / ((int64_t)min_len + max_gap + 1) + (max_len ? T / max_len : 0);
}

extern "C" int xv_vad_segments_i32(const float *vad, const int32_t *utt_start, const int32_t *utt_len, int n_utts, int64_t n_frames,
                                   int max_gap, int min_len, int pad, int max_len, const int32_t *seg_off, const int32_t *seg_cap,
                                   int64_t n_slots, int32_t *seg_count, int32_t *seg_first, int32_t *seg_len, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    if (n_utts < 0 || n_frames < 0 || n_slots < 0 || !params_ok(max_gap, min_len, pad, max_len) || !vad || !utt_start || !utt_len ||
        !seg_off || !seg_cap || !seg_count || !seg_first || !seg_len ||
        workspace_bytes < xv_vad_segments_workspace_bytes(n_frames) || (workspace_bytes > 0 && !workspace))
        return fail(XV_ERR_BAD_ARG, "vad_segments: bad argument");
    if (n_utts == 0) return 0;
    const SegParams q = {max_gap, min_len, pad, max_len};
    hipLaunchKernelGGL(vad_segments_kernel, dim3((unsigned)n_utts), dim3(TILE), 0, (hipStream_t)stream, vad, utt_start, utt_len,
                       (long)n_frames, q, seg_off, seg_cap, (long)n_slots, seg_count, seg_first, seg_len);
    return launch_status("vad_segments_kernel");
}
