// xv_egs.hip -- training examples ("egs") cut on the MI355X: stages 3-5 of the recipe for the part that scales with the data.
//
// The reference writes a second copy of all features (run.sh stage 3: apply-cmvn-sliding | select-voiced-frames | copy-feats) and
// create_tar_files.py then cuts float16 chunks out of that copy, addressed in VOICED-frame numbering by a ranges file.  Here
//     xv_vad_compact_i32   builds, per utterance, the list of its voiced frames (voiced_row[utt_start[u] + j] = raw frame of the j-th
//                          voiced frame, voiced_count[u] = their number = utt2num_frames of the *_no_sil set), and
//     xv_egs_chunks_f16    goes from the RAW rows straight to the packed [B, T, F] float16 members: for output row j of chunk c
//                              t = voiced_row[utt_start[u] + chunk_first[c] + j]
//                              y[chunk_dst[c] + j F + f] = half_rne(float(double(x[t][f]) - sum_{ws <= s < we} double(x[s][f]) / (we - ws)))
//                          with the window [ws, we) of xv_frontend.hip over RAW frames (CMN comes before the selection in the
//                          reference).  No fp32 no-sil copy exists at any point; only frames that land in a chunk are normalised.
//
// xv_vad_compact_i32: one wave per utterance walks it 64 frames at a time; a frame's rank among the voiced ones is the running count
// plus the number of voiced lanes below it (ballot + popcount).  No atomics, one fixed order: the same bits on every run.
//
// xv_egs_chunks_f16: lanes = feature dimensions and one 32-lane group per (chunk, 64-output-row segment), as in xv_frontend.hip.  The
// fp64 window sum slides from one output row to the next; consecutive voiced frames lie one or more raw frames apart, so the window
// moves right by that gap (a gap as long as the window restarts the sum).  The stores: a row is feat_dim contiguous halves and the
// rows of a chunk lie back to back, so a group writes one contiguous run of (rows F) halves, row by row, one 2-byte store per lane --
// rows of 23 halves start on odd half-words every other row, so no wider store is aligned for every row, and pairing lanes into
// dword stores would not lower the instruction count (one store instruction per row either way).  The partial 128-byte lines of
// neighbouring rows merge in the write-back L2 before they leave for HBM; the kernel's time is the window reads, not the stores.
#include "xv_device.h"

#include <hip/hip_fp16.h>

namespace {

constexpr int SEG = 64;            // output rows per lane group
constexpr int GROUPS = 8;          // lane groups (of 32) per 256-thread block
constexpr int WAVES = 4;           // utterances per 256-thread block of the compaction

__global__ __launch_bounds__(256) void vad_compact_kernel(const float *__restrict__ vad, const int *__restrict__ utt_start,
                                                          const int *__restrict__ utt_len, int n_utts, long n_frames,
                                                          int *__restrict__ voiced_count, int *__restrict__ voiced_row)
{
    const int u = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (u >= n_utts) return;
    const int lane = threadIdx.x & 63;
    const long base = utt_start[u];
    const int T = utt_len[u];
    if (base < 0 || T < 0 || base + T > n_frames) {          // a span outside the buffers: nothing is read or written for it
        if (lane == 0) voiced_count[u] = 0;
        return;
    }
    int count = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const bool v = t < T && vad[base + t] != 0.0f;
        const unsigned long long m = __ballot(v);
        if (v) voiced_row[base + count + __popcll(m & ((1ull << lane) - 1ull))] = t;
        count += __popcll(m);
    }
    if (lane == 0) voiced_count[u] = count;
}

__global__ __launch_bounds__(256) void egs_chunks_kernel(const float *__restrict__ x, int ldx, int F, long x_rows,
                                                         const int *__restrict__ utt_start, const int *__restrict__ utt_len, int n_utts,
                                                         const int *__restrict__ voiced_count, const int *__restrict__ voiced_row,
                                                         const int *__restrict__ chunk_utt, const int *__restrict__ chunk_first,
                                                         const int *__restrict__ chunk_len, const long *__restrict__ chunk_dst,
                                                         int n_chunks, int segs_per_chunk, int window, int center, int min_window,
                                                         __half *__restrict__ y, long y_elems)
{
    const long g = (long)blockIdx.x * GROUPS + (threadIdx.x >> 5);
    const long c = g / segs_per_chunk;
    if (c >= n_chunks) return;
    const int a = (int)(g % segs_per_chunk) * SEG;
    const int len = chunk_len[c];
    if (a >= len) return;
    const int u = chunk_utt[c];
    if (u < 0 || u >= n_utts) return;
    const long base = utt_start[u];
    const int T = utt_len[u];
    if (base < 0 || T <= 0 || base + T > x_rows) return;
    const int count = min(voiced_count[u], T);
    const long first = chunk_first[c];
    const long dst = chunk_dst[c];
    // output rows whose voiced index lies in [0, count) and whose halves lie inside y; the others are skipped
    const int j0 = (int)min(max((long)a, -first), (long)len);
    int j1 = (int)min((long)min(a + SEG, len), (long)count - first);
    if (dst < 0) return;
    if (dst + (long)j1 * F > y_elems) j1 = (int)min((long)j1, (y_elems - dst) / F);
    if (j0 >= j1) return;
    const int f0 = threadIdx.x & 31;
    auto bounds = [&](int t, int &ws, int &we) { cmn_window_bounds(t, T, window, center, min_window, ws, we); };
    const int *rows = voiced_row + base + first;
    for (int f = f0; f < F; f += 32) {                 // F <= 32 in every recipe: one trip
        const float *col = x + base * ldx + f;
        int ws = 0, we = 0;
        double sum = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int t = rows[j];
            if (t < 0 || t >= T) continue;             // not an index compact() wrote: no read, no write
            int nws, nwe;
            bounds(t, nws, nwe);
            // voiced frames ascend, so the window only moves right: by the gap to the previous voiced frame.  A window that has left
            // the old one behind (or an index list that does not ascend) starts its sum afresh.
            cmn_window_move(col, ldx, ws, we, nws, nwe, sum);
            float v = (float)((double)col[(long)t * ldx] - sum / (double)(we - ws));
            // Two roundings, as the reference's float32 features cast with astype(float16): the compiler would otherwise fold
            // double -> float -> half into ONE rounding from the double (seen in the ISA: a software f64 -> f16 sequence), which
            // differs where the float lands on a half tie.  The empty statement makes the float opaque; it emits nothing.
            asm volatile("" : "+v"(v));
            y[dst + (long)j * F + f] = __float2half_rn(v);
        }
    }
}

}  // namespace

extern "C" int xv_vad_compact_i32(const float *vad, const int32_t *utt_start, const int32_t *utt_len, int n_utts, int64_t n_frames,
                                  int32_t *voiced_count, int32_t *voiced_row, void *stream)
{
    if (n_utts <= 0) return 0;
    if (!utt_start || !utt_len || !voiced_count || n_frames < 0 || (n_frames > 0 && (!vad || !voiced_row)))
        return fail(XV_ERR_BAD_ARG, "vad_compact: bad argument");
    hipLaunchKernelGGL(vad_compact_kernel, dim3((n_utts + WAVES - 1) / WAVES), dim3(256), 0, (hipStream_t)stream, vad, utt_start,
                       utt_len, n_utts, (long)n_frames, voiced_count, voiced_row);
    return launch_status("vad_compact_kernel");
}

extern "C" int xv_egs_chunks_f16(const float *x, int ldx, int feat_dim, int64_t x_rows, const int32_t *utt_start,
                                 const int32_t *utt_len, int n_utts, const int32_t *voiced_count, const int32_t *voiced_row,
                                 const int32_t *chunk_utt, const int32_t *chunk_first, const int32_t *chunk_len,
                                 const int64_t *chunk_dst, int n_chunks, int max_chunk_len, int cmn_window, int center, int min_window,
                                 void *y, int64_t y_elems, void *stream)
{
    if (n_chunks <= 0 || max_chunk_len <= 0 || n_utts <= 0) return 0;
    if (!x || !utt_start || !utt_len || !voiced_count || !voiced_row || !chunk_utt || !chunk_first || !chunk_len || !chunk_dst || !y ||
        feat_dim <= 0 || ldx < feat_dim || x_rows <= 0 || y_elems <= 0 || cmn_window <= 0 || min_window <= 0)
        return fail(XV_ERR_BAD_ARG, "egs_chunks: bad argument");
    const int spc = (max_chunk_len + SEG - 1) / SEG;
    const long groups = (long)n_chunks * spc;
    const long blocks = (groups + GROUPS - 1) / GROUPS;
    if (blocks > 0x7fffffffL) return fail(XV_ERR_UNSUPPORTED, "egs_chunks: too many chunks for one launch");
    hipLaunchKernelGGL(egs_chunks_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, feat_dim, (long)x_rows,
                       utt_start, utt_len, n_utts, voiced_count, voiced_row, chunk_utt, chunk_first, chunk_len,
                       (const long *)chunk_dst, n_chunks, spc, cmn_window, center, min_window, (__half *)y, (long)y_elems);
    return launch_status("egs_chunks_kernel");
}
