// xv_subseg.hip -- sliding-window ("sub-segment") extraction: the packed batch rows of OVERLAPPING chunks.
//
// xv_cmn_sliding_scatter_f32 gives every raw frame one destination row; with one x-vector per 1.5 s window cut every 0.75 s a voiced
// frame belongs to window / period chunks.  xv_cmn_sliding_gather_f32 turns the indirection round: it is indexed by OUTPUT row.  For
// output row j of chunk c of utterance u
//     t = voiced_row[utt_start[u] + chunk_first[c] + j]                        (no VAD: t = chunk_first[c] + j)
//     y[(chunk_row[c] + j) ldy + f] = float(double(x[t][f]) - sum_{ws <= s < we} double(x[s][f]) / (we - ws))
// with the window [ws, we) of xv_frontend.hip over RAW frames (CMN comes before the selection).  It is the fp32, packed-row sibling
// of egs_chunks_kernel (xv_egs.hip): lanes = feature dimensions, one 32-lane group per (chunk, 64-output-row segment); the fp64
// window sum moves right by the gap to the previous voiced frame and restarts when the window has left the old one behind
// (cmn_window_move, xv_device.h).  A group's first row pays a full window of reads (all L2 hits: the neighbouring groups read the
// same frames) and a frame is normalised once per chunk it lies in; both are small next to the network that follows.
// A row is feat_dim contiguous floats (92 B of a 96-B batch row): one coalesced store per row; columns >= feat_dim and rows no chunk
// names are never written.  No atomics, one fixed order per output element: the same bits on every run.
#include "xv_device.h"

namespace {

constexpr int SEG = 64;            // output rows per lane group
constexpr int GROUPS = 8;          // lane groups (of 32) per 256-thread block

__global__ __launch_bounds__(256) void cmn_sliding_gather_kernel(const float *__restrict__ x, int ldx, int F, long x_rows,
                                                                 const int *__restrict__ utt_start, const int *__restrict__ utt_len,
                                                                 int n_utts, const int *__restrict__ voiced_count,
                                                                 const int *__restrict__ voiced_row, const int *__restrict__ chunk_utt,
                                                                 const int *__restrict__ chunk_first, const int *__restrict__ chunk_len,
                                                                 const int *__restrict__ chunk_row, int n_chunks, int segs_per_chunk,
                                                                 int window, int center, int min_window, float *__restrict__ y, int ldy,
                                                                 long y_rows)
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
    const int count = voiced_row ? min(voiced_count[u], T) : T;
    const long first = chunk_first[c];
    const long row0 = chunk_row[c];
    // output rows whose voiced index lies in [0, count) and whose batch row lies in [0, y_rows); the others are skipped
    const int j0 = (int)min(max(max((long)a, -first), -row0), (long)len);
    const int j1 = (int)min(min(min((long)a + SEG, (long)len), (long)count - first), y_rows - row0);
    if (j0 >= j1) return;
    const int f0 = threadIdx.x & 31;
    const int *rows = voiced_row ? voiced_row + base + first : nullptr;
    for (int f = f0; f < F; f += 32) {                 // F <= 32 in every recipe: one trip
        const float *col = x + base * ldx + f;
        int ws = 0, we = 0;
        double sum = 0.0;
        for (int j = j0; j < j1; ++j) {
            const int t = rows ? rows[j] : (int)(first + j);
            if (t < 0 || t >= T) continue;             // not an index compact() wrote: no read, no write
            int nws, nwe;
            cmn_window_bounds(t, T, window, center, min_window, nws, nwe);
            cmn_window_move(col, ldx, ws, we, nws, nwe, sum);
            y[(row0 + j) * ldy + f] = (float)((double)col[(long)t * ldx] - sum / (double)(we - ws));
        }
    }
}

}  // namespace

extern "C" int xv_cmn_sliding_gather_f32(const float *x, int ldx, int feat_dim, int64_t x_rows, const int32_t *utt_start,
                                         const int32_t *utt_len, int n_utts, const int32_t *voiced_count, const int32_t *voiced_row,
                                         const int32_t *chunk_utt, const int32_t *chunk_first, const int32_t *chunk_len,
                                         const int32_t *chunk_row, int n_chunks, int max_chunk_len, int cmn_window, int center,
                                         int min_window, float *y, int ldy, int64_t y_rows, void *stream)
{
    if (n_chunks == 0) return 0;
    if (!x || !utt_start || !utt_len || !chunk_utt || !chunk_first || !chunk_len || !chunk_row || !y || (!voiced_count != !voiced_row) ||
        n_chunks < 0 || n_utts < 0 || feat_dim <= 0 || ldx < feat_dim || ldy < feat_dim || x_rows < 0 || y_rows < 0 || cmn_window <= 0 ||
        min_window <= 0)
        return fail(XV_ERR_BAD_ARG, "cmn_sliding_gather: bad argument");
    if (max_chunk_len <= 0 || n_utts == 0 || x_rows == 0 || y_rows == 0) return 0;      // no row can be read or written
    const int spc = (max_chunk_len + SEG - 1) / SEG;
    const long groups = (long)n_chunks * spc;
    const long blocks = (groups + GROUPS - 1) / GROUPS;
    if (blocks > 0x7fffffffL) return fail(XV_ERR_UNSUPPORTED, "cmn_sliding_gather: too many chunks for one launch");
    hipLaunchKernelGGL(cmn_sliding_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, feat_dim,
                       (long)x_rows, utt_start, utt_len, n_utts, voiced_count, voiced_row, chunk_utt, chunk_first, chunk_len, chunk_row,
                       n_chunks, spc, cmn_window, center, min_window, y, ldy, (long)y_rows);
    return launch_status("cmn_sliding_gather_kernel");
}
