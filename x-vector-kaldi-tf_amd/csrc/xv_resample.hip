// xv_resample.hip -- sample-rate conversion in front of the MFCC kernel: what compute-mfcc-feats does with --allow-downsample /
// --allow-upsample (Kaldi's ResampleWaveform = LinearResample, a Hann-windowed sinc applied once to the whole wave), for many
// ragged utterances and several rate pairs per launch.  The algorithm is restated in DESIGN.md §8.11 and include/xvector_hip.h;
// the host side (xvector_amd/resample.py) builds the per-pair tables (first tap, tap count and fp32 weights of each of the Uo
// output phases) and the tile list.
//
// One workgroup per tile of OUT_TILE consecutive outputs of one utterance.  Output o = u Uo + p reads the taps k0 .. k0 + ntaps[p]
// - 1 with k0 = first[p] + u Ui, so a tile reads one contiguous input span of about OUT_TILE Ui / Uo + row samples.  The workgroup
// stages that span in LDS as fp32 (16 bytes per lane from global memory, 16-byte LDS stores; the span starts at the 16-byte
// boundary at or below its first sample, so both sides are aligned whatever the utterance's offset), and the weight rows too
// when the table fits (Uo row <= W_LDS floats: 80 x 67 for 44.1 k -> 8 k; a lane's row starts row dwords after its neighbour's).
// With one phase (Uo = 1: 16 k -> 8 k, 48 k -> 8 k) the row is the same for all outputs and is read with wave-uniform loads
// instead.  Thread t then runs the chain acc = fmaf(w[j], x[k0 + j], acc), j ascending from acc = 0, over the taps inside the
// wave, for outputs t, t + 256, ... of the tile: consecutive lanes store consecutive outputs.  The chain is the definition of a
// sample: its bits do not depend on the tile, the batch or the neighbours.  Per output the kernel moves 2 Ui / Uo bytes in
// (int16) and 4 out against 2 row flop, far below the ridge; measured, its time goes with the taps (one LDS read of x each),
// not with the bytes: 2.3 TB/s for 16 k -> 8 k, 0.76 TB/s for 44.1 k -> 8 k.
#include "xv_device.h"

namespace {

constexpr int RT = 256;                 // threads per workgroup
constexpr int OUT_TILE = XV_RS_OUT_TILE;
constexpr int RPT = OUT_TILE / RT;      // outputs per thread
constexpr int W_LDS = 8192;             // a table whose Uo * row is at most this many floats has its weights in LDS
constexpr int SPAN_MAX = 32 * 1024;     // most staged input samples of a tile (128 KiB; with W_LDS, the 160 KiB of a CU)

struct RsTables {
    int n;
    int64_t t[XV_RS_MAX_TABLES][XV_RS_TAB_FIELDS];
};

// 16 bytes of samples at x (16-byte aligned) as fp32
__device__ __forceinline__ void load16(const int16_t *x, float *v)
{
    const uint4 q = *(const uint4 *)x;
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = (float)(int16_t)(w[i] & 0xffffu);
        v[2 * i + 1] = (float)(int16_t)(w[i] >> 16);
    }
}
__device__ __forceinline__ void load16(const float *x, float *v)
{
    const f32x4 q = *(const f32x4 *)x;
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
}

// one fmaf chain: taps jlo .. jhi - 1 of weight row w against xs[base + j]
__device__ __forceinline__ float chain(const float *w, const float *xs, int base, int jlo, int jhi)
{
    float acc = 0.0f;
    for (int j = jlo; j < jhi; ++j) acc = fmaf(w[j], xs[base + j], acc);
    return acc;
}

// lds = xs[span_cap], then the weight rows of a table that fits (up to W_LDS floats); span_cap is a multiple of 8
template <class T>
__global__ __launch_bounds__(RT) void resample_kernel(const T *__restrict__ in, const int64_t *__restrict__ in_offset,
                                                      const int64_t *__restrict__ in_samples, const int64_t *__restrict__ out_offset,
                                                      const int64_t *__restrict__ out_samples, const int64_t *__restrict__ utt_table,
                                                      int n_utts, const RsTables tabs, const int32_t *__restrict__ first,
                                                      const int32_t *__restrict__ ntaps, const float *__restrict__ w,
                                                      const int64_t *__restrict__ tiles, float *__restrict__ out, int span_cap)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int V = 16 / (int)sizeof(T);
    float *xs = lds, *ws = lds + span_cap;
    const int tid = threadIdx.x;
    const int64_t utt = tiles[2 * blockIdx.x], o0 = tiles[2 * blockIdx.x + 1];
    if (utt < 0 || utt >= n_utts) return;
    const int64_t tb = utt_table[utt];
    if (tb < 0 || tb >= tabs.n) return;
    const int64_t n = in_samples[utt], n_out = out_samples[utt];
    if (o0 < 0 || o0 >= n_out) return;
    const int64_t *d = tabs.t[tb];
    const int Ui = (int)d[XV_RS_UI], Uo = (int)d[XV_RS_UO], row = (int)d[XV_RS_ROW];
    const int32_t *fst = first + d[XV_RS_PHASE_OFF], *nt = ntaps + d[XV_RS_PHASE_OFF];
    const float *wg = w + d[XV_RS_W_OFF];
    const bool w_lds = Uo > 1 && Uo * row <= W_LDS;
    const T *x = in + in_offset[utt];
    const int64_t u0 = o0 / Uo;
    const int p0 = (int)(o0 - u0 * Uo);
    const int tile_n = (int)min((int64_t)OUT_TILE, n_out - o0);

    // the span: from the first tap of the tile's first output to the last tap of its last one (first[] + u Ui and the row ends
    // are non-decreasing in o: the host checks its tables for it), begun at the 16-byte boundary at or below its first sample
    const int pl = p0 + tile_n - 1;
    const int64_t s_lo = fst[p0] + u0 * Ui;
    const int64_t s_hi = fst[pl % Uo] + (u0 + pl / Uo) * Ui + nt[pl % Uo];
    const int mis = (int)((int64_t)((uintptr_t)x / sizeof(T)) + s_lo) & (V - 1);
    const int64_t a = s_lo - mis;
    const int span = (int)min((int64_t)span_cap, s_hi - a);
    for (int e = V * tid; e < span; e += V * RT) {
        const int64_t s = a + e;
        float v[V];
        if (s >= 0 && s + V <= n) load16(x + s, v);
        else {
#pragma unroll
            for (int i = 0; i < V; ++i) v[i] = s + i >= 0 && s + i < n ? (float)x[s + i] : 0.0f;
        }
#pragma unroll
        for (int i = 0; i < V; i += 4) *(f32x4 *)(xs + e + i) = f32x4{v[i], v[i + 1], v[i + 2], v[i + 3]};
    }
    if (w_lds)
        for (int i = tid; i < Uo * row; i += RT) ws[i] = wg[i];
    __syncthreads();

    if (Uo == 1) {
        // one phase: the row is the same for every output, so the tap index runs over the whole row for all lanes at once, the
        // weight is a wave-uniform (scalar) load, and a lane takes part in the taps of its own range; its RPT chains interleave
        int base[RPT], jlo[RPT], jhi[RPT];
        float acc[RPT];
        const int nt0 = nt[0];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int ol = tid + RT * r;
            const int64_t k0 = fst[0] + (o0 + ol) * Ui;
            base[r] = (int)(k0 - a);
            jlo[r] = (int)max(max((int64_t)0, -k0), (int64_t)-base[r]);
            jhi[r] = ol < tile_n ? (int)min(min((int64_t)nt0, n - k0), (int64_t)(span - base[r])) : 0;
            acc[r] = 0.0f;
        }
        if (tile_n == OUT_TILE && s_lo >= 0 && s_hi <= n && s_hi - a <= span) {
            // a full tile whose every row lies inside the wave (all but the tiles at an utterance's ends): no tap to skip
            for (int j = 0; j < nt0; ++j) {
                const float wj = wg[j];
#pragma unroll
                for (int r = 0; r < RPT; ++r) acc[r] = fmaf(wj, xs[base[r] + j], acc[r]);
            }
        } else {
            for (int j = 0; j < nt0; ++j) {
                const float wj = wg[j];
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    if (j >= jlo[r] && j < jhi[r]) acc[r] = fmaf(wj, xs[base[r] + j], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RPT; ++r)
            if (tid + RT * r < tile_n) out[out_offset[utt] + o0 + tid + RT * r] = acc[r];
        return;
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int ol = tid + RT * r;
        if (ol >= tile_n) break;
        const int q = p0 + ol, p = q % Uo;
        const int64_t k0 = fst[p] + (u0 + q / Uo) * Ui;
        const int base = (int)(k0 - a);
        // taps inside the wave (the others are skipped, not multiplied by zero) and inside the staged span
        const int jlo = (int)max(max((int64_t)0, -k0), (int64_t)-base);
        const int jhi = (int)min(min((int64_t)nt[p], n - k0), (int64_t)(span - base));
        out[out_offset[utt] + o0 + ol] = w_lds ? chain(ws + p * row, xs, base, jlo, jhi) : chain(wg + (int64_t)p * row, xs, base, jlo, jhi);
    }
}

}  // namespace

extern "C" int64_t xv_resample_num_output(int64_t n, int rate_in, int rate_out)
{
    if (rate_in <= 0 || rate_out <= 0 || rate_in == rate_out) return -1;
    int64_t g = rate_in, b = rate_out;
    while (b) {
        const int64_t t = g % b;
        g = b, b = t;
    }
    // lcm ticks: an input sample is rate_out / g of them, an output sample rate_in / g
    const int64_t L = n * (rate_out / g);
    if (L <= 0) return 0;
    const int64_t tpo = rate_in / g;
    int64_t last = L / tpo;
    if (last * tpo == L) --last;
    return last + 1;
}

extern "C" int xv_resample_f32(const void *in, int in_format, const int64_t *in_offset, const int64_t *in_samples,
                               const int64_t *out_offset, const int64_t *out_samples, const int64_t *utt_table, int n_utts,
                               const int64_t *tables, int n_tables, const int32_t *first, const int32_t *ntaps, const float *w,
                               const int64_t *tiles, int64_t n_tiles, float *out, void *stream)
{
    if (n_utts < 0 || n_tables < 0 || n_tiles < 0 || (in_format != 0 && in_format != 1))
        return fail(XV_ERR_BAD_ARG, "resample: bad argument");
    if (n_tiles == 0) return 0;
    if (!in || !in_offset || !in_samples || !out_offset || !out_samples || !utt_table || !tables || !first || !ntaps || !w || !tiles ||
        !out || n_utts == 0 || n_tables == 0)
        return fail(XV_ERR_BAD_ARG, "resample: bad argument");
    if ((uintptr_t)in % (in_format == 0 ? 2 : 4)) return fail(XV_ERR_BAD_ARG, "resample: misaligned input");
    if (n_tables > XV_RS_MAX_TABLES) return fail(XV_ERR_UNSUPPORTED, "resample: too many rate pairs for one launch");
    if (n_tiles > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "resample: too many tiles for one launch");
    RsTables tabs;
    tabs.n = n_tables;
    int64_t span_cap = 8, w_floats = 0;
    for (int t = 0; t < n_tables; ++t) {
        const int64_t *d = tables + XV_RS_TAB_FIELDS * t;
        if (d[XV_RS_UI] < 1 || d[XV_RS_UO] < 1 || d[XV_RS_ROW] < 1 || d[XV_RS_PHASE_OFF] < 0 || d[XV_RS_W_OFF] < 0 || d[XV_RS_SPAN] < 1 ||
            d[XV_RS_UI] > 0x7fffffff)
            return fail(XV_ERR_BAD_ARG, "resample: bad table descriptor");
        if (d[XV_RS_ROW] > XV_RS_MAX_ROW || d[XV_RS_UO] > XV_RS_MAX_UO)
            return fail(XV_ERR_UNSUPPORTED, "resample: a tap row longer than 1024 or more than 4096 output phases");
        // + 8: the samples between the 16-byte boundary and the span's first one, rounded up to whole 16-byte LDS stores
        const int64_t cap = (d[XV_RS_SPAN] + 8 + 7) / 8 * 8;
        if (cap > SPAN_MAX) return fail(XV_ERR_UNSUPPORTED, "resample: the input span of a tile does not fit in LDS (rate ratio too large)");
        span_cap = cap > span_cap ? cap : span_cap;
        const int64_t wf = d[XV_RS_UO] * d[XV_RS_ROW];
        if (d[XV_RS_UO] > 1 && wf <= W_LDS && wf > w_floats) w_floats = wf;
        for (int f = 0; f < XV_RS_TAB_FIELDS; ++f) tabs.t[t][f] = d[f];
    }
    const size_t lds = sizeof(float) * (size_t)(span_cap + w_floats);
    static std::atomic<unsigned long long> opted{0};
    const void *kernels[] = {(const void *)resample_kernel<int16_t>, (const void *)resample_kernel<float>};
    if (int rc = opt_in_dynamic_lds(opted, kernels, (int)(sizeof(float) * (SPAN_MAX + W_LDS)))) return rc;
    if (in_format == 0)
        hipLaunchKernelGGL(resample_kernel<int16_t>, dim3((unsigned)n_tiles), dim3(RT), lds, (hipStream_t)stream, (const int16_t *)in,
                           in_offset, in_samples, out_offset, out_samples, utt_table, n_utts, tabs, first, ntaps, w, tiles, out,
                           (int)span_cap);
    else
        hipLaunchKernelGGL(resample_kernel<float>, dim3((unsigned)n_tiles), dim3(RT), lds, (hipStream_t)stream, (const float *)in,
                           in_offset, in_samples, out_offset, out_samples, utt_table, n_utts, tabs, first, ntaps, w, tiles, out,
                           (int)span_cap);
    return launch_status("resample_kernel");
}
