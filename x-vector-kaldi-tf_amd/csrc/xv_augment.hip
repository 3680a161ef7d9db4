// xv_augment.hip -- stage 2 of the recipe on the MI355X: what Kaldi's wav-reverberate does to one wav.scp entry (reverberation
// with a room impulse response, additive noises at given SNRs, level, shift / trim / repeat, the int16 write), for many ragged
// utterances per launch.  The semantics are restated in DESIGN.md §8.7; the host side (xvector_amd/augment.py) parses the
// entries, decodes every distinct RIR and noise once, and lays out the descriptor tables read here.
//
// Pipeline of one evaluation level (an evaluation whose noise is itself a nested wav-reverberate runs one level later):
//   power   sum of squares of each distinct int16 segment (inputs, noises), per tile       one workgroup per 16384 samples
//   conv    y = x * h (full linear convolution) and x * h[start:end] (early reverb)       one workgroup per 2048 outputs
//   gains   P0, E and the noise scales (segment sums from the power tiles)                 one thread per utterance
//   mix     y += s_i n_i at the offsets, sum of y^2 per tile                              one workgroup per 1024 samples
//   level   P1 and the level scale (volume or sqrt(P0 / P1))                              one thread per utterance
//   write   shift, trim / repeat, scale, truncate toward zero, saturate to int16           one workgroup per 1024 samples
// Every reduction is fp64 in a fixed order, and every tile starts at a multiple of its size counted from its own utterance's
// first sample, so an utterance's bits depend on its own inputs only, never on the batch.  Every output sample is written by
// exactly one thread; the only atomics are integer clip counters.
//
// The waveform is fp64 from the convolution to the write.  The products of the taps (int16 / 32768) and int16 samples are exact
// in fp64, and so are their sums at these magnitudes (partial sums below 2^35 on a 2^-15 grid), so the convolution is exact.  Each
// noise add (an fp32 scale times an int16 sample, an exact product, added to y) rounds once in fp64, and so does the level
// product (fp64 y times the fp32 level); the truncation to int16 is the only rounding at fp32 scale or coarser.  The
// convolution is the direct form.  Per output sample it costs 2 min(N, L) flop (fp64 FMA) and, per tile of 2048 outputs, one pass over
// the taps through LDS: ~2 B of HBM per output from the x window and 4 L B per tile of h, i.e. 2 L / (2 + 2 L / 1024) flop/B
// (~1000 at L = 8000): far above any ridge, so the bound is the fp64 FMA rate (DESIGN.md §8.7 has the roofline and the
// measured rate, and why the direct form was kept over FFT overlap-save).
#include "xv_device.h"

namespace {

constexpr int CT = 256;                 // conv: threads per workgroup
constexpr int CR = 8;                   // conv: consecutive outputs per thread
constexpr int CTILE = CT * CR;          // conv: outputs per tile
constexpr int CCH = 1024;               // conv: taps per LDS chunk
constexpr int CXS = CTILE + CCH;        // conv: x window per chunk (CTILE + CCH - 1 used, one spare)
constexpr int ET = 256;                 // element-wise kernels: threads per workgroup
constexpr int EPT = 4;                  // element-wise kernels: samples per thread
constexpr int PTILE = 16384;            // power: samples per tile (64 per thread)

// LDS index of x-window element j: one pad word per 8, so lane t reading element 8 t + e hits bank (9 t + ..) mod 32
__device__ __forceinline__ int xs_idx(int j) { return j + (j >> 3); }

// fixed-order workgroup sum of one fp64 per thread (n threads, n a power of two); every thread gets the total
template <int NT>
__device__ __forceinline__ double block_sum(double v, double *part)
{
    part[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int m = NT / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) part[threadIdx.x] += part[threadIdx.x + m];
        __syncthreads();
    }
    const double s = part[0];
    __syncthreads();
    return s;
}

// segment s = segments[4s ..] = (off, len, tile0, ntiles); tile t = tiles[2t ..] = (segment, i0), i0 a multiple of PTILE:
// tile_sumsq[t] = the fp64 sum of sig[off + i]^2 over i in [i0, min(i0 + PTILE, len)), in a fixed order
__global__ __launch_bounds__(ET) void aug_power_kernel(const int16_t *__restrict__ sig, const int64_t *__restrict__ segments,
                                                       const int64_t *__restrict__ tiles, double *__restrict__ tile_sumsq)
{
    __shared__ double part[ET];
    const int64_t *sg = segments + 4 * tiles[2 * blockIdx.x];
    const int64_t i0 = tiles[2 * blockIdx.x + 1];
    const int64_t off = sg[0], end = min(sg[1], i0 + PTILE);
    double s = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < end; i += ET) {
        const double v = (double)sig[off + i];
        s += v * v;
    }
    s = block_sum<ET>(s, part);
    if (threadIdx.x == 0) tile_sumsq[blockIdx.x] = s;
}

// the fp64 sum of squares of segment s: its power tiles in order
__device__ __forceinline__ double segment_sumsq(const int64_t *segments, const double *power_sumsq, int64_t s)
{
    const int64_t *sg = segments + 4 * s;
    double v = 0.0;
    for (int64_t t = 0; t < sg[3]; ++t) v += power_sumsq[sg[2] + t];
    return v;
}

// job j: x = sig[x_off .. + N), h = taps[h_off .. + L), outputs n in [0, N + L - 1) to y[y_off + n] (y_off < 0: not written);
// tile t = (job, n0) covers outputs n0 .. n0 + CTILE - 1 and leaves the fp64 sum of their squares in tile_sumsq[t]
__global__ __launch_bounds__(CT) void aug_conv_kernel(const int16_t *__restrict__ sig, const float *__restrict__ taps,
                                                      const int64_t *__restrict__ jobs, const int64_t *__restrict__ tiles,
                                                      double *__restrict__ y, double *__restrict__ tile_sumsq)
{
    __shared__ float xs[CXS + CXS / 8];
    __shared__ float hs[CCH];
    __shared__ double part[CT];
    const int tid = threadIdx.x;
    const int64_t *job = jobs + 5 * tiles[2 * blockIdx.x];
    const int64_t n0 = tiles[2 * blockIdx.x + 1];
    const int64_t x_off = job[0], N = job[1], h_off = job[2], L = job[3], y_off = job[4];
    const int64_t ylen = N + L - 1;
    const int16_t *x = sig + x_off;
    const float *h = taps + h_off;
    // taps that meet a sample of x for some output of the tile: n - k in [0, N), k in [0, L)
    const int64_t k_lo = max((int64_t)0, n0 - N + 1), k_hi = min(L - 1, n0 + CTILE - 1);
    double acc[CR];
#pragma unroll
    for (int r = 0; r < CR; ++r) acc[r] = 0.0;
    for (int64_t kc = k_lo; kc <= k_hi; kc += CCH) {
        // chunk taps kc + c, c < CCH; output n0 + CR t + r at tap kc + c reads x[base + CR t + r + (CCH - 1 - c)]
        const int64_t base = n0 - kc - (CCH - 1);
        for (int c = tid; c < CCH; c += CT) hs[c] = kc + c <= k_hi ? h[kc + c] : 0.0f;
        for (int j = tid; j < CXS; j += CT) {
            const int64_t s = base + j;
            xs[xs_idx(j)] = s >= 0 && s < N ? (float)x[s] : 0.0f;
        }
        __syncthreads();
        double w[2 * CR];
#pragma unroll
        for (int r = 0; r < CR; ++r) w[r] = (double)xs[xs_idx(CR * tid + r)];
        for (int d = 0; d < CCH; d += CR) {
#pragma unroll
            for (int e = 0; e < CR; ++e) w[CR + e] = (double)xs[xs_idx(CR * tid + CR + d + e)];
#pragma unroll
            for (int e = 0; e < CR; ++e) {
                const double hv = (double)hs[CCH - 1 - d - e];
#pragma unroll
                for (int r = 0; r < CR; ++r) acc[r] = fma(hv, w[r + e], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < CR; ++r) w[r] = w[CR + r];
        }
        __syncthreads();
    }
    double ss = 0.0;
#pragma unroll
    for (int r = 0; r < CR; ++r) {
        const int64_t n = n0 + CR * tid + r;
        if (n < ylen) {
            if (y_off >= 0) y[y_off + n] = acc[r];
            ss += acc[r] * acc[r];
        }
    }
    ss = block_sum<CT>(ss, part);
    if (tid == 0) tile_sumsq[blockIdx.x] = ss;
}

__global__ void aug_gains_kernel(const int64_t *__restrict__ utt, int n_utts, const int64_t *__restrict__ refs,
                                 const float *__restrict__ ref_snr, const int64_t *__restrict__ segments,
                                 const double *__restrict__ power_sumsq,
                                 const double *__restrict__ conv_sumsq, double *__restrict__ utt_out, double *__restrict__ ref_power,
                                 float *__restrict__ ref_scale)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_utts) return;
    const int64_t *d = utt + XV_AUG_UTT_FIELDS * u;
    const double p0 = segment_sumsq(segments, power_sumsq, d[XV_AUG_X_SEG]) / (double)d[XV_AUG_N];
    double e = p0;
    if (d[XV_AUG_EARLY_NTILES] > 0) {
        double s = 0.0;
        for (int64_t t = 0; t < d[XV_AUG_EARLY_NTILES]; ++t) s += conv_sumsq[d[XV_AUG_EARLY_TILE0] + t];
        e = s / (double)d[XV_AUG_EARLY_LEN];
    }
    utt_out[4 * u + 0] = p0;
    utt_out[4 * u + 1] = e;
    for (int64_t r = d[XV_AUG_REF0]; r < d[XV_AUG_REF0] + d[XV_AUG_NREF]; ++r) {
        const int64_t *q = refs + XV_AUG_REF_FIELDS * r;
        const int64_t len = q[XV_AUG_REF_NOISE_LEN];
        const double pn = len > 0 ? segment_sumsq(segments, power_sumsq, q[XV_AUG_REF_NOISE_SEG]) / (double)len : 0.0;
        ref_power[r] = pn;
        ref_scale[r] = pn > 0.0 ? (float)sqrt(pow(10.0, -(double)ref_snr[r] / 10.0) * e / pn) : 0.0f;
    }
}

// tile t = (utterance, n0): samples n0 .. n0 + ET * EPT - 1 of y (the convolution in y, or x itself without an RIR) plus the
// scaled noises in list order (fp64: the product of the fp32 scale and an int16 sample is exact), written back to y, fp64 sum of
// squares per tile
__global__ __launch_bounds__(ET) void aug_mix_kernel(const int16_t *__restrict__ sig, const int64_t *__restrict__ utt,
                                                     const int64_t *__restrict__ refs, const float *__restrict__ ref_scale,
                                                     const int64_t *__restrict__ tiles, double *__restrict__ y,
                                                     double *__restrict__ tile_sumsq)
{
    __shared__ double part[ET];
    const int64_t *d = utt + XV_AUG_UTT_FIELDS * tiles[2 * blockIdx.x];
    const int64_t n0 = tiles[2 * blockIdx.x + 1];
    const int64_t ylen = d[XV_AUG_Y_LEN], y_off = d[XV_AUG_Y_OFF], x_off = d[XV_AUG_X_OFF];
    const bool rir = d[XV_AUG_RIR] != 0;
    const int64_t r0 = d[XV_AUG_REF0], nr = d[XV_AUG_NREF];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int64_t n = n0 + threadIdx.x + ET * i;
        if (n >= ylen) break;
        double v = rir ? y[y_off + n] : (double)sig[x_off + n];
        for (int64_t r = r0; r < r0 + nr; ++r) {
            const int64_t *q = refs + XV_AUG_REF_FIELDS * r;
            const int64_t j = n - q[XV_AUG_REF_OFFSET];
            if (j >= 0 && j < q[XV_AUG_REF_NOISE_LEN]) v += (double)ref_scale[r] * (double)sig[q[XV_AUG_REF_NOISE_OFF] + j];
        }
        y[y_off + n] = v;
        ss += v * v;
    }
    ss = block_sum<ET>(ss, part);
    if (threadIdx.x == 0) tile_sumsq[blockIdx.x] = ss;
}

__global__ void aug_level_kernel(const int64_t *__restrict__ utt, int n_utts, const double *__restrict__ utt_param,
                                 const double *__restrict__ mix_sumsq, double *__restrict__ utt_out)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n_utts) return;
    const int64_t *d = utt + XV_AUG_UTT_FIELDS * u;
    double s = 0.0;
    for (int64_t t = 0; t < d[XV_AUG_MIX_NTILES]; ++t) s += mix_sumsq[d[XV_AUG_MIX_TILE0] + t];
    const double p1 = s / (double)d[XV_AUG_Y_LEN];
    const double volume = utt_param[2 * u], normalize = utt_param[2 * u + 1];
    float level = 1.0f;
    if (volume > 0.0) level = (float)volume;
    else if (normalize != 0.0 && p1 > 0.0) level = (float)sqrt(utt_out[4 * u] / p1);
    utt_out[4 * u + 2] = p1;
    utt_out[4 * u + 3] = (double)level;
}

// tile t = (utterance, m0): output m = trunc_sat(y[shift + (m mod N)] * level) for m < M (fp64; the fp32 level times y), to
// out[out_off + m]
__global__ __launch_bounds__(ET) void aug_write_kernel(const double *__restrict__ y, const int64_t *__restrict__ utt,
                                                       const double *__restrict__ utt_out, const int64_t *__restrict__ tiles,
                                                       void *__restrict__ out, int fmt, unsigned long long *__restrict__ clipped)
{
    const int u = (int)tiles[2 * blockIdx.x];
    const int64_t *d = utt + XV_AUG_UTT_FIELDS * u;
    const int64_t m0 = tiles[2 * blockIdx.x + 1];
    const int64_t M = d[XV_AUG_M], N = d[XV_AUG_N], src0 = d[XV_AUG_Y_OFF] + d[XV_AUG_SHIFT], out_off = d[XV_AUG_OUT_OFF];
    const double level = utt_out[4 * u + 3];           // an fp32 value
    int nclip = 0;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int64_t m = m0 + threadIdx.x + ET * i;
        if (m >= M) break;
        const double v = trunc(y[src0 + (m < N ? m : m % N)] * level);
        float q = (float)v;
        if (!(v >= -32768.0)) q = -32768.0f, ++nclip;           // (NaN saturates low and counts as clipped)
        else if (v > 32767.0) q = 32767.0f, ++nclip;
        if (fmt == 0) ((int16_t *)out)[out_off + m] = (int16_t)q;
        else ((float *)out)[out_off + m] = q;
    }
    // integer count, one atomic per wave with clipping
    for (int m = 32; m >= 1; m >>= 1) nclip += __shfl_xor(nclip, m, 64);
    if ((threadIdx.x & 63) == 0 && nclip) atomicAdd(clipped + u, (unsigned long long)nclip);
}

}  // namespace

extern "C" int xv_augment_power_f64(const int16_t *sig, const int64_t *segments, const int64_t *tiles, int64_t n_tiles,
                                    double *tile_sumsq, void *stream)
{
    if (n_tiles == 0) return 0;
    if (n_tiles < 0 || !sig || !segments || !tiles || !tile_sumsq) return fail(XV_ERR_BAD_ARG, "augment_power: bad argument");
    if (n_tiles > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "augment_power: too many tiles for one launch");
    hipLaunchKernelGGL(aug_power_kernel, dim3((unsigned)n_tiles), dim3(ET), 0, (hipStream_t)stream, sig, segments, tiles, tile_sumsq);
    return launch_status("aug_power_kernel");
}

extern "C" int xv_augment_conv_f64(const int16_t *sig, const float *taps, const int64_t *jobs, const int64_t *tiles, int64_t n_tiles,
                                   double *y, double *tile_sumsq, void *stream)
{
    if (n_tiles == 0) return 0;
    if (n_tiles < 0 || !sig || !taps || !jobs || !tiles || !tile_sumsq) return fail(XV_ERR_BAD_ARG, "augment_conv: bad argument");
    if (n_tiles > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "augment_conv: too many tiles for one launch");
    hipLaunchKernelGGL(aug_conv_kernel, dim3((unsigned)n_tiles), dim3(CT), 0, (hipStream_t)stream, sig, taps, jobs, tiles, y, tile_sumsq);
    return launch_status("aug_conv_kernel");
}

extern "C" int xv_augment_gains_f32(const int64_t *utt, int n_utts, const int64_t *refs, const float *ref_snr, const int64_t *segments,
                                    const double *power_sumsq, const double *conv_sumsq, double *utt_out, double *ref_power,
                                    float *ref_scale, void *stream)
{
    if (n_utts == 0) return 0;
    if (n_utts < 0 || !utt || !segments || !power_sumsq || !utt_out) return fail(XV_ERR_BAD_ARG, "augment_gains: bad argument");
    hipLaunchKernelGGL(aug_gains_kernel, dim3((n_utts + 63) / 64), dim3(64), 0, (hipStream_t)stream, utt, n_utts, refs, ref_snr,
                       segments, power_sumsq, conv_sumsq, utt_out, ref_power, ref_scale);
    return launch_status("aug_gains_kernel");
}

extern "C" int xv_augment_mix_f64(const int16_t *sig, const int64_t *utt, const int64_t *refs, const float *ref_scale,
                                  const int64_t *tiles, int64_t n_tiles, double *y, double *tile_sumsq, void *stream)
{
    if (n_tiles == 0) return 0;
    if (n_tiles < 0 || !sig || !utt || !tiles || !y || !tile_sumsq) return fail(XV_ERR_BAD_ARG, "augment_mix: bad argument");
    if (n_tiles > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "augment_mix: too many tiles for one launch");
    hipLaunchKernelGGL(aug_mix_kernel, dim3((unsigned)n_tiles), dim3(ET), 0, (hipStream_t)stream, sig, utt, refs, ref_scale, tiles, y,
                       tile_sumsq);
    return launch_status("aug_mix_kernel");
}

extern "C" int xv_augment_level_f32(const int64_t *utt, int n_utts, const double *utt_param, const double *mix_sumsq, double *utt_out,
                                    void *stream)
{
    if (n_utts == 0) return 0;
    if (n_utts < 0 || !utt || !utt_param || !mix_sumsq || !utt_out) return fail(XV_ERR_BAD_ARG, "augment_level: bad argument");
    hipLaunchKernelGGL(aug_level_kernel, dim3((n_utts + 63) / 64), dim3(64), 0, (hipStream_t)stream, utt, n_utts, utt_param, mix_sumsq,
                       utt_out);
    return launch_status("aug_level_kernel");
}

extern "C" int xv_augment_write(const double *y, const int64_t *utt, const double *utt_out, const int64_t *tiles, int64_t n_tiles,
                                void *out, int sample_format, unsigned long long *clipped, void *stream)
{
    if (n_tiles == 0) return 0;
    if (n_tiles < 0 || !y || !utt || !utt_out || !tiles || !out || !clipped || (sample_format != 0 && sample_format != 1))
        return fail(XV_ERR_BAD_ARG, "augment_write: bad argument");
    if (n_tiles > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "augment_write: too many tiles for one launch");
    hipLaunchKernelGGL(aug_write_kernel, dim3((unsigned)n_tiles), dim3(ET), 0, (hipStream_t)stream, y, utt, utt_out, tiles, out,
                       sample_format, clipped);
    return launch_status("aug_write_kernel");
}
