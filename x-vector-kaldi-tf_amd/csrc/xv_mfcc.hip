// xv_mfcc.hip -- stage 1 of the recipe on the MI355X: MFCC features (compute-mfcc-feats) and the energy VAD (compute-vad).
//
// The algorithm is restated in DESIGN.md §8.6 from Kaldi's published feature-window.cc / mel-computations.cc /
// feature-mfcc.cc / ivector/voice-activity-detection.cc; every table (window, sparse mel bank, lifter x DCT, FFT twiddles) is
// built on the host (xvector_amd/mfcc.py) and only read here.
//
// Shape: one wave (a 64-thread workgroup) owns a run of RUN consecutive output rows, which may cross utterance boundaries; the
// utterance of the first row is found by a binary search over the per-utterance first rows, then followed forward.  Per frame:
// the samples are gathered straight from HBM (reflected indices serve the snip-edges=false edges: no second code path; frames
// overlap 2.5x at 25 / 10 ms, so the repeats hit L1 / L2), dithered with Philox4x32-10 + Box-Muller, DC and energy by fp64 wave
// reductions, pre-emphasis and window into LDS, an N/2-point complex radix-2 Stockham FFT ping-ponging between two LDS
// buffers, the real split step into the power spectrum, the sparse mel bank (lane = band), log, lifter x DCT (lane = cepstrum).
// Every frame is computed by one wave in one fixed order: its bits depend on its utterance's samples and key only, never on
// the batch, its position in it, or the launch.
//
// Per frame at 8 kHz (len 200, padded 256, 23 bins, 23 cepstra): ~9.3 kflop of DSP (+~5 k integer ops of Philox with dither)
// against ~252 B of HBM traffic (160 B of new int16 at a 10 ms shift -- the 2.5x frame overlap hits L1 / L2 -- and 92 B of
// cepstra written): ~37-57 flop/B, above the MI355X's fp32 ridge (157.3 TF / 8 TB/s = ~20 flop/B), so the roofline bound is
// the ALUs.  Measured it reaches a few % of either peak: what limits it is the per-frame latency chain of one
// wave (LDS round trips and barriers per FFT stage, serial mel / DCT dot products), not a roof.
#include "xv_device.h"

namespace {

constexpr int WAVE = 64;
constexpr int RUN = 8;                 // consecutive output rows per workgroup
constexpr int MAX_PAD = 1024;          // padded lengths 128 .. 1024 (powers of two)
constexpr int MAX_BINS = 128;

struct MfccArgs {
    const void *samples;
    int fmt;                           // 0: int16, 1: fp32
    const int64_t *utt_offset, *utt_samples, *utt_row0;
    const uint64_t *utt_key;
    int n_utts;
    int64_t total_rows;
    const float *window;               // [frame_length]
    const int32_t *mel_first, *mel_len;
    const float *mel_w;                // [num_bins, mel_ld]
    int num_bins, mel_ld;
    const float *dct;                  // [num_ceps, num_bins]: lifter x DCT-II
    int num_ceps;
    const float2 *twiddle;             // [padded / 2]: exp(-2 pi i k / padded)
    int frame_length, frame_shift, padded, log2_half, snip_edges;
    float dither, preemph;
    int remove_dc, use_energy, raw_energy;
    float log_energy_floor;            // -inf: no floor
    float *feats;
    int64_t ld_feats;
    float *logmel;
    int64_t ld_logmel;
};

__device__ __forceinline__ int64_t num_frames(int64_t n, int len, int shift, int snip)
{
    if (snip) return n < len ? 0 : 1 + (n - len) / shift;
    return (n + shift / 2) / shift;
}

// Philox4x32-10 (Salmon et al., SC'11), the Random123 reference constants
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = make_uint4((uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1, (uint32_t)p0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// N(0, 1) for sample i of frame t: counter (i, t mod 2^32, t >> 32, 0), Box-Muller on the top 24 bits of the first two words
__device__ __forceinline__ float gauss(uint64_t key, int64_t t, int i)
{
    const uint4 r = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), 0u), (uint32_t)key,
                                  (uint32_t)(key >> 32));
    const float u1 = ((float)(r.x >> 8) + 0.5f) * 5.9604644775390625e-8f;      // (0, 1)
    const float u2 = (float)(r.y >> 8) * 5.9604644775390625e-8f;               // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

__global__ __launch_bounds__(WAVE) void mfcc_kernel(MfccArgs a)
{
    __shared__ float2 buf[2][MAX_PAD / 2];          // the frame (as N/2 complex values), then the FFT's ping-pong
    __shared__ float mel[MAX_BINS];
    const int lane = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * RUN;
    if (r0 >= a.total_rows) return;
    // utterance of row r0: the largest u with utt_row0[u] <= r0 (utterances without frames share the next one's first row)
    int lo = 0, hi = a.n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.utt_row0[mid] <= r0) lo = mid;
        else hi = mid - 1;
    }
    int u = lo;
    const int L = a.frame_length, N = a.padded, H = N >> 1;
    const int64_t r_end = min(r0 + RUN, a.total_rows);
    for (int64_t r = r0; r < r_end; ++r) {
        while (u + 1 < a.n_utts && a.utt_row0[u + 1] <= r) ++u;
        const int64_t ns = a.utt_samples[u];
        const int64_t t = r - a.utt_row0[u];
        if (t >= num_frames(ns, L, a.frame_shift, a.snip_edges)) continue;     // rows the tables do not give a frame: untouched
        const int64_t first = a.snip_edges ? t * a.frame_shift : t * a.frame_shift + a.frame_shift / 2 - L / 2;
        const int16_t *s16 = (const int16_t *)a.samples + a.utt_offset[u];
        const float *s32 = (const float *)a.samples + a.utt_offset[u];
        const uint64_t key = a.utt_key[u];
        float *x = (float *)buf[0];
        // 1. gather (reflected), dither; fp64 sums for the DC offset
        double sum = 0.0;
        for (int i = lane; i < L; i += WAVE) {
            int64_t s = first + i;
            while (s < 0 || s >= ns) s = s < 0 ? -s - 1 : 2 * ns - 1 - s;
            float v = a.fmt == 0 ? (float)s16[s] : s32[s];
            if (a.dither != 0.0f) v += a.dither * gauss(key, t, i);
            x[i] = v;
            sum += (double)v;
        }
        const float mean = a.remove_dc ? (float)(wave_sum(sum) / (double)L) : 0.0f;
        __syncthreads();
        // 2-3. DC removal, raw log energy
        double e = 0.0;
        float v[MAX_PAD / WAVE], prev[MAX_PAD / WAVE];
#pragma unroll
        for (int q = 0; q < MAX_PAD / WAVE; ++q) {
            const int i = lane + q * WAVE;
            if (i < L) {
                v[q] = x[i] - mean;
                prev[q] = i > 0 ? x[i - 1] - mean : v[q];
                e += (double)v[q] * (double)v[q];
            }
        }
        float log_energy = 0.0f;
        if (a.use_energy && a.raw_energy) log_energy = logf(fmaxf((float)wave_sum(e), 1.1920928955078125e-7f));
        __syncthreads();
        // 4-6. pre-emphasis (on the DC-free samples), window, zero padding
        double e_win = 0.0;
#pragma unroll
        for (int q = 0; q < MAX_PAD / WAVE; ++q) {
            const int i = lane + q * WAVE;
            if (i < N) {
                float w = 0.0f;
                if (i < L) {
                    w = (a.preemph != 0.0f ? v[q] - a.preemph * prev[q] : v[q]) * a.window[i];
                    e_win += (double)w * (double)w;
                }
                x[i] = w;
            }
        }
        if (a.use_energy && !a.raw_energy) log_energy = logf(fmaxf((float)wave_sum(e_win), 1.1920928955078125e-7f));
        if (log_energy < a.log_energy_floor) log_energy = a.log_energy_floor;
        __syncthreads();
        // 7. N/2-point complex FFT of z[n] = x[2n] + i x[2n+1]: radix-2 Stockham, twiddles exp(-2 pi i k / (2 Ns)) = table[k N / (2 Ns)]
        int src = 0;
        for (int st = 0; st < a.log2_half; ++st) {
            const int Ns = 1 << st;
            for (int j = lane; j < H / 2; j += WAVE) {
                const int k = j & (Ns - 1);
                const float2 a0 = buf[src][j];
                const float2 a1 = cmul(buf[src][j + H / 2], a.twiddle[k << (a.log2_half - st)]);
                const int d = ((j - k) << 1) + k;
                buf[src ^ 1][d] = make_float2(a0.x + a1.x, a0.y + a1.y);
                buf[src ^ 1][d + Ns] = make_float2(a0.x - a1.x, a0.y - a1.y);
            }
            src ^= 1;
            __syncthreads();
        }
        // split step: X_k = (Z_k + conj Z_{H-k}) / 2 - i W^k (Z_k - conj Z_{H-k}) / 2, power |X_k|^2 for k < H (Nyquist unused)
        float *pw = (float *)buf[src ^ 1];
        for (int k = lane; k < H; k += WAVE) {
            const float2 z = buf[src][k], zc = buf[src][(H - k) & (H - 1)];
            const float2 ev = make_float2(0.5f * (z.x + zc.x), 0.5f * (z.y - zc.y));
            const float2 od = make_float2(0.5f * (z.y + zc.y), -0.5f * (z.x - zc.x));
            const float2 xo = cmul(a.twiddle[k], od);
            const float re = ev.x + xo.x, im = ev.y + xo.y;
            pw[k] = re * re + im * im;
        }
        __syncthreads();
        // mel bank, log
        for (int b = lane; b < a.num_bins; b += WAVE) {
            const int f = a.mel_first[b], n = a.mel_len[b];
            const float *w = a.mel_w + (int64_t)b * a.mel_ld;
            float m = 0.0f;
            for (int j = 0; j < n; ++j) m = fmaf(w[j], pw[f + j], m);
            const float lm = logf(fmaxf(m, 1.1920928955078125e-7f));
            mel[b] = lm;
            if (a.logmel) a.logmel[r * a.ld_logmel + b] = lm;
        }
        __syncthreads();
        // lifter x DCT; c0 := log energy
        for (int c = lane; c < a.num_ceps; c += WAVE) {
            const float *d = a.dct + (int64_t)c * a.num_bins;
            float y = 0.0f;
            for (int b = 0; b < a.num_bins; ++b) y = fmaf(d[b], mel[b], y);
            if (c == 0 && a.use_energy) y = log_energy;
            a.feats[r * a.ld_feats + c] = y;
        }
        __syncthreads();
    }
}

// compute-vad: one workgroup per utterance.  The sum of column 0 in fp64 in a fixed order (thread j: rows j, j + 256, ...
// ascending, then a fixed tree), so the threshold of an utterance never depends on the batch it came in.
constexpr int VAD_THREADS = 256;

__global__ __launch_bounds__(VAD_THREADS) void vad_energy_kernel(const float *__restrict__ feats, int64_t ld,
                                                                 const int64_t *__restrict__ row0, const int32_t *__restrict__ n_frames,
                                                                 float threshold, float mean_scale, int context, float proportion,
                                                                 float *__restrict__ out)
{
    __shared__ double part[VAD_THREADS];
    const int u = blockIdx.x;
    const int T = n_frames[u];
    if (T <= 0) return;
    const float *c0 = feats + row0[u] * ld;
    double s = 0.0;
    for (int t = threadIdx.x; t < T; t += VAD_THREADS) s += (double)c0[(int64_t)t * ld];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int m = VAD_THREADS / 2; m >= 1; m >>= 1) {
        if (threadIdx.x < m) part[threadIdx.x] += part[threadIdx.x + m];
        __syncthreads();
    }
    const double thr = (double)threshold + (double)mean_scale * part[0] / (double)T;
    for (int t = threadIdx.x; t < T; t += VAD_THREADS) {
        int num = 0, den = 0;
        for (int t2 = t - context; t2 <= t + context; ++t2) {
            if (t2 >= 0 && t2 < T) {
                ++den;
                if ((double)c0[(int64_t)t2 * ld] > thr) ++num;
            }
        }
        out[row0[u] + t] = (float)num >= (float)den * proportion ? 1.0f : 0.0f;
    }
}

}  // namespace

extern "C" int xv_mfcc_f32(const void *samples, int sample_format, const int64_t *utt_offset, const int64_t *utt_samples,
                           const int64_t *utt_row0, const uint64_t *utt_key, int n_utts, int64_t total_rows, const float *window,
                           const int32_t *mel_first, const int32_t *mel_len, const float *mel_w, int num_bins, int mel_ld,
                           const float *lifter_dct, int num_ceps, const float *twiddle, int frame_length, int frame_shift,
                           int padded_length, int snip_edges, float dither, float preemph_coeff, int remove_dc, int use_energy,
                           int raw_energy, float energy_floor, float *feats, int64_t ld_feats, float *logmel, int64_t ld_logmel,
                           void *stream)
{
    if (padded_length < 128 || padded_length > MAX_PAD || (padded_length & (padded_length - 1)))
        return fail(XV_ERR_UNSUPPORTED, "mfcc: padded length must be a power of two in [128, 1024]");
    if (num_bins > MAX_BINS) return fail(XV_ERR_UNSUPPORTED, "mfcc: more than 128 mel bins");
    if (n_utts < 0 || total_rows < 0 || (sample_format != 0 && sample_format != 1) || frame_length < 1 ||
        frame_length > padded_length || frame_shift < 1 || num_bins < 1 || num_ceps < 1 || num_ceps > num_bins || mel_ld < 1 ||
        ld_feats < num_ceps || (logmel && ld_logmel < num_bins) || dither < 0.0f)
        return fail(XV_ERR_BAD_ARG, "mfcc: bad argument");
    if (total_rows == 0) return 0;
    if (n_utts == 0 || !samples || !utt_offset || !utt_samples || !utt_row0 || !utt_key || !window || !mel_first || !mel_len ||
        !mel_w || !lifter_dct || !twiddle || !feats)
        return fail(XV_ERR_BAD_ARG, "mfcc: bad argument");
    const int64_t blocks = (total_rows + RUN - 1) / RUN;
    if (blocks > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "mfcc: too many rows for one launch");
    MfccArgs a;
    a.samples = samples;
    a.fmt = sample_format;
    a.utt_offset = utt_offset;
    a.utt_samples = utt_samples;
    a.utt_row0 = utt_row0;
    a.utt_key = utt_key;
    a.n_utts = n_utts;
    a.total_rows = total_rows;
    a.window = window;
    a.mel_first = mel_first;
    a.mel_len = mel_len;
    a.mel_w = mel_w;
    a.num_bins = num_bins;
    a.mel_ld = mel_ld;
    a.dct = lifter_dct;
    a.num_ceps = num_ceps;
    a.twiddle = (const float2 *)twiddle;
    a.frame_length = frame_length;
    a.frame_shift = frame_shift;
    a.padded = padded_length;
    a.log2_half = 0;
    while ((2 << a.log2_half) < padded_length) ++a.log2_half;
    a.snip_edges = snip_edges;
    a.dither = dither;
    a.preemph = preemph_coeff;
    a.remove_dc = remove_dc;
    a.use_energy = use_energy;
    a.raw_energy = raw_energy;
    a.log_energy_floor = energy_floor > 0.0f ? logf(energy_floor) : -__builtin_huge_valf();
    a.feats = feats;
    a.ld_feats = ld_feats;
    a.logmel = logmel;
    a.ld_logmel = ld_logmel;
    hipLaunchKernelGGL(mfcc_kernel, dim3((unsigned)blocks), dim3(WAVE), 0, (hipStream_t)stream, a);
    return launch_status("mfcc_kernel");
}

extern "C" int xv_vad_energy_f32(const float *feats, int64_t ld, const int64_t *utt_row0, const int32_t *n_frames, int n_utts,
                                 float energy_threshold, float energy_mean_scale, int frames_context, float proportion_threshold,
                                 float *out, void *stream)
{
    if (n_utts == 0) return 0;
    if (n_utts < 0 || !feats || ld < 1 || !utt_row0 || !n_frames || !out || frames_context < 0)
        return fail(XV_ERR_BAD_ARG, "vad_energy: bad argument");
    hipLaunchKernelGGL(vad_energy_kernel, dim3(n_utts), dim3(VAD_THREADS), 0, (hipStream_t)stream, feats, ld, utt_row0, n_frames,
                       energy_threshold, energy_mean_scale, frames_context, proportion_threshold, out);
    return launch_status("vad_energy_kernel");
}
