// pitch_track.hip -- a guide f0 curve from a recording, on the device: YIN (de Cheveigne & Kawahara 2002) with a lag-centred difference function, one launch
// for a batch of waveforms.  DESIGN.md 4.11, the rule: include/visinger_hip.h "f6".  Not in the reference, whose extractors (utils/audio/pitch_extractors.py)
// call parselmouth / pyworld on the host, one file at a time.
//   Per frame t (centre c = t hop + hop / 2, base = c - W / 2) and lag tau = 1 .. tau_max + 1:  d(tau) = sum_{j < W} (x[base - tau/2 + j] - x[base - tau/2 + j + tau])^2,
//   then S = prefix sum of d, d' = d tau / S, the YIN search on d' and a parabola through its minimum.
// Tiling.  A workgroup of 256 lanes takes F consecutive frames of one row (F <= 8, chosen by the host: the span fits the LDS and the fewest lanes idle) and
// stages their common span of samples ONCE (zeros outside [0, lengths[b])).  The work items are (frame, lag group g): lags 8g .. 8g + 7 of one frame in one lane.
// Those eight lags read only two sample streams, a = x[base - 4g + j - {0 .. 3}] and b = x[base + 4g + j + {0 .. 4}], so a step of four samples j costs two
// 16-byte LDS reads for 32 subtract / multiply-add pairs -- the rest of both windows slides through registers.  Neighbouring lanes' streams are 4 dwords apart
// and every read is 16 bytes at a multiple of 4 dwords: the 16 lanes of a ds_read_b128 group have distinct lane numbers modulo 16, so they cover the 64 banks
// once, conflict-free (two 8-byte reads per two samples, the first form of this kernel, were merged by the compiler into ds_read2_b64, which runs at a quarter
// of that rate).  The alignment is a property of the image, not of the data: when the hop is no multiple of 4 the frames' bases fall on other residues, so 2
// (hop = 2 mod 4) or 4 (odd hop) images of the span, shifted by those residues, are staged and a frame reads the one that aligns it.
// Summation order (fixed per frame and lag, whatever F, B, L, T are): d(tau) = ((B_0 + B_1) + B_2) + ..., B_k = the chain acc = fmaf(v, v, acc) from acc = 0
// over j = 32k .. min(32k + 31, W - 1) ascending, v = a - b rounded to fp32.  S: see the tail.  fp32 on the VALU throughout: the MFMA form of this sum is
// energy - 2 autocorrelation, which cancels in fp32 near a period, where d' is read.
#include "vs_internal.h"

#include <cmath>

namespace vs {

constexpr int YIN_THREADS = 256;
constexpr int YIN_MAX_TAU = 1024;              // tau_max: d' has tau_max + 2 slots, a lane of the scan takes 17 of them (64 x 17 = 1088)
constexpr int YIN_MAX_W = 2048;
constexpr int YIN_MAX_F = 8;                   // frames per workgroup
constexpr int YIN_LDS_FLOATS = 15360;          // 60 KiB of the workgroup's 64
constexpr int YIN_SCAN = 17;                   // lags per lane of the prefix sum

struct YinArgs {
    const float *wav;
    const long long *lengths;
    float *f0, *per, *cand_hz, *cand_d;                         // yin: f0, per (or NULL); candidates: cand_hz, cand_d [B, T, 8]
    long long B, L, T;
    int sr, hop, W, tau_min, tau_max, G, F, K, n_img, DP;        // G lag groups of 8; K images (1, 2 or 4 shifts); n_img floats per image; DP floats per d' row
    float thr, silence_w;                                       // thr: YIN's threshold, or the candidates' gate; silence_w = silence * W (one fp32 product, on the host)
};

// the eight difference sums of lags 8g .. 8g + 7 for one frame; img: the frame's image, rel (a multiple of 4) = index of x[base] in it.
// Lag 8g + m compares a = pa[j - (m >> 1)] with b = pb[j + ((m + 1) >> 1)], pa = &x[base - 4g], pb = &x[base + 4g].
__device__ __forceinline__ void yin_lag8(const float *__restrict__ img, int rel, int g, int W, float (&tot)[8]) {
    const float *pa = img + rel - 4 * g, *pb = img + rel + 4 * g;          // both at a multiple of four floats: 16-byte reads
    float4 ap = *reinterpret_cast<const float4 *>(pa - 4);                  // pa[j - 4 .. j - 1]
    float4 bc = *reinterpret_cast<const float4 *>(pb);                      // pb[j .. j + 3]
#pragma unroll
    for (int m = 0; m < 8; ++m) tot[m] = 0.f;
    for (int jb = 0; jb < W; jb += 32) {
        float acc[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[m] = 0.f;
        const int n = W - jb < 32 ? W - jb : 32;
        if (n == 32) {
#pragma unroll
            for (int j = 0; j < 32; j += 4) {
                const float4 ac = *reinterpret_cast<const float4 *>(pa + jb + j), bn = *reinterpret_cast<const float4 *>(pb + jb + j + 4);
                const float A[8] = {ap.x, ap.y, ap.z, ap.w, ac.x, ac.y, ac.z, ac.w};      // A[4 + i] = pa[jb + j + i]
                const float Bv[8] = {bc.x, bc.y, bc.z, bc.w, bn.x, bn.y, bn.z, bn.w};     // Bv[i] = pb[jb + j + i]
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int m = 0; m < 8; ++m) {
                        const float v = A[4 + i - (m >> 1)] - Bv[i + ((m + 1) >> 1)];
                        acc[m] = fmaf(v, v, acc[m]);
                    }
                }
                ap = ac, bc = bn;
            }
        } else {
            for (int j = 0; j < n; ++j) {                                    // the last block, one sample at a time (W no multiple of 32)
                const float a = pa[jb + j], b4 = pb[jb + j + 4];
                const float A[4] = {a, ap.w, ap.z, ap.y}, Bv[5] = {bc.x, bc.y, bc.z, bc.w, b4};
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    const float v = A[m >> 1] - Bv[(m + 1) >> 1];
                    acc[m] = fmaf(v, v, acc[m]);
                }
                ap = make_float4(ap.y, ap.z, ap.w, a), bc = make_float4(bc.y, bc.z, bc.w, b4);
            }
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) tot[m] += acc[m];
    }
}

// step 5 of f6: the parabola through d'(lag - 1 .. lag + 1) and the frequency of its minimum
__device__ __forceinline__ float yin_hz(const float *d, int lag, int sr) {
    const float y0 = d[lag - 1], y1 = d[lag], y2 = d[lag + 1], den = y0 - 2.f * y1 + y2;
    const float off = den > 0.f ? fminf(fmaxf(0.5f * (y0 - y2) / den, -0.5f), 0.5f) : 0.f;
    return (float)sr / ((float)lag + off);
}

// CAND = false: vs_f0_yin (steps 3 - 5 of f6 on the d' row).  CAND = true: vs_f0_candidates (f12: the local minima of the same row below the gate).  Everything up
// to the energy of step 4 is the same code in the same order: a frame's d' row holds the same bits in both.
template <bool CAND>
__global__ void __launch_bounds__(YIN_THREADS) yin_kernel(const YinArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *img0 = lds, *dp = lds + p.K * p.n_img;                                         // K images of n_img floats, then d / d' rows [F][DP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long t0 = (long long)blockIdx.x * p.F;
    const int n_stage = (p.F - 1) * p.hop + 8 * p.G + p.W;                                // (<= n_img, by the host's choice of F)
    const int step = 4 / p.K;                                                             // image q holds the span shifted by q * step samples
    for (long long row = blockIdx.y; row < p.B; row += gridDim.y) {
        long long len = p.lengths ? p.lengths[row] : p.L;
        len = len < 0 ? 0 : (len > p.L ? p.L : len);
        long long n_b = len / p.hop;
        n_b = n_b < p.T ? n_b : p.T;
        const int nf = (int)(n_b - t0 < 0 ? 0 : (n_b - t0 < p.F ? n_b - t0 : p.F));       // frames of this workgroup inside the row
        if constexpr (CAND) {                                                             // ... and beyond it: every slot empty
            const long long te = t0 + p.F < p.T ? t0 + p.F : p.T;
            for (long long i = (t0 + nf) * 8 + tid; i < te * 8; i += YIN_THREADS) {
                p.cand_hz[row * p.T * 8 + i] = 0.f;
                p.cand_d[row * p.T * 8 + i] = 1.f;
            }
        } else {
            for (long long t = t0 + nf + tid; t < t0 + p.F && t < p.T; t += YIN_THREADS) {   // ... and beyond it
                p.f0[row * p.T + t] = 0.f;
                if (p.per) p.per[row * p.T + t] = 0.f;
            }
        }
        if (nf == 0) continue;                                                            // (uniform over the workgroup)
        const long long base0 = t0 * p.hop + p.hop / 2 - p.W / 2, lo = base0 - 4 * p.G;  // x[base0] sits at index 4G of image 0
        const float *src = p.wav + row * p.L;
        for (int i = tid; i < n_stage; i += YIN_THREADS) {
            const long long s = lo + i;
            const float v = (s >= 0 && s < len) ? src[s] : 0.f;
            for (int q = 0; q < p.K; ++q)
                if (i >= q * step) img0[q * p.n_img + i - q * step] = v;                  // image q: [i] = x[lo + q * step + i]
        }
        __syncthreads();
        for (int item = tid; item < nf * p.G; item += YIN_THREADS) {
            const int f = item / p.G, g = item - f * p.G;
            const int rel = 4 * p.G + f * p.hop;                                          // index of x[base_f] in image 0; (rel & 3) / step: its image
            float tot[8];
            yin_lag8(img0 + ((rel & 3) / step) * p.n_img, rel & ~3, g, p.W, tot);
            float4 *d = reinterpret_cast<float4 *>(dp + f * p.DP + 8 * g);                // (slot 0 holds d(0) = 0 and is never read)
            d[0] = make_float4(tot[0], tot[1], tot[2], tot[3]), d[1] = make_float4(tot[4], tot[5], tot[6], tot[7]);
        }
        __syncthreads();
        // the tail, one wave per frame.  S(tau) = E_l + P: lane l = (tau - 1) / 17 adds d(17 l + 1) .. d(tau) ascending into P (from 0), E_l = the sum of the
        // lanes' totals below l, formed by the doubling scan v += shfl_up(v, 1, 2, 4, .., 32) and shifted down by one lane.
        for (int f0 = 0; f0 < p.F; f0 += YIN_THREADS / 64) {
            const int f = f0 + wave;
            const bool live = f < nf;
            float *d = dp + (live ? f : 0) * p.DP;
            const int last = p.tau_max + 1;
            float loc[YIN_SCAN], run = 0.f;
#pragma unroll
            for (int k = 0; k < YIN_SCAN; ++k) {
                const int tau = YIN_SCAN * lane + 1 + k;
                run += (live && tau <= last) ? d[tau] : 0.f;
                loc[k] = run;
            }
            float inc = run;
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                const float o = __shfl_up(inc, s);
                if (lane >= s) inc += o;
            }
            float exc = __shfl_up(inc, 1);
            if (lane == 0) exc = 0.f;
#pragma unroll                                                                            // (a lane overwrites the lags it has read itself)
            for (int k = 0; k < YIN_SCAN; ++k) {
                const int tau = YIN_SCAN * lane + 1 + k;
                if (live && tau <= last) {
                    const float S = exc + loc[k], dv = d[tau];
                    d[tau] = (S > 0.f && S < INFINITY) ? dv * (float)tau / S : 1.f;
                }
            }
            __syncthreads();                                                              // (the wave's d' row is complete)
            if (!live) continue;                                                          // (no barrier below)
            const long long t = t0 + f;
            // energy of the frame's window: lane l adds x^2 over j = l, l + 64, .. ascending (fmaf from 0), then the butterfly e += shfl_xor(e, 32, 16, .., 1)
            const int rel = 4 * p.G + f * p.hop;
            float e = 0.f;
            for (int j = lane; j < p.W; j += 64) {
                const float v = img0[rel + j];
                e = fmaf(v, v, e);
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) e += __shfl_xor(e, s);
            if constexpr (CAND) {
                // the lags tau with d'(tau - 1) > d'(tau) <= d'(tau + 1) (tau_min needs no left neighbour) and d'(tau) < gate, ascending: a ballot per 64 lags,
                // a candidate's slot = the count so far + the candidates in the lanes below it.  Slots 0 .. 6; the rest, slot 7 included, are empty.
                float *ch = p.cand_hz + (row * p.T + t) * 8, *cd = p.cand_d + (row * p.T + t) * 8;
                int count = 0;
                if (fabsf(e) < INFINITY && e > p.silence_w) {
                    for (int tau0 = p.tau_min; tau0 <= p.tau_max && count < 7; tau0 += 64) {
                        const int tau = tau0 + lane;
                        bool c = false;
                        float v = 1.f;
                        if (tau <= p.tau_max) {
                            v = d[tau];
                            c = v < p.thr && v <= d[tau + 1] && (tau == p.tau_min || d[tau - 1] > v);
                        }
                        const unsigned long long m = __ballot(c);
                        const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
                        if (c && slot < 7) {
                            ch[slot] = yin_hz(d, tau, p.sr);
                            cd[slot] = v;
                        }
                        count += __popcll(m);
                    }
                    count = count < 7 ? count : 7;
                }
                if (lane >= count && lane < 8) {
                    ch[lane] = 0.f;
                    cd[lane] = 1.f;
                }
                continue;
            }
            // g = argmin of d' over [tau_min, tau_max], the lowest tau on a tie
            float best = INFINITY;
            int arg = p.tau_max;
            for (int tau = p.tau_min + lane; tau <= p.tau_max; tau += 64) {
                const float v = d[tau];
                if (v < best) best = v, arg = tau;
            }
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const float ov = __shfl_xor(best, s);
                const int oa = __shfl_xor(arg, s);
                if (ov < best || (ov == best && oa < arg)) best = ov, arg = oa;
            }
            float per = fminf(fmaxf(1.f - best, 0.f), 1.f), hz = 0.f;
            if (!(fabsf(e) < INFINITY)) {
                per = 0.f;
            } else if (e > p.silence_w) {
                int lag = 0;                                                              // the first tau below thr ...
                for (int tau0 = p.tau_min; tau0 <= p.tau_max && !lag; tau0 += 64) {
                    const int tau = tau0 + lane;
                    const unsigned long long m = __ballot(tau <= p.tau_max && d[tau] < p.thr);
                    if (m) lag = tau0 + __builtin_ctzll(m);
                }
                if (lag) {
                    while (lag + 1 <= p.tau_max && d[lag + 1] < d[lag]) ++lag;            // ... then down to the bottom of its dip
                    hz = yin_hz(d, lag, p.sr);
                }
            }
            if (lane == 0) {
                p.f0[row * p.T + t] = hz;
                if (p.per) p.per[row * p.T + t] = per;
            }
        }
        __syncthreads();                                                                  // (the next row restages the images)
    }
}

}  // namespace vs

using namespace vs;

// the checks and the launch shape the two entry points share; `what`: "threshold" or "gate"
static int yin_setup(const char *who, const char *what, int64_t B, int64_t L, int sr, int hop, float f0_min, float f0_max, int window, float threshold,
                     float silence, int64_t T, YinArgs &a, size_t &lds_bytes) {
    VS_REQUIRE(B > 0 && L > 0 && T > 0, "%s: B, L, T must be positive (got %lld, %lld, %lld)", who, (long long)B, (long long)L, (long long)T);
    VS_REQUIRE(L < (1ll << 31) && T < (1ll << 31) && B <= INT64_MAX / T && B <= INT64_MAX / L, "%s: L = %lld or T = %lld is not below 2^31, or B * L / B * T is out of range",
               who, (long long)L, (long long)T);
    VS_REQUIRE(hop >= 1 && sr >= 1, "%s: hop = %d and sr = %d must be at least 1", who, hop, sr);
    VS_REQUIRE(f0_min > 0.f && f0_min < INFINITY && f0_max > 0.f && f0_max < INFINITY && f0_min < f0_max,
               "%s: 0 < f0_min < f0_max < inf is required (got %g, %g)", who, (double)f0_min, (double)f0_max);
    VS_REQUIRE(threshold > 0.f && threshold < INFINITY, "%s: %s = %g is not a finite number > 0", who, what, (double)threshold);
    VS_REQUIRE(silence >= 0.f, "%s: silence = %g is negative (or NaN)", who, (double)silence);
    const double tmax_d = std::ceil((double)sr / (double)f0_min), tmin_d = std::floor((double)sr / (double)f0_max);
    VS_REQUIRE(tmax_d <= YIN_MAX_TAU, "%s: tau_max = ceil(sr / f0_min) = %.0f exceeds %d", who, tmax_d, YIN_MAX_TAU);
    const int tau_max = (int)tmax_d, tau_min = tmin_d < 2 ? 2 : (int)tmin_d;
    VS_REQUIRE(tau_min < tau_max, "%s: tau_min = %d is not below tau_max = %d", who, tau_min, tau_max);
    const int W = window == 0 ? 2 * tau_max : window;
    VS_REQUIRE(W >= tau_max && W <= YIN_MAX_W, "%s: window = %d is not in [tau_max = %d, %d]", who, W, tau_max, YIN_MAX_W);
    a.B = B, a.L = L, a.T = T, a.sr = sr, a.hop = hop, a.W = W, a.tau_min = tau_min, a.tau_max = tau_max;
    a.G = (tau_max + 2 + 7) / 8;                                                  // lags 0 .. tau_max + 1 in groups of eight
    a.DP = 8 * a.G;
    a.K = (hop & 1) ? 4 : ((hop & 2) ? 2 : 1);                                    // the shifts (f * hop) & 3 that occur
    a.thr = threshold, a.silence_w = silence * (float)W;
    // frames per workgroup (the result does not depend on it): among those whose span fits the LDS, at most 8 and at most T, the count that leaves the fewest
    // of the 256 lanes idle over the passes of the (frame, lag group) items; the larger on a tie.  One frame always fits.
    const long long one = 8ll * a.G + W;
    int F = 1;
    double best = 0.;
    for (int f = 1; f <= YIN_MAX_F && f <= T; ++f) {
        const long long n_img = (one + (long long)(f - 1) * hop + 3) & ~3ll;
        if (f > 1 && a.K * n_img + (long long)f * a.DP > YIN_LDS_FLOATS) break;
        const int items = f * a.G;
        const double use = (double)items / (double)(YIN_THREADS * ((items + YIN_THREADS - 1) / YIN_THREADS));
        if (use >= best) best = use, F = f;
    }
    a.F = F;
    a.n_img = (int)((one + (long long)(F - 1) * hop + 3) & ~3ll);
    lds_bytes = sizeof(float) * ((size_t)a.K * a.n_img + (size_t)F * a.DP);
    return VS_OK;
}

extern "C" {

int vs_f0_yin(const float *wav, const int64_t *lengths, int64_t B, int64_t L, int sr, int hop, float f0_min, float f0_max, int window, float threshold,
              float silence, float *f0_hz, float *periodicity, int64_t T, void *stream) {
    VS_REQUIRE(wav && f0_hz, "vs_f0_yin: wav and f0_hz must not be NULL");
    VS_REQUIRE(wav != f0_hz && wav != periodicity && f0_hz != periodicity && (const void *)lengths != (const void *)f0_hz &&
                   (!lengths || (const void *)lengths != (const void *)periodicity),
               "vs_f0_yin: wav, lengths, f0_hz and periodicity must be distinct buffers");
    YinArgs a;
    size_t lds_bytes;
    VS_TRY(yin_setup("vs_f0_yin", "threshold", B, L, sr, hop, f0_min, f0_max, window, threshold, silence, T, a, lds_bytes));
    a.wav = wav, a.lengths = (const long long *)lengths, a.f0 = f0_hz, a.per = periodicity, a.cand_hz = a.cand_d = nullptr;
    hipLaunchKernelGGL(yin_kernel<false>, dim3((unsigned)ceil_div(T, a.F), (unsigned)(B < 65535 ? B : 65535)), dim3(YIN_THREADS), lds_bytes, as_stream(stream), a);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

int vs_f0_candidates(const float *wav, const int64_t *lengths, int64_t B, int64_t L, int sr, int hop, float f0_min, float f0_max, int window, float gate,
                     float silence, float *cand_hz, float *cand_d, int64_t T, void *stream) {
    VS_REQUIRE(wav && cand_hz && cand_d, "vs_f0_candidates: wav, cand_hz and cand_d must not be NULL");
    VS_REQUIRE(wav != cand_hz && wav != cand_d && cand_hz != cand_d && (const void *)lengths != (const void *)cand_hz && (const void *)lengths != (const void *)cand_d,
               "vs_f0_candidates: wav, lengths, cand_hz and cand_d must be distinct buffers");
    YinArgs a;
    size_t lds_bytes;
    VS_TRY(yin_setup("vs_f0_candidates", "gate", B, L, sr, hop, f0_min, f0_max, window, gate, silence, T, a, lds_bytes));
    VS_REQUIRE(B <= INT64_MAX / T / 8, "vs_f0_candidates: B * T * 8 is out of range (B = %lld, T = %lld)", (long long)B, (long long)T);
    a.wav = wav, a.lengths = (const long long *)lengths, a.f0 = a.per = nullptr, a.cand_hz = cand_hz, a.cand_d = cand_d;
    hipLaunchKernelGGL(yin_kernel<true>, dim3((unsigned)ceil_div(T, a.F), (unsigned)(B < 65535 ? B : 65535)), dim3(YIN_THREADS), lds_bytes, as_stream(stream), a);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
