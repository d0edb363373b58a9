// sample_ops.hip -- seeded per-item normal noise and the reparameterised prior sample of the synthesis path in ONE launch
// (models/visinger.py:107  z_p = (mu_p + randn_like(mu_p) * exp(logs_p)) * frame_mask: randn_like + exp + mul + add + mul, five aten launches
// plus the generator's Philox bookkeeping).  No reference counterpart for the stream: torch's generator ties a value to the batch it was drawn in;
// here a value depends on (item seed, take, channel, frame) only, so an item's noise is the same in any batch, row, padding or number of takes.
//   stream (DESIGN.md "Seeded sampling"): Philox4x32-10 (Random123 constants), key = (seed low word, seed high word), counter =
//   (frame t, channel quad c >> 2, take, 0); one call gives the four channels 4q .. 4q + 3 of frame t by two Box-Muller pairs:
//   u1 = ((x >> 8) + 1) 2^-24 in (0, 1], u2 = (y >> 8) 2^-24 in [0, 1), n = sqrt(-2 ln u1) (cos, sin)(2 pi u2);  |n| <= sqrt(48 ln 2) = 5.77.
// One lane per (channel quad, frame), lanes along t: every global access is a coalesced dword row segment for any T.  HBM-bound (12 B per
// output element against ~100 integer operations per four); precise logf / sqrtf / expf / sincospif (the test bar is derived from them).
#include "vs_internal.h"

namespace vs {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&x)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float &n0, float &n1) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;      // (0, 1]: both conversions exact
    const float u2x2 = (float)(b >> 8) * 0x1p-23f;            // 2 u2 in [0, 2)
    const float r = sqrtf(-2.f * logf(u1));
    float s, c;
    sincospif(u2x2, &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// PRIOR = false: out[row, c, t] = n.  PRIOR = true: out = z = (mu + noise_scale n exp(logs)) mask, eps (optional) = n.
// grid: (frame blocks of 256, channel quads, rows b * K + k); the y / z extents are walked with a stride where they exceed the grid limits.
template <bool PRIOR>
__global__ void __launch_bounds__(256) sample_kernel(const long long *__restrict__ seeds, unsigned take0, long long K, const float *__restrict__ mu,
                                                     const float *__restrict__ logs, long long stat_bs, const float *__restrict__ mask,
                                                     float noise_scale, float *__restrict__ out, float *__restrict__ eps, long long rows,
                                                     int H, long long T) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int quads = (H + 3) >> 2;
    for (long long row = blockIdx.z; row < rows; row += gridDim.z) {
        const long long b = row / K;
        const unsigned take = take0 + (unsigned)(row - b * K);
        const unsigned long long seed = (unsigned long long)seeds[b];
        float m = 1.f;
        if (PRIOR && mask) m = mask[b * T + t];
        for (int q = blockIdx.y; q < quads; q += gridDim.y) {
            const int c0 = q * 4;
            float *o = out + (row * H + c0) * T + t;
            if (PRIOR && !eps && m == 0.f) {       // a masked frame is exactly 0 whatever the statistics hold: no draw needed
                for (int i = 0; i < 4 && c0 + i < H; ++i) o[(long long)i * T] = 0.f;
                continue;
            }
            unsigned x[4];
            philox4x32_10((unsigned)t, (unsigned)q, take, 0u, (unsigned)seed, (unsigned)(seed >> 32), x);
            float n[4];
            box_muller(x[0], x[1], n[0], n[1]);
            box_muller(x[2], x[3], n[2], n[3]);
            if (!PRIOR) {
                for (int i = 0; i < 4 && c0 + i < H; ++i) o[(long long)i * T] = n[i];
            } else {
                const long long so = b * stat_bs + (long long)c0 * T + t;
                float *e = eps ? eps + (row * H + c0) * T + t : nullptr;
                for (int i = 0; i < 4 && c0 + i < H; ++i) {
                    const float z = mu[so + (long long)i * T] + (noise_scale * n[i]) * expf(logs[so + (long long)i * T]);
                    o[(long long)i * T] = m == 0.f ? 0.f : z * m;
                    if (e) e[(long long)i * T] = n[i];
                }
            }
        }
    }
}

static int check_stream_args(const char *fn, const void *seeds, const void *out, int64_t take0, int64_t K, int64_t B, int64_t H, int64_t T) {
    VS_REQUIRE(seeds && out, "%s: seeds and the output must not be NULL", fn);
    VS_REQUIRE(B > 0 && H > 0 && T > 0, "%s: B, H, T must be positive (got %lld, %lld, %lld)", fn, (long long)B, (long long)H, (long long)T);
    VS_REQUIRE(K >= 1, "%s: K (takes) must be >= 1 (got %lld)", fn, (long long)K);
    VS_REQUIRE(take0 >= 0, "%s: take0 must be >= 0 (got %lld)", fn, (long long)take0);
    VS_REQUIRE(take0 <= (1ll << 32) && K <= (1ll << 32) - take0, "%s: take0 + K exceeds 2^32 (the take word of the counter)", fn);
    VS_REQUIRE(T <= (1ll << 32), "%s: T exceeds 2^32 (the frame word of the counter)", fn);
    VS_REQUIRE(H <= 0x7fffffff - 3 && B <= INT64_MAX / K, "%s: H or B * K out of range", fn);
    return VS_OK;
}

template <bool PRIOR>
static int launch(const long long *seeds, int64_t take0, int64_t K, const float *mu, const float *logs, int64_t stat_bs, const float *mask,
                  float noise_scale, float *out, float *eps, int64_t B, int64_t H, int64_t T, void *stream) {
    const int64_t rows = B * K, quads = ceil_div(H, 4);
    dim3 grid((unsigned)ceil_div(T, 256), (unsigned)(quads < 65535 ? quads : 65535), (unsigned)(rows < 65535 ? rows : 65535));
    hipLaunchKernelGGL(sample_kernel<PRIOR>, grid, dim3(256), 0, as_stream(stream), seeds, (unsigned)take0, (long long)K, mu, logs, (long long)stat_bs,
                       mask, noise_scale, out, eps, (long long)rows, (int)H, (long long)T);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_normal_fill(const int64_t *seeds, int64_t take0, int64_t K, float *out, int64_t B, int64_t H, int64_t T, void *stream) {
    VS_TRY(check_stream_args("vs_normal_fill", seeds, out, take0, K, B, H, T));
    return launch<false>((const long long *)seeds, take0, K, nullptr, nullptr, 0, nullptr, 1.f, out, nullptr, B, H, T, stream);
}

int vs_prior_sample(const float *mu, const float *logs, int64_t stat_batch_stride, const float *mask, const int64_t *seeds, int64_t take0,
                    int64_t K, float noise_scale, float *z, float *eps_out, int64_t B, int64_t H, int64_t T, void *stream) {
    VS_TRY(check_stream_args("vs_prior_sample", seeds, z, take0, K, B, H, T));
    VS_REQUIRE(mu && logs, "vs_prior_sample: mu and logs must not be NULL");
    VS_REQUIRE(H <= INT64_MAX / T && stat_batch_stride >= H * T, "vs_prior_sample: stat_batch_stride %lld is below H * T (rows of one item overlap the next)",
               (long long)stat_batch_stride);
    return launch<true>((const long long *)seeds, take0, K, mu, logs, stat_batch_stride, mask, noise_scale, z, eps_out, B, H, T, stream);
}

}  // extern "C"
