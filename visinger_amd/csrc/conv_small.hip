// conv_small.hip -- the two convs that leave the MFMA tiles: the VALU kernel for at most 4 output channels and the single-frame
// 1 x 1 kernel.  Each has a predicate over the handle and the filled launch parameters, and a launcher.
#include "conv_common.h"

#include <algorithm>

namespace vs {

// ---------------------------------------------------------------------------------------------------------------
// Convs with <= 4 output channels (HiFi-GAN conv_post 32->1 k7 + tanh, decoder.py:34,55-57; PitchPredictor.linear
// 192->2, predictor.py:14): a 32-row MFMA tile would be 97 % padding (measured 1.7 ms for conv_post at 2 TFLOP/s),
// and the op is a pure HBM stream of its input (1.07 GB for conv_post), so it runs on the VALU: one thread per
// 4 consecutive output frames, weights through the scalar cache, x re-read across taps through L1.
struct SmallParams {
    const float *x;
    long long x_bs;
    const float *w;      // effective weights [c_out][c_in][k]
    const float *bias;   // [c_out] or null
    const float *bias_b;
    long long bias_b_bs;
    const float *mask;   // [B, T]
    float *y;
    long long y_bs;
    int B, Cin, Cout, Tin, Tout, K, dil, pad, in_act, out_act, out_mask;
    float scale;
    int x_bf16;          // x holds bf16 elements (bf16-resident activations: the generator's last stage in BASELINE config 5); x_bs in elements
};

// ---------------------------------------------------------------------------------------------------------------
// 1 x 1 convs over ONE frame per item (the conditioning vectors: WN.cond_layer 256 -> 2 * hidden * n_layers on the speaker embedding,
// modules/visinger/wavenet.py cond_layer; the g-convs of the flow and the generator, decoder.py:38-39): y[b][m] = bias[m] + sum_c W[m][c] x[b][c].
// On the tile kernels the items are grid.z and the time axis the tile's columns -- one valid column in 128 or 256, a full K loop per
// item and row tile: 63 us for 256 -> 1536 at B = 32 (tools/conv_census.py, round 6).  Here a workgroup takes one 32-row tile of W for up
// to 32 items: x staged once in LDS (zero-padded to the chunk grid), the weights read straight from the fp32 fragment buffer Wp (lane =
// row: consecutive rows are consecutive float4s), fp32 FMAs; VS_MATH_BF16 rounds both operands to bf16 first, as its matrix kernels do.
struct T1Params {
    const float *x;
    long long x_bs;
    const float *wp;     // Wp[m_tile][chunk][quad(2)][64][4] (k = 1: one tap)
    const float *biasp;  // packed bias [MT_alloc * 32]
    const float *bias_b;
    long long bias_b_bs;
    float *y;
    long long y_bs;
    int B, Cin, c_out, nchunks, bf16;
    float scale;
};
__global__ void __launch_bounds__(256) conv_t1_kernel(const T1Params p) {
    extern __shared__ __attribute__((aligned(16))) float t1_xs[];       // [items of this workgroup][nchunks * 16]
    const int tid = threadIdx.x, row = tid & 31, bg = tid >> 5;
    const int mt = blockIdx.x, b0 = blockIdx.y * 32;
    const int nb = min(32, p.B - b0), CP = p.nchunks * 16;
    // (sixteen loads per thread in flight, unconditional on clamped indices: one load per loop trip was 32 round trips to a cold L2, 22 of the
    //  launch's 27 us)
    for (int e0 = 0; e0 < nb * CP; e0 += 256 * 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = min(e0 + tid + 256 * u, nb * CP - 1), bi = e / CP, c = e - bi * CP;
            v[u] = p.x[(long long)(b0 + bi) * p.x_bs + min(c, p.Cin - 1)];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = e0 + tid + 256 * u;
            if (e < nb * CP) {
                float t = (e % CP < p.Cin) ? v[u] : 0.f;
                if (p.bf16) t = u2f(rne_bf16(t) & 0xffff0000u);
                t1_xs[e] = t;
            }
        }
    }
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float4 *w = reinterpret_cast<const float4 *>(p.wp) + (long long)mt * p.nchunks * 128;
    // the weights of eight chunks are requested before any is used: the launch is a few dozen workgroups, each a chain of loads from a cold L2
    for (int c0 = 0; c0 < p.nchunks; c0 += 8) {
        float4 wq[8][4];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 *wc = w + min(c0 + u, p.nchunks - 1) * 128;
            wq[u][0] = wc[row]; wq[u][1] = wc[row + 32]; wq[u][2] = wc[64 + row]; wq[u][3] = wc[64 + row + 32];      // (quad, parity): channels 8 quad + 2 i + parity
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (c0 + u < p.nchunks) {
                if (p.bf16) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        wq[u][t].x = u2f(rne_bf16(wq[u][t].x) & 0xffff0000u); wq[u][t].y = u2f(rne_bf16(wq[u][t].y) & 0xffff0000u);
                        wq[u][t].z = u2f(rne_bf16(wq[u][t].z) & 0xffff0000u); wq[u][t].w = u2f(rne_bf16(wq[u][t].w) & 0xffff0000u);
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int bi = bg + 8 * i;
                    if (bi < nb) {
                        const float4 *xv = reinterpret_cast<const float4 *>(t1_xs + bi * CP + (c0 + u) * 16);
                        const float4 x0 = xv[0], x1 = xv[1], x2 = xv[2], x3 = xv[3];
                        float a = 0.f;                                     // (a chunk's sixteen products first, then onto the running sum: shorter rounding chains)
                        a += wq[u][0].x * x0.x; a += wq[u][1].x * x0.y; a += wq[u][0].y * x0.z; a += wq[u][1].y * x0.w;
                        a += wq[u][0].z * x1.x; a += wq[u][1].z * x1.y; a += wq[u][0].w * x1.z; a += wq[u][1].w * x1.w;
                        a += wq[u][2].x * x2.x; a += wq[u][3].x * x2.y; a += wq[u][2].y * x2.z; a += wq[u][3].y * x2.w;
                        a += wq[u][2].z * x3.x; a += wq[u][3].z * x3.y; a += wq[u][2].w * x3.z; a += wq[u][3].w * x3.w;
                        acc[i] += a;
                    }
                }
            }
        }
    }
    const int m = mt * 32 + row;
    if (m >= p.c_out) return;
    const float bias = p.biasp[m];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int bi = bg + 8 * i;
        if (bi < nb) {
            float v = acc[i] + bias;
            if (p.bias_b) v += p.bias_b[(long long)(b0 + bi) * p.bias_b_bs + m];
            p.y[(long long)(b0 + bi) * p.y_bs + m] = v * p.scale;
        }
    }
}

// KT > 0: compile-time taps KT and padding PAD (PAD <= 4, KT-1-PAD <= 4), dilation 1, T % 4 == 0, 16-B aligned rows: each thread
// produces 4 consecutive frames from three aligned float4 loads per input channel (its own 16 bytes, coalesced, plus
// its two neighbours' through L1), activates every value once and keeps the window in registers for all taps.
// KT == 0: generic runtime taps / dilation / alignment, one scalar load per (tap, frame).
template <int COUT, int KT, int PAD>
__global__ void __launch_bounds__(256) conv_small_kernel(const SmallParams p) {
    constexpr int NQ = 4;
    const int b = blockIdx.y;
    const int n0 = (blockIdx.x * 256 + threadIdx.x) * NQ;
    if (n0 >= p.Tout) return;
    const float *xb = p.x + (long long)b * p.x_bs;
    const unsigned short *xh = reinterpret_cast<const unsigned short *>(p.x) + (long long)b * p.x_bs;     // the same rows as bf16 elements
    const bool xbf = p.x_bf16 != 0;
    const float *mb = p.mask ? p.mask + (long long)b * p.Tin : nullptr;
    const bool act_lrelu = (p.in_act == VS_IN_LRELU || p.in_act == VS_IN_LRELU_MASK);
    const bool act_mask = (p.in_act >= VS_IN_MASK);
    float acc[COUT][NQ];
#pragma unroll
    for (int c = 0; c < COUT; ++c)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[c][q] = 0.f;
    if constexpr (KT > 0) {
        // window = frames n0-4 .. n0+7 ; frame n0 + q + k - pad is window[q + k - pad + 4]
        const bool okl = (n0 >= 4), okr = (n0 + 8 <= p.Tin);
        const int nl = okl ? n0 - 4 : n0, nr = okr ? n0 + 4 : n0;
        float mw[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) mw[i] = 1.f;
        if (act_mask) {
            const float4 a = *reinterpret_cast<const float4 *>(mb + nl), c4 = *reinterpret_cast<const float4 *>(mb + n0),
                         d = *reinterpret_cast<const float4 *>(mb + nr);
            mw[0] = a.x; mw[1] = a.y; mw[2] = a.z; mw[3] = a.w; mw[4] = c4.x; mw[5] = c4.y; mw[6] = c4.z; mw[7] = c4.w;
            mw[8] = d.x; mw[9] = d.y; mw[10] = d.z; mw[11] = d.w;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) { mw[i] = okl ? mw[i] : 0.f; mw[8 + i] = okr ? mw[8 + i] : 0.f; }
        for (int ci = 0; ci < p.Cin; ++ci) {
            const float *xr = xb + (long long)ci * p.Tin;
            float4 a, c4, d;
            if (xbf) {
                const unsigned short *xq = xh + (long long)ci * p.Tin;
                a = bf4_to_f4(*reinterpret_cast<const uint2 *>(xq + nl));
                c4 = bf4_to_f4(*reinterpret_cast<const uint2 *>(xq + n0));
                d = bf4_to_f4(*reinterpret_cast<const uint2 *>(xq + nr));
            } else {
                a = *reinterpret_cast<const float4 *>(xr + nl);
                c4 = *reinterpret_cast<const float4 *>(xr + n0);
                d = *reinterpret_cast<const float4 *>(xr + nr);
            }
            float xw[12] = {a.x, a.y, a.z, a.w, c4.x, c4.y, c4.z, c4.w, d.x, d.y, d.z, d.w};
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                float v = xw[i];
                if (act_lrelu) v = lrelu(v);
                xw[i] = v * mw[i];
            }
#pragma unroll
            for (int c = 0; c < COUT; ++c) {
#pragma unroll
                for (int k = 0; k < KT; ++k) {
                    const float wv = (c < p.Cout) ? p.w[((long long)c * p.Cin + ci) * KT + k] : 0.f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[c][q] += wv * xw[q + k - PAD + 4];
                }
            }
        }
    } else {
        for (int ci = 0; ci < p.Cin; ++ci) {
            const float *xr = xb + (long long)ci * p.Tin;
            for (int k = 0; k < p.K; ++k) {
                const int off = k * p.dil - p.pad;
                float xv[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int n = n0 + q + off;
                    const bool ok = (n >= 0 && n < p.Tin);
                    float v = ok ? (xbf ? u2f((unsigned)(xh + (long long)ci * p.Tin)[n] << 16) : xr[n]) : 0.f;
                    if (act_lrelu) v = lrelu(v);
                    if (act_mask) v *= ok ? mb[n] : 0.f;
                    xv[q] = v;
                }
#pragma unroll
                for (int c = 0; c < COUT; ++c) {
                    const float wv = (c < p.Cout) ? p.w[((long long)c * p.Cin + ci) * p.K + k] : 0.f;
#pragma unroll
                    for (int q = 0; q < NQ; ++q) acc[c][q] += wv * xv[q];
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
        if (c < p.Cout) {
            float bv = p.bias ? p.bias[c] : 0.f;
            if (p.bias_b) bv += p.bias_b[(long long)b * p.bias_b_bs + c];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int n = n0 + q;
                if (n < p.Tout) {
                    float v = (acc[c][q] + bv) * p.scale;
                    if (p.out_act == VS_OUT_TANH) v = tanhf(v);
                    else if (p.out_act == VS_OUT_RELU) v = fmaxf(v, 0.f);
                    if (p.out_mask) v *= mb[n];
                    p.y[(long long)b * p.y_bs + (long long)c * p.Tout + n] = v;
                }
            }
        }
    }
}

// one plain LINEAR destination: no row split, no residual, no accumulate input (neither kernel here has an epilogue for them)
static bool plain_linear_out(const ConvParams &p) {
    return !p.split_row && !p.out[0].res && !p.out[0].acc && p.out[0].mode == VS_OUT_LINEAR;
}

// (the VALU kernel reduces over c_in * k serially per thread: right for conv_post 32 -> 1 and the pitch head 192 -> 2, which
// stream a long input once; the discriminators' 1024 -> 1 conv_post over a few thousand positions needs the parallelism of
// the MFMA tiles even at 1 valid row in 32)
bool small_conv_applies(const vs_conv *h, const ConvParams &p) {
    return h->kind == VS_CONV1D && h->c_out <= 4 && h->c_in * h->k <= 2048 && !(h->flags & (VS_CONV_FLIP_IN | VS_CONV_FLIP_OUT | VS_CONV_ADJOINT)) &&
           !p.y_bf16 && plain_linear_out(p) && !opt(OPT_NO_SMALL_CONV);
}

int launch_small_conv(const vs_conv *h, const ConvParams &p, hipStream_t s) {
    SmallParams q;
    q.x = p.x; q.x_bs = p.x_bs; q.w = h->weff.as<float>(); q.bias = h->has_bias ? h->beff.as<float>() : nullptr;
    q.bias_b = p.bias_b; q.bias_b_bs = p.bias_b_bs; q.mask = p.mask; q.y = p.out[0].y; q.y_bs = p.out[0].y_bs;
    q.B = p.B; q.Cin = h->c_in; q.Cout = h->c_out; q.Tin = p.Tin; q.Tout = p.Tout; q.K = h->k; q.dil = h->dil;
    q.pad = h->pad; q.in_act = p.in_act; q.out_act = p.out[0].out_act; q.out_mask = p.out[0].out_mask;
    q.scale = p.out[0].scale;
    q.x_bf16 = p.x_bf16;
    dim3 grid((unsigned)ceil_div(p.Tout, 256 * 4), (unsigned)p.B);
    const bool vec_ok = (p.Tin % 4 == 0) && (p.Tout == p.Tin) && al16(q.x) && (q.x_bs % 4 == 0) && (!q.mask || al16(q.mask));
    const bool k7 = vec_ok && (h->k == 7 && h->dil == 1 && h->pad == 3), k1 = vec_ok && (h->k == 1 && h->pad == 0);
#define VS_SMALL(CO)                                                                                   \
    do {                                                                                               \
        if (k7) hipLaunchKernelGGL((conv_small_kernel<CO, 7, 3>), grid, dim3(256), 0, s, q);           \
        else if (k1) hipLaunchKernelGGL((conv_small_kernel<CO, 1, 0>), grid, dim3(256), 0, s, q);      \
        else hipLaunchKernelGGL((conv_small_kernel<CO, 0, 0>), grid, dim3(256), 0, s, q);              \
        set_last_kernel("conv_small_kernel<%d, %d, %d>", CO, k7 ? 7 : (k1 ? 1 : 0), k7 ? 3 : 0);       \
    } while (0)
    if (h->c_out == 1) VS_SMALL(1);
    else if (h->c_out == 2) VS_SMALL(2);
    else VS_SMALL(4);
#undef VS_SMALL
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

// one frame per item, k = 1 (conditioning vectors): conv_t1_kernel -- the tile kernels would compute one valid column in 128.
// (pad == 0: the kernel writes one frame per row; a padded 1 x 1 conv has 1 + 2 * pad of them)
bool t1_conv_applies(const vs_conv *h, const ConvParams &p) {
    return h->kind == VS_CONV1D && h->k == 1 && h->pad == 0 && p.Tin == 1 && h->flags == 0 && !p.x_bf16 && !p.y_bf16 && p.in_act == VS_IN_NONE &&
           plain_linear_out(p) && p.out[0].out_act == VS_OUT_NONE && !p.out[0].out_mask && h->nchunks * 16 * 32 * 4 <= 64 * 1024 && !opt(OPT_NO_T1_CONV);
}

int launch_t1_conv(const vs_conv *h, const ConvParams &p, hipStream_t s) {
    T1Params q;
    q.x = p.x; q.x_bs = p.x_bs; q.wp = h->wp.as<float>(); q.biasp = p.biasp; q.bias_b = p.bias_b; q.bias_b_bs = p.bias_b_bs;
    q.y = p.out[0].y; q.y_bs = p.out[0].y_bs; q.B = p.B; q.Cin = h->c_in; q.c_out = h->c_out; q.nchunks = h->nchunks;
    q.bf16 = (h->math == VS_MATH_BF16); q.scale = p.out[0].scale;
    const int nbmax = std::min(32, p.B);
    hipLaunchKernelGGL(conv_t1_kernel, dim3((unsigned)h->MT, (unsigned)ceil_div(p.B, 32)), dim3(256), (size_t)nbmax * h->nchunks * 16 * sizeof(float), s, q);
    VS_CHECK_HIP(hipGetLastError());
    set_last_kernel("conv_t1_kernel");
    return VS_OK;
}

}  // namespace vs
