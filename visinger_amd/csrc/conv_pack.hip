// conv_pack.hip -- binding weights to a conv handle: the weight-norm row scales, the pack of a weight into the fragment order of
// the conv kernels (fp32 fragments Wp, the planes Ws of the split engines through conv_split.hip, the F(2,3) transform), and the
// vs_conv_set_weights* entry points with the staging ring of the batch form.
#include "conv_common.h"

#include <algorithm>
#include <mutex>
#include <unordered_set>
#include <vector>

namespace vs {

// ---------------------------------------------------------------------------------------------------------------
// weight-norm row scales and packing

// scale[r] = g[r] / ||v[r, :]||_2 ; one wave per row
__global__ void rownorm_scale_kernel(const float *__restrict__ v, const float *__restrict__ g, float *__restrict__ scale,
                                     long long rows, long long cols) {
    const long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *vr = v + row * cols;
    float ss = 0.f;
    for (long long c = lane; c < cols; c += 64) ss += vr[c] * vr[c];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) ss += __shfl_xor(ss, s);
    if (lane == 0) scale[row] = g[row] / sqrtf(ss);
}

__global__ void weightnorm_apply_kernel(const float *__restrict__ v, const float *__restrict__ scale, float *__restrict__ w,
                                        long long rows, long long cols) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * cols) w[i] = v[i] * scale[i / cols];
}

struct PackParams {
    const float *w;      // source weight (or weight_v)
    const float *scale;  // per-dim0 scale (weight norm) or null
    const float *bias;   // source bias or null
    float *wp;
    float *biasp;
    int kind, c_in, c_out, k, up, pad, dmin, KT, CP, MT_alloc, Hh;
    unsigned flags;
    int wino_tail1;      // pack_wino_kernel: the single tap of the last group in the direct form (k = 7 specialised instances)
    unsigned *maxbits, *maxbits_clear;   // split-f16 arithmetic: largest |w| (bits) of this pack -> *maxbits; the other slot is zeroed for the next pack
};

// bias of virtual row m (rows past the real ones: 0)
__device__ __forceinline__ float packed_bias(const PackParams &q, int m) {
    int row = -1;
    if (q.kind == VS_CONV1D) {
        if (m < q.c_out) row = (q.flags & VS_CONV_FLIP_OUT) ? q.c_out - 1 - m : m;
    } else if (q.kind == VS_CONV1D_PAIRED) {
        const int pair = m >> 6, which = (m >> 5) & 1, c = pair * 32 + (m & 31);
        if (c < q.Hh) row = which * q.Hh + ((q.flags & VS_CONV_FLIP_OUT) ? q.Hh - 1 - c : c);
    } else {
        const int phase = m / q.c_out;
        if (phase < q.up) row = m - phase * q.c_out;
    }
    return (row >= 0 && q.bias) ? q.bias[row] : 0.f;
}

// The value of fragment element Wp[m_tile][tap][chunk][quad(2)][64 lanes][4]: lane l of quad qd holds channel pairs
// chunk*8 + qd*4 + (0..3), i.e. row m_tile*32 + (l & 31), (logical) input channel 2 * pair + (l >> 5)
__device__ __forceinline__ float packed_weight(const PackParams &q, int mt, int tap, int chunk, int quad, int lane, int sub) {
    const int cp = chunk * (CK / 2) + quad * 4 + sub;
    const int m = mt * 32 + (lane & 31);
    int ci = cp * 2 + (lane >> 5);
    float val = 0.f;
    if (ci < q.c_in) {
        if (q.flags & VS_CONV_FLIP_IN) ci = q.c_in - 1 - ci;
        if (q.kind == VS_CONV1D) {
            if (m < q.c_out) {
                const int row = (q.flags & VS_CONV_FLIP_OUT) ? q.c_out - 1 - m : m;
                val = (q.flags & VS_CONV_ADJOINT) ? q.w[((long long)ci * q.c_out + row) * q.k + (q.k - 1 - tap)]
                                                  : q.w[((long long)row * q.c_in + ci) * q.k + tap];
                if (q.scale) val *= q.scale[row];
            }
        } else if (q.kind == VS_CONV1D_PAIRED) {
            const int pair = mt >> 1, which = mt & 1, c = pair * 32 + (lane & 31);
            if (c < q.Hh) {
                const int row = which * q.Hh + ((q.flags & VS_CONV_FLIP_OUT) ? q.Hh - 1 - c : c);
                val = q.w[((long long)row * q.c_in + ci) * q.k + tap];
                if (q.scale) val *= q.scale[row];
            }
        } else {  // transposed: w is [c_in, c_out, k]; virtual row m = phase*c_out + co; tap <-> delta = dmin + tap
            const int phase = m / q.c_out;
            if (phase < q.up) {
                const int co = m - phase * q.c_out;
                const int kk = (q.dmin + tap) * q.up + phase + q.pad;
                if (kk >= 0 && kk < q.k) {
                    val = q.w[((long long)ci * q.c_out + co) * q.k + kk];
                    if (q.scale) val *= q.scale[ci];
                }
            }
        }
    }
    return val;
}

// blk of nblk: this block's place among the blocks that pack q (the whole grid of the one- and two-handle launches, a slice of it in the batch launch)
__device__ __forceinline__ void pack_conv_body(const PackParams &q, unsigned blk, unsigned nblk) {
    const long long total = (long long)q.MT_alloc * q.KT * q.CP * 64;
    const long long work = max(total, (long long)q.MT_alloc * 32);
    if (blk == 0 && threadIdx.x == 0 && q.maxbits_clear) *q.maxbits_clear = 0u;
    unsigned m = 0u;
    // grid-stride: at most 1024 blocks however large the weight (the largest |w| below is ONE atomic per block: tens of thousands of
    // same-address atomics -- the discriminators' 1024 x 1024 x 5 convs -- serialised into most of a millisecond per pack)
    for (long long e = (long long)blk * blockDim.x + threadIdx.x; e < work; e += (long long)nblk * blockDim.x) {
        if (e < (long long)q.MT_alloc * 32) q.biasp[e] = packed_bias(q, (int)e);   // bias over virtual rows
        if (e < total) {
            const int sub = (int)(e & 3);
            const int lane = (int)((e >> 2) & 63);
            const int quad = (int)((e >> 8) & 1);
            long long t = e >> 9;
            const int nchunks = q.CP / (CK / 2);
            const int chunk = (int)(t % nchunks);
            t /= nchunks;
            const int tap = (int)(t % q.KT);
            const int mt = (int)(t / q.KT);
            const float v = packed_weight(q, mt, tap, chunk, quad, lane, sub);
            q.wp[e] = v;
            m = f16_maxkey(m, v);      // (finite magnitudes only: a NaN / Inf weight must not set the scale)
        }
    }
    if (q.maxbits) {       // (uniform over the launch) the conv's largest weight, for the scale of the f16 planes
        __shared__ unsigned red[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) atomicMax(q.maxbits, max(max(red[0], red[1]), max(red[2], red[3])));
    }
}
__global__ void pack_conv_kernel(const PackParams q) { pack_conv_body(q, blockIdx.x, gridDim.x); }
// two handles fed from the same weight (a conv and the ADJOINT handle of its grad-input: vs_conv_set_weights_pair) in ONE launch:
// blockIdx.y selects the handle.  A training step packs every weight for both; two launches per handle were 1 068 of its 6 175.
__global__ void pack_conv_pair_kernel(const PackParams q0, const PackParams q1) {
    if (blockIdx.y == 0) pack_conv_body(q0, blockIdx.x, gridDim.x);
    else pack_conv_body(q1, blockIdx.x, gridDim.x);
}
// ANY number of handles in one launch (vs_conv_set_weights_batch: every conv of a network at the top of a training pass): the jobs and the first
// block of each (blk0[n] = the grid) come from a table in device memory; a block finds its job by bisection.
__global__ void pack_conv_multi_kernel(const PackParams *__restrict__ jobs, const unsigned *__restrict__ blk0, int n) {
    int lo = 0, hi = n - 1;
    const unsigned b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk0[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    const PackParams q = jobs[lo];
    pack_conv_body(q, b - blk0[lo], blk0[lo + 1] - blk0[lo]);
}

// The same pack for the bf16-pipe engine in ONE launch: thread (cell = (m_tile, tap, chunk), lane) produces the eight values of its bf16
// fragment (pack_split_kernel's mapping: row lane & 31, channels chunk*16 + 8*(lane >> 5) + j), writes them to the fp32 fragment buffer
// Wp (kept: vs_conv_set_math and the lazy F(2,3) transforms are built from it) and, split into planes, to Ws.  A training step re-packs
// every conv's weight twice (forward and grad-input handles): two launches per pack were 1 400 of its 7 000.
__global__ void pack_conv_split_kernel(const PackParams q, void *ws, int npl) {
    const int nchunks = q.CP / (CK / 2);
    const long long total = (long long)q.MT_alloc * q.KT * nchunks * 64;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (long long)q.MT_alloc * 32) q.biasp[e] = packed_bias(q, (int)e);
    if (e >= total) return;
    const int lane = (int)(e & 63);
    const long long cell = e >> 6;
    const int chunk = (int)(cell % nchunks);
    const int tap = (int)((cell / nchunks) % q.KT);
    const int mt = (int)(cell / ((long long)nchunks * q.KT));
    const int row = lane & 31, kg = lane >> 5;
    float *const wpc = q.wp + cell * 512;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int cl = 8 * kg + j, cp = cl >> 1, par = cl & 1;
        v[j] = packed_weight(q, mt, tap, chunk, cp >> 2, row + 32 * par, cp & 3);
        wpc[(cp >> 2) * 256 + (row + 32 * par) * 4 + (cp & 3)] = v[j];
    }
    u32x4 *dst = reinterpret_cast<u32x4 *>(ws) + cell * npl * 64 + lane;
    if (npl == 1) {
        unsigned d[4][1];
#pragma unroll
        for (int t = 0; t < 4; ++t) split_pair<1>(v[2 * t], v[2 * t + 1], d[t]);
        u32x4 o; o.x = d[0][0]; o.y = d[1][0]; o.z = d[2][0]; o.w = d[3][0];
        dst[0] = o;
    } else {
        unsigned d[4][3];
#pragma unroll
        for (int t = 0; t < 4; ++t) split_pair<3>(v[2 * t], v[2 * t + 1], d[t]);
        for (int pl = 0; pl < npl; ++pl) {
            u32x4 o; o.x = d[0][pl]; o.y = d[1][pl]; o.z = d[2][pl]; o.w = d[3][pl];
            dst[pl * 64] = o;
        }
    }
}

// Winograd F(2,3) weight transform + fragment packing for conv_wino_kernel:
//   Up[m_tile][chunk][group][half][ci_pair(4)][64 lanes][xi(4)], lane l <-> (row m_tile*32 + (l&31), ci = chunk*16 + half*8 +
//   2*ci_pair + (l>>5)); taps beyond k are zeros (the last group of k = 7 / 11 is partial).
__global__ void pack_wino_kernel(const PackParams q, int G, int nchunks) {
    const long long total = (long long)q.MT_alloc * nchunks * G * 2 * 16 * 64;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int xi = (int)(e & 3);
    const int lane = (int)((e >> 2) & 63);
    const int cp4 = (int)((e >> 8) & 3);
    long long t = e >> 10;
    const int half = (int)(t & 1);
    t >>= 1;
    const int g = (int)(t % G);
    t /= G;
    const int chunk = (int)(t % nchunks);
    const int mt = (int)(t / nchunks);
    const int ci = chunk * CK + half * 8 + cp4 * 2 + (lane >> 5);
    // built from the fp32 fragment buffer Wp (q.w), which already holds flips / weight-norm scale / adjoint and zeros in the padding:
    // the transform is made by the first launch that needs it (the bf16-pipe engine and the training path never do)
    auto wv = [&](int tap) -> float {
        const int cp = ci >> 1;
        return q.w[((((long long)mt * q.KT + tap) * nchunks + (cp >> 3)) * 2 + ((cp & 7) >> 2)) * 256 + ((ci & 1) * 32 + (lane & 31)) * 4 + (cp & 3)];
    };
    float val = 0.f;
    {
        const int k0 = 3 * g;
        const float w0 = (k0 < q.k) ? wv(k0) : 0.f;
        const float w1 = (k0 + 1 < q.k) ? wv(k0 + 1) : 0.f;
        const float w2 = (k0 + 2 < q.k) ? wv(k0 + 2) : 0.f;
        if (q.wino_tail1 && k0 + 1 == q.k) val = (xi == 0) ? w0 : (xi == 3) ? -w0 : 0.f;       // single last tap: direct form
        else if (q.wino_tail1 && k0 + 2 == q.k) val = (xi == 0) ? w0 : (xi == 1) ? (w0 + w1) : (xi == 3) ? w1 : 0.f;   // two: F(2,2)
        else val = (xi == 0) ? w0 : (xi == 1) ? 0.5f * (w0 + w1 + w2) : (xi == 2) ? 0.5f * (w0 - w1 + w2) : w2;
    }
    q.wp[e] = val;
}
// effective (weight-norm folded) weights in the reference layout, for the VALU path
__global__ void fold_weights_kernel(const float *__restrict__ w, const float *__restrict__ scale, float *__restrict__ out,
                                    long long rows, long long cols) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * cols) out[i] = scale ? w[i] * scale[i / cols] : w[i];
}

// ---------------------------------------------------------------------------------------------------------------
// what the vs_conv_set_weights* entry points (and the re-pack of vs_conv_set_math) share

static long long fragment_count(const vs_conv *h) { return (long long)h->MT_alloc * h->KT * h->CP * 64; }     // fp32 elements of Wp
static long long plane_cells(const vs_conv *h) { return (long long)h->MT_alloc * h->KT * h->nchunks * 64; }   // (cell, lane): eight values each in Ws

// work items of pack_conv_body for one handle (its fragments, at least its bias rows) and the grid that strides over them
static long long pack_work(const vs_conv *h) { return std::max(fragment_count(h), (long long)h->MT_alloc * 32); }
static unsigned pack_blocks(long long work) { return (unsigned)std::min<long long>(ceil_div(work, 256), 1024); }

// the VALU conv of conv_small.hip reads the weight in the reference layout (weff / beff): vs_conv_set_weights alone keeps that copy
static bool keeps_valu_weights(const vs_conv *h) { return h->kind == VS_CONV1D && h->c_out <= 4 && !(h->flags & VS_CONV_ADJOINT); }
// the fused forms (pair, batch) serve the training step's common case: split-f16, and not the <= 4-row VALU conv
static bool takes_fused_pack(const vs_conv *h) { return h->math == VS_MATH_SPLIT3 && !keeps_valu_weights(h); }

// {s_w, 1 / s_w, max |w| bits of the even packs, of the odd packs, scratch maximum of a vs_conv_set_math re-pack, 3 spare words}
static int reserve_wscale(vs_conv *h, hipStream_t s) {
    if (h->wsc.p) return VS_OK;
    VS_TRY(h->wsc.reserve(32));
    VS_CHECK_HIP(hipMemsetAsync(h->wsc.p, 0, 32, s));
    return VS_OK;
}

// the buffers a bind writes in the handle's arithmetic: fp32 fragments and packed bias always, the scale words for split-f16, the planes
// for every split engine
static int reserve_pack_buffers(vs_conv *h, hipStream_t s) {
    VS_TRY(h->wp.reserve((size_t)fragment_count(h) * sizeof(float)));
    VS_TRY(h->biasp.reserve((size_t)h->MT_alloc * 32 * sizeof(float)));
    if (h->math == VS_MATH_SPLIT3) VS_TRY(reserve_wscale(h, s));
    if (h->math) VS_TRY(h->ws.reserve((size_t)plane_cells(h) * split_planes(h->math) * 16));
    return VS_OK;
}

// The two max-|w| words of a split-f16 handle take turns: the pack of weight version pack_gen leaves the conv's largest |w| in slot
// (pack_gen & 1) and zeroes the other one for the next version.
static unsigned *max_slot(const vs_conv *h, int gen) { return reinterpret_cast<unsigned *>(h->wsc.as<float>() + 2) + (gen & 1); }

// fp32 fragments + bias of handle h from (w, bias).  scale: the weight-norm row scales of the plain call, NULL for an already folded weight.
// On a split-f16 handle this starts a new weight version (once per bind).
static PackParams pack_params(vs_conv *h, const float *w, const float *scale, const float *bias) {
    PackParams q;
    q.w = w; q.scale = scale; q.bias = bias; q.wp = h->wp.as<float>(); q.biasp = h->biasp.as<float>();
    q.kind = h->kind; q.c_in = h->c_in; q.c_out = h->c_out; q.k = h->k; q.up = h->dil; q.pad = h->pad; q.dmin = h->dmin;
    q.KT = h->KT; q.CP = h->CP; q.MT_alloc = h->MT_alloc; q.Hh = h->Hh; q.flags = h->flags; q.wino_tail1 = 0;
    q.maxbits = q.maxbits_clear = nullptr;
    if (h->math == VS_MATH_SPLIT3) {
        ++h->pack_gen;
        q.maxbits = max_slot(h, h->pack_gen);
        q.maxbits_clear = max_slot(h, h->pack_gen + 1);
    }
    return q;
}

// The planes of the split engines from the fp32 fragments.  maxbits_ready: the fp32 pack of THIS weight version has just left the conv's
// largest |w| in its slot (the bind paths); otherwise (vs_conv_set_math on a bound handle) pack_split finds it with a pass of its own over
// the fp32 fragments, through the handle's own scratch word: no allocation on any pack path (stream capture)
static vs_split_pack split_pack_params(const vs_conv *h, bool maxbits_ready) {
    vs_split_pack q;
    q.wp = h->wp.as<float>(); q.ws = h->ws.p; q.MT_alloc = h->MT_alloc; q.KT = h->KT; q.nchunks = h->nchunks; q.terms = h->math;
    q.wscale = nullptr;
    q.maxbits = nullptr;
    q.scratch = nullptr;
    if (h->math == VS_MATH_SPLIT3) {
        q.wscale = h->wsc.as<float>();
        if (maxbits_ready) q.maxbits = max_slot(h, h->pack_gen);
        else q.scratch = reinterpret_cast<unsigned *>(q.wscale + 4);
    }
    return q;
}

// Winograd-domain fragments of the fp32 engine, from the fp32 fragment buffer Wp of the current weight version
int pack_wino_weights(vs_conv *h, hipStream_t s) {
    if (h->wino_packed) return VS_OK;
    VS_TRY(order_write(h, s));         // (s becomes the producing stream of this version: a launch on another stream waits for the transform)
    const size_t nw = (size_t)h->MT_alloc * h->nchunks * h->wino_groups * 2 * 16 * 64;
    VS_TRY(h->wpw.reserve(nw * sizeof(float)));
    PackParams qw;
    memset(&qw, 0, sizeof(qw));
    qw.w = h->wp.as<float>(); qw.wp = h->wpw.as<float>(); qw.k = h->k; qw.KT = h->KT; qw.MT_alloc = h->MT_alloc;
    qw.wino_tail1 = (h->wino_k7 || h->wino_k11) ? 1 : 0;
    hipLaunchKernelGGL(pack_wino_kernel, dim3((unsigned)ceil_div((long long)nw, 256)), dim3(256), 0, s, qw, h->wino_groups, h->nchunks);
    VS_CHECK_HIP(hipGetLastError());
    h->wino_packed = true;
    return VS_OK;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_weightnorm_fold(const float *v, const float *g, float *w, int64_t rows, int64_t cols, void *stream) {
    VS_REQUIRE(v && g && w && rows > 0 && cols > 0, "vs_weightnorm_fold: bad arguments");
    hipStream_t s = as_stream(stream);
    float *scale = nullptr;
    VS_CHECK_HIP(hipMallocAsync((void **)&scale, sizeof(float) * rows, s));
    hipLaunchKernelGGL(rownorm_scale_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, v, g, scale,
                       (long long)rows, (long long)cols);
    hipLaunchKernelGGL(weightnorm_apply_kernel, dim3((unsigned)ceil_div(rows * cols, 256)), dim3(256), 0, s, v, scale, w,
                       (long long)rows, (long long)cols);
    VS_CHECK_HIP(hipGetLastError());
    VS_CHECK_HIP(hipFreeAsync(scale, s));
    return VS_OK;
}

int vs_conv_set_math(vs_conv_t *h, int math, void *stream) {
    VS_REQUIRE(h, "vs_conv_set_math: NULL handle");
    VS_REQUIRE(math == VS_MATH_F32 || math == VS_MATH_BF16 || math == VS_MATH_SPLIT6 || math == VS_MATH_SPLIT3, "vs_conv_set_math: unknown arithmetic %d", math);
    if (h->math == math) return VS_OK;
    h->math = math;
    if (math && h->weights_set) {      // a bound handle: the planes of the new arithmetic from the fp32 fragments it already holds
        hipStream_t s = as_stream(stream);
        VS_TRY(order_write(h, s));
        VS_TRY(reserve_pack_buffers(h, s));
        VS_TRY(pack_split(split_pack_params(h, false), s));
    }
    return VS_OK;
}

int vs_conv_get_math(const vs_conv_t *h) { return h ? h->math : -1; }

int vs_conv_set_weights(vs_conv_t *h, const float *w, const float *g, const float *bias, void *stream) {
    VS_REQUIRE(h && w, "vs_conv_set_weights: NULL handle or weight");
    VS_REQUIRE(!(h->flags & VS_CONV_ADJOINT) || !g, "vs_conv_set_weights: an ADJOINT handle takes the plain forward weight (g must be NULL)");
    hipStream_t s = as_stream(stream);
    VS_TRY(order_write(h, s));
    const float *scale = nullptr;
    if (g) {
        // weight_norm(dim=0): rows = dim 0 of the weight (c_out for Conv1d, c_in for ConvTranspose1d)
        const long long rows = (h->kind == VS_CONV_TRANSPOSE1D) ? h->c_in : h->c_out;
        const long long cols = (long long)h->c_in * h->c_out * h->k / rows;
        VS_TRY(h->scale.reserve(rows * sizeof(float)));
        hipLaunchKernelGGL(rownorm_scale_kernel, dim3((unsigned)ceil_div(rows, 4)), dim3(256), 0, s, w, g,
                           h->scale.as<float>(), rows, cols);
        scale = h->scale.as<float>();
    }
    VS_TRY(reserve_pack_buffers(h, s));
    const PackParams q = pack_params(h, w, scale, bias);
    if (h->math == VS_MATH_SPLIT3) {
        // split-f16: the planes need the largest weight first (one scale per conv): fp32 fragments, then the scaled planes
        hipLaunchKernelGGL(pack_conv_kernel, dim3(pack_blocks(pack_work(h))), dim3(256), 0, s, q);
        VS_CHECK_HIP(hipGetLastError());
        VS_TRY(pack_split(split_pack_params(h, true), s));
    } else if (h->math) {
        // bf16-pipe arithmetic: fp32 fragments + bf16 planes in one launch
        const long long total = std::max(plane_cells(h), (long long)h->MT_alloc * 32);
        hipLaunchKernelGGL(pack_conv_split_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, s, q, h->ws.p, split_planes(h->math));
    } else {
        hipLaunchKernelGGL(pack_conv_kernel, dim3(pack_blocks(pack_work(h))), dim3(256), 0, s, q);
    }
    h->wino_packed = false;        // (the F(2,3) transform of the fp32 engine is rebuilt from Wp by the first launch that uses it)
    if (keeps_valu_weights(h)) {
        const long long cols = (long long)h->c_in * h->k;
        VS_TRY(h->weff.reserve((size_t)h->c_out * cols * sizeof(float)));
        hipLaunchKernelGGL(fold_weights_kernel, dim3((unsigned)ceil_div(h->c_out * cols, 256)), dim3(256), 0, s, w, scale,
                           h->weff.as<float>(), (long long)h->c_out, cols);
        h->has_bias = bias != nullptr;
        if (bias) {
            VS_TRY(h->beff.reserve((size_t)h->c_out * sizeof(float)));
            VS_CHECK_HIP(hipMemcpyAsync(h->beff.p, bias, (size_t)h->c_out * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    VS_CHECK_HIP(hipGetLastError());
    h->weights_set = true;
    return VS_OK;
}

int vs_conv_set_weights_pair(vs_conv_t *h0, vs_conv_t *h1, const float *w, const float *bias0, void *stream) {
    VS_REQUIRE(h0 && h1 && w, "vs_conv_set_weights_pair: NULL handle or weight");
    // h1 reads the SAME weight tensor as the grad-input conv of h0: anything else would index `w` out of bounds in the pack
    VS_REQUIRE((h1->flags & VS_CONV_ADJOINT) && !(h0->flags & VS_CONV_ADJOINT) && h1->c_in == h0->c_out && h1->c_out == h0->c_in && h1->k == h0->k &&
                   (h0->kind == VS_CONV_TRANSPOSE1D || h1->dil == h0->dil),
               "vs_conv_set_weights_pair: the second handle is not the VS_CONV_ADJOINT counterpart of the first (c_in / c_out swapped, same k and dilation)");
    if (!(takes_fused_pack(h0) && takes_fused_pack(h1))) {      // everything else is the two plain calls
        VS_TRY(vs_conv_set_weights(h0, w, nullptr, bias0, stream));
        return vs_conv_set_weights(h1, w, nullptr, nullptr, stream);
    }
    hipStream_t s = as_stream(stream);
    PackParams q[2];
    vs_conv *hs[2] = {h0, h1};
    long long work = 0;
    for (int i = 0; i < 2; ++i) {
        VS_TRY(order_write(hs[i], s));
        VS_TRY(reserve_pack_buffers(hs[i], s));
        q[i] = pack_params(hs[i], w, nullptr, i == 0 ? bias0 : nullptr);
        work = std::max(work, pack_work(hs[i]));
    }
    hipLaunchKernelGGL(pack_conv_pair_kernel, dim3(pack_blocks(work), 2), dim3(256), 0, s, q[0], q[1]);
    VS_CHECK_HIP(hipGetLastError());
    vs_split_pack sp[2];
    for (int i = 0; i < 2; ++i) {
        sp[i] = split_pack_params(hs[i], true);
        hs[i]->wino_packed = false;
        hs[i]->weights_set = true;
    }
    return pack_split_pair(sp[0], sp[1], s);
}

}  // extern "C"

// ---- vs_conv_set_weights_batch: the table of one batch (PackParams x n | vs_split_pack x n | first pack block x (n + 1) | first split block x (n + 1))
// goes to the device through one of a ring of pinned staging buffers, each with a device twin and an event recorded behind the launches that read
// it: a slot is reused only when its event has completed (normally long ago: a training step makes two or three batches).
namespace {
struct BatchSlot {
    void *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    int device = -1;          // the device `dev` and `ev` belong to (the ring served whichever device was current at first use)
};
// marks a slot busy from the moment its host buffer has been handed to an asynchronous copy, whatever happens afterwards (on an error behind the copy
// the slot stayed "free" and its host buffer could be rewritten while the copy was still in flight)
struct SlotInFlight {
    BatchSlot *sl;
    hipStream_t s;
    ~SlotInFlight() {
        if (hipEventRecord(sl->ev, s) == hipSuccess) sl->pending = true;
        else (void)hipStreamSynchronize(s);
    }
};
struct BatchArena {
    std::mutex mu;
    static constexpr int NSLOT = 8;
    BatchSlot slot[NSLOT];
    int next = 0;
};
BatchArena g_batch;

int batch_slot(size_t bytes, BatchSlot **out) {
    BatchSlot &sl = g_batch.slot[g_batch.next];
    g_batch.next = (g_batch.next + 1) % BatchArena::NSLOT;
    if (sl.pending) {
        VS_CHECK_HIP(hipEventSynchronize(sl.ev));
        sl.pending = false;
    }
    int cur = 0;
    VS_CHECK_HIP(hipGetDevice(&cur));
    if (sl.device != cur) {       // first use, or the process moved to another device: this slot's device buffer and event are re-made there
        if (sl.ev) (void)hipEventDestroy(sl.ev);
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
        sl.ev = nullptr;
        sl.host = sl.dev = nullptr;
        sl.cap = 0;
        sl.device = cur;
    }
    if (!sl.ev) VS_CHECK_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (bytes > sl.cap) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) (void)hipFree(sl.dev);
        sl.host = sl.dev = nullptr;
        sl.cap = 0;
        const size_t cap = std::max<size_t>(bytes * 2, 64 * 1024);
        VS_CHECK_HIP(hipHostMalloc(&sl.host, cap, hipHostMallocDefault));
        VS_CHECK_HIP(hipMalloc(&sl.dev, cap));
        sl.cap = cap;
    }
    *out = &sl;
    return VS_OK;
}
}  // namespace

extern "C" int vs_conv_set_weights_batch(vs_conv_t *const *handles, const float *const *w, const float *const *bias, int n, void *stream) {
    VS_REQUIRE(n >= 0 && (n == 0 || (handles && w)), "vs_conv_set_weights_batch: NULL array");
    hipStream_t s = as_stream(stream);
    // handles outside the batch kernels' case (other arithmetic, the <= 4-row VALU convs) take the plain call
    std::vector<int> idx;
    idx.reserve(n);
    for (int i = 0; i < n; ++i) {
        vs_conv *h = handles[i];
        VS_REQUIRE(h && w[i], "vs_conv_set_weights_batch: entry %d: NULL handle or weight", i);
        if (!takes_fused_pack(h)) VS_TRY(vs_conv_set_weights(h, w[i], nullptr, bias ? bias[i] : nullptr, stream));
        else idx.push_back(i);
    }
    const int m = (int)idx.size();
    if (m == 0) return VS_OK;
    if (m == 1) return vs_conv_set_weights(handles[idx[0]], w[idx[0]], nullptr, bias ? bias[idx[0]] : nullptr, stream);
    {   // no handle twice in one batch: each job flips its handle's weight-maximum slot (pack_gen), so a duplicate would make one job clear the slot the other reads
        std::unordered_set<const vs_conv *> seen;
        for (int j = 0; j < m; ++j)
            VS_REQUIRE(seen.insert(handles[idx[j]]).second, "vs_conv_set_weights_batch: entry %d: the same handle appears twice in one batch", idx[j]);
    }
    std::lock_guard<std::mutex> lock(g_batch.mu);
    const size_t off_sp = (size_t)m * sizeof(PackParams), off_b0 = off_sp + (size_t)m * sizeof(vs_split_pack),
                 off_b1 = off_b0 + (size_t)(m + 1) * sizeof(unsigned), bytes = off_b1 + (size_t)(m + 1) * sizeof(unsigned);
    BatchSlot *sl = nullptr;
    VS_TRY(batch_slot(bytes, &sl));
    char *hb = static_cast<char *>(sl->host);
    PackParams *q = reinterpret_cast<PackParams *>(hb);
    vs_split_pack *sp = reinterpret_cast<vs_split_pack *>(hb + off_sp);
    unsigned *b0 = reinterpret_cast<unsigned *>(hb + off_b0), *b1 = reinterpret_cast<unsigned *>(hb + off_b1);
    unsigned nb0 = 0, nb1 = 0;
    for (int j = 0; j < m; ++j) {
        vs_conv *h = handles[idx[j]];
        VS_TRY(order_write(h, s));
        VS_TRY(reserve_pack_buffers(h, s));
        q[j] = pack_params(h, w[idx[j]], nullptr, bias ? bias[idx[j]] : nullptr);
        b0[j] = nb0;
        nb0 += pack_blocks(pack_work(h));
        sp[j] = split_pack_params(h, true);
        b1[j] = nb1;
        nb1 += (unsigned)ceil_div(plane_cells(h), 256);
        h->wino_packed = false;
        h->weights_set = true;
    }
    b0[m] = nb0;
    b1[m] = nb1;
    VS_CHECK_HIP(hipMemcpyAsync(sl->dev, sl->host, bytes, hipMemcpyHostToDevice, s));
    SlotInFlight in_flight{sl, s};         // (records the slot's event behind everything launched below, on every way out)
    const char *db = static_cast<const char *>(sl->dev);
    hipLaunchKernelGGL(pack_conv_multi_kernel, dim3(nb0), dim3(256), 0, s, reinterpret_cast<const PackParams *>(db),
                       reinterpret_cast<const unsigned *>(db + off_b0), m);
    VS_CHECK_HIP(hipGetLastError());
    VS_TRY(pack_split_multi(reinterpret_cast<const vs_split_pack *>(db + off_sp), reinterpret_cast<const unsigned *>(db + off_b1), m, nb1, s));
    return VS_OK;
}
