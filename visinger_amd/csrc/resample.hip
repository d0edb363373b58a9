// resample.hip -- rational polyphase sample-rate conversion on the device: recordings at 44.1 / 48 kHz in, waveforms at 44.1 / 48 kHz out, one launch for a
// batch of ragged rows.  DESIGN.md 4.15, the rule: include/visinger_hip.h "f9".  Not in the reference, which resamples on the host through librosa.
//   y[b, n] = sum_i x[b, i] h(n M - i L) over 0 <= i < len_b, |n M - i L| <= W.  With n M = q L + p (0 <= p < L) and C = ceil(W / L) the terms are
//   i = q - C + j, j = 0 .. P - 1 (P = 2 C + 1), with the tap h((C - j) L + p): the fp32 TABLE row of phase p, zero where the prototype is.
// Table layout (the host builds it, resample.py design()): [L][P], row rho holds the phase (rho M) mod L -- the phase of every output n with n mod L = rho.
// Tiling.  A tile is R = 4 groups of G = g L consecutive outputs (g = round(256 / L), at least 1: G is about 256) and starts at a multiple of 4 G, so
//   n0 M is a multiple of L.  Lane c < G takes the outputs n0 + c + r G, r = 0 .. 3: all four on table row c mod L, their windows g M samples apart
//   (q = q0 + floor(c M / L) + r g M, exactly).  One tap of the row therefore serves four products: five LDS words for four fmas where one output a lane
//   takes eight.  A workgroup (G rounded up to whole waves, 256 lanes walking the groups when L > 256) loads the table into LDS ONCE (16-byte loads),
//   then walks the tiles of its row (tile index blockIdx.x, + gridDim.x, ..), staging each tile's input span plus the filter's reach with 16-byte loads
//   (zeros outside [0, len_b)).  Stores: consecutive lanes, consecutive words.
// Banking (ds_read_b32: 32 banks of 4 B, a wave in two groups of 32 lanes).  Table: consecutive lanes read word (c mod L) P + j of consecutive rows, and P
//   is odd -- an odd pitch is a bijection modulo 32, so the 32 lanes of a group fall on 32 different banks (across the wrap c mod L = 0 two stretches
//   of rows may meet pairwise; with L <= 32 there are only L different words, each broadcast).  Rows in PHASE order would put lane c on row
//   (c (M mod L)) mod L: at 147 / 80 the stride 80 P maps a group onto 2 banks.  Grouping outputs of equal phase along the lanes instead (the table read
//   wave-uniform) strides the input by M words: 16-way conflicts at M = 80, none at odd M -- here equal phases sit in one lane's registers instead, and
//   the layout does not depend on the ratio.  Input: lane c's window starts at floor(c M / L), which steps floor or ceil(M / L) words a lane: for M <= L
//   the 32 words of a group lie within 32 consecutive ones (conflict-free, equal words broadcast); for L < M <= 2 L they span up to 64: two lanes a
//   bank at worst, the price of down-conversion here.
// Summation order (fixed per output, whatever B, the row, the padding, n_in, n_out, the grid): acc = 0, then acc = fma(x[q - C + j], table[n mod L][j], acc)
//   (v_fma_f32: one rounding) for j = 0 .. P - 1 ascending -- ascending i in one chain.  Terms outside [0, len_b) or outside the prototype enter as a product with an exact zero.
#include "vs_internal.h"

namespace vs {

constexpr int RS_R = 4;                                    // outputs per lane and tile: the groups of a tile
constexpr int RS_MAX_THREADS = 384;

// g: periods of L outputs per group, G = g L about 256 lanes' worth
static inline long long rs_group(long long L) {
    const long long g = (256 + L / 2) / L;
    return (g < 1 ? 1 : g) * L;
}

// One fused multiply-add as an opaque scalar instruction (conv_common.h: mul_f32_scalar / add_f32_scalar): unrolled, the four chains of a lane share the tap h,
// and hipcc's SLP vectoriser pairs them into v_pk_fma_f32 with op_sel:[_,1] on h -- the form that returns wrong low results in lanes 48-63 beside another wave's
// MFMAs on gfx950, which is where this kernel runs under synthesize(streams=2).  build.py refuses an object that holds one.
__device__ __forceinline__ float fma_f32_scalar(float a, float b, float c) {
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

struct ResampleArgs {
    const float *x, *table;
    const long long *lengths;
    float *y;
    long long *out_lengths;
    long long B, n_in, n_out;
    int L, M, P, C, G, step, tab_floats, vec;              // G: outputs per group; step = G M / L: samples between a lane's windows; tab_floats: L * P rounded
};                                                         // up to 4 (the input span sits behind it); vec: rows of x are 16-byte aligned

__global__ void __launch_bounds__(RS_MAX_THREADS) resample_kernel(const ResampleArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *tab = lds, *xs = lds + p.tab_floats;
    const int tid = threadIdx.x, nt = blockDim.x;
    const long long tile = (long long)RS_R * p.G;
    {
        const int n_tab = p.L * p.P, n4 = n_tab >> 2;                                     // (the table is 16-byte aligned: checked by the host)
        const float4 *src = reinterpret_cast<const float4 *>(p.table);
        for (int v = tid; v < n4; v += nt) reinterpret_cast<float4 *>(tab)[v] = src[v];
        for (int i = 4 * n4 + tid; i < n_tab; i += nt) tab[i] = p.table[i];
    }
    for (long long row = blockIdx.y; row < p.B; row += gridDim.y) {
        long long len = p.lengths ? p.lengths[row] : p.n_in;
        len = len < 0 ? 0 : (len > p.n_in ? p.n_in : len);
        const long long out_len = (len * p.L + p.M - 1) / p.M, n_valid = out_len < p.n_out ? out_len : p.n_out;
        if (p.out_lengths && blockIdx.x == 0 && tid == 0) p.out_lengths[row] = out_len;
        const float *src = p.x + row * p.n_in;
        float *dst = p.y + row * p.n_out;
        for (long long n0 = blockIdx.x * tile; n0 < p.n_out; n0 += gridDim.x * tile) {
            if (n0 >= n_valid) {                                                          // (uniform over the workgroup: no barrier is skipped by some lanes only)
                for (long long n = n0 + tid; n < n0 + tile && n < p.n_out; n += nt) dst[n] = 0.f;
                continue;
            }
            const long long q0 = n0 / p.L * p.M;                                          // n0 M / L, exactly (64-bit: n M passes 2^31 on long rows)
            const int cnt = (int)(n_valid - n0 < tile ? n_valid - n0 : tile);
            const long long s0 = (q0 - p.C) & ~3ll;                                       // the span starts at a multiple of four samples (also below 0)
            const int q_last = (int)((long long)(cnt - 1) * p.M / p.L);
            const int n_stage = ((int)(q0 + q_last + p.C - s0) + 4) & ~3;                 // <= the span the host sized the LDS for
            __syncthreads();                                                              // (the table is in place; the previous tile's reads are done)
            for (int v = tid; 4 * v < n_stage; v += nt) {
                const long long s = s0 + 4 * v;
                float4 w;
                if (p.vec && s >= 0 && s + 4 <= p.n_in) {
                    w = *reinterpret_cast<const float4 *>(src + s);
                    w.x = s < len ? w.x : 0.f, w.y = s + 1 < len ? w.y : 0.f, w.z = s + 2 < len ? w.z : 0.f, w.w = s + 3 < len ? w.w : 0.f;
                } else {
                    w.x = (s >= 0 && s < len) ? src[s] : 0.f, w.y = (s + 1 >= 0 && s + 1 < len) ? src[s + 1] : 0.f;
                    w.z = (s + 2 >= 0 && s + 2 < len) ? src[s + 2] : 0.f, w.w = (s + 3 >= 0 && s + 3 < len) ? src[s + 3] : 0.f;
                }
                reinterpret_cast<float4 *>(xs)[v] = w;
            }
            __syncthreads();
            for (int c = tid; c < p.G && c < cnt; c += nt) {                              // (no barrier inside)
                const float *ph = tab + (c % p.L) * p.P;
                const float *px0 = xs + (int)(q0 - p.C - s0) + (int)((long long)c * p.M / p.L);
                const float *px[RS_R];
                float acc[RS_R];
#pragma unroll
                for (int r = 0; r < RS_R; ++r) {
                    px[r] = c + r * p.G < cnt ? px0 + r * p.step : px0;                   // a group beyond the row reads the first group's window
                    acc[r] = 0.f;
                }
                int j = 0;
                for (; j + 8 <= p.P; j += 8) {                                            // eight taps' reads in flight; the chains stay in order
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float h = ph[j + u];
#pragma unroll
                        for (int r = 0; r < RS_R; ++r) acc[r] = fma_f32_scalar(px[r][j + u], h, acc[r]);
                    }
                }
                for (; j < p.P; ++j) {
                    const float h = ph[j];
#pragma unroll
                    for (int r = 0; r < RS_R; ++r) acc[r] = fma_f32_scalar(px[r][j], h, acc[r]);
                }
#pragma unroll
                for (int r = 0; r < RS_R; ++r) {
                    const long long n = n0 + c + r * p.G;
                    if (n < p.n_out) dst[n] = c + r * p.G < cnt ? acc[r] : 0.f;
                }
            }
            for (long long n = n0 + cnt + tid; n < n0 + tile && n < p.n_out; n += nt)     // lanes c >= cnt of the first group: zeros the loop above did not write
                if ((n - n0) % p.G >= cnt) dst[n] = 0.f;
        }
    }
}

// floats of LDS the input span of one tile needs: the alignment slack, the tile's own samples and the filter's reach on both sides, in fours
static long long rs_span(long long L, long long M, long long P) {
    return (3 + (RS_R * rs_group(L) - 1) * M / L + P + 4) & ~3ll;
}

}  // namespace vs

using namespace vs;

extern "C" {

int64_t vs_resample_tile(int L) { return L < 1 ? 0 : RS_R * rs_group(L); }

int vs_resample_fits(int L, int M, int P) {
    if (L < 1 || M < 1 || M > VS_RESAMPLE_MAX_M || P < 3 || !(P & 1)) return 0;
    const long long tab = (long long)L * P;
    if (tab * 4 > VS_RESAMPLE_TABLE_BYTES) return 0;
    return (((tab + 3) & ~3ll) + rs_span(L, M, P)) * 4 <= VS_RESAMPLE_LDS_BYTES;
}

int vs_resample_poly(const float *x, const int64_t *lengths, int64_t B, int64_t n_in, const float *table, int L, int M, int P, float *y, int64_t n_out,
                     int64_t *out_lengths, void *stream) {
    VS_REQUIRE(x && table && y, "vs_resample_poly: x, table and y must not be NULL");
    VS_REQUIRE(x != y && table != y && x != table && (const void *)lengths != (const void *)y && (const void *)out_lengths != (const void *)y &&
                   (!out_lengths || ((const void *)out_lengths != (const void *)x && (const void *)out_lengths != (const void *)table && out_lengths != lengths)),
               "vs_resample_poly: x, lengths, table, y and out_lengths must be distinct buffers");
    VS_REQUIRE(B > 0 && n_in > 0 && n_out > 0, "vs_resample_poly: B, n_in, n_out must be positive (got %lld, %lld, %lld)", (long long)B, (long long)n_in,
               (long long)n_out);
    VS_REQUIRE(n_in < (1ll << 40) && n_out < (1ll << 40) && B <= INT64_MAX / 4 / n_in && B <= INT64_MAX / 4 / n_out,
               "vs_resample_poly: n_in = %lld or n_out = %lld is not below 2^40, or B * n_in / B * n_out is out of range", (long long)n_in, (long long)n_out);
    VS_REQUIRE(L >= 1 && M >= 1 && M <= VS_RESAMPLE_MAX_M, "vs_resample_poly: L = %d and M = %d must be at least 1, M at most %d", L, M, VS_RESAMPLE_MAX_M);
    VS_REQUIRE(P >= 3 && (P & 1), "vs_resample_poly: P = %d must be odd and at least 3 (2 ceil(W / L) + 1)", P);
    VS_REQUIRE((long long)L * P * 4 <= VS_RESAMPLE_TABLE_BYTES, "vs_resample_poly: the table of L = %d rows of P = %d taps exceeds the budget of %d bytes", L, P,
               VS_RESAMPLE_TABLE_BYTES);
    VS_REQUIRE(vs_resample_fits(L, M, P), "vs_resample_poly: the table and a tile's input span (L = %d, M = %d, P = %d) exceed %d bytes of LDS", L, M, P,
               VS_RESAMPLE_LDS_BYTES);
    VS_REQUIRE(((uintptr_t)table & 15) == 0, "vs_resample_poly: the table must be 16-byte aligned");
    ResampleArgs a;
    a.x = x, a.table = table, a.lengths = (const long long *)lengths, a.y = y, a.out_lengths = (long long *)out_lengths;
    a.B = B, a.n_in = n_in, a.n_out = n_out, a.L = L, a.M = M, a.P = P, a.C = (P - 1) / 2;
    a.G = (int)rs_group(L), a.step = (int)(rs_group(L) / L * M);
    a.tab_floats = (L * P + 3) & ~3;
    a.vec = ((uintptr_t)x & 15) == 0 && n_in % 4 == 0;
    const size_t lds_bytes = sizeof(float) * ((size_t)a.tab_floats + (size_t)rs_span(L, M, P));
    const int threads = a.G <= RS_MAX_THREADS ? (a.G + 63) & ~63 : 256;           // whole waves over a group; the lanes walk a longer one
    // the workgroups of a row share its tiles (tile index + k gridDim.x).  As many workgroups as the chip holds at once -- by LDS and by the 5 waves a SIMD
    // takes of this kernel -- so that the table is loaded once per resident workgroup and no second, partly filled round of workgroups trails the first
    // (2 - 5 % against a fixed 1024 workgroups).  The result does not depend on it.
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        cus = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    }
    const long long by_lds = (160 * 1024) / (long long)lds_bytes, by_waves = (20 * 64) / threads;
    const long long per_cu = by_lds < by_waves ? (by_lds < 1 ? 1 : by_lds) : (by_waves < 1 ? 1 : by_waves);
    const long long gy = B < 65535 ? B : 65535, tiles = ceil_div(n_out, (int64_t)RS_R * a.G);
    long long gx = ceil_div(cus * per_cu, gy);
    gx = gx < tiles ? gx : tiles;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)gx, (unsigned)gy), dim3((unsigned)threads), lds_bytes, as_stream(stream), a);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
