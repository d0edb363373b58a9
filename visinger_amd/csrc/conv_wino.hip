// conv_wino.hip -- the minimal-filtering (Winograd F(2,3)) kernel of the fp32 conv engine and its launchers (the kernel's own
// comment below says what it computes; vs_conv_forward in conv_engine.hip decides which launches take it).
#include "conv_common.h"

#include <algorithm>
#include <type_traits>

namespace vs {

// One half-step of conv_wino_kernel: 4 input-channel pairs of one tap group, F(2,3): four products per pair column.
// x values of channel pair cp + 1 are read from LDS under the MFMAs of pair cp; the V's of a pair are all formed before its
// first MFMA (a VALU result consumed by the very next MFMA costs wait states).  xa/xb: LDS addresses of (x0, x2) and (x1, x3)
// of the wave's two pair tiles -- with dilation 1 the even and odd columns of the window are staged in separate halves of
// each LDS row, so both are unit-stride across lanes (a stride-2 read is a 2-way bank conflict); otherwise xb = xa + DIL.
// (A partial last tap group can run as F(2,2) / direct form into the same accumulators -- k=7: 10 instead of 12 MFMAs -- but
// any RUNTIME control flow with MFMAs on the accumulators in both arms makes hipcc spill them: the generic kernel zero-pads
// the taps, and the k = 7 instances (TG = 3) unroll the six half-steps of a chunk as straight-line code.)
template <int DIL, int TAPS>
__device__ __forceinline__ void wino_half_step(f32x16 (&acc)[4][2], const float (&a)[16], const float *xa0, const float *xb0,
                                               const float *xa1, const float *xb1, int RP) {
    // TAPS == 3: F(2,3), four products.  TAPS == 1 (the last group of k = 7 in the k-specialised instances, where the step
    // sequence of a chunk is straight-line code -- no branch carries the accumulators): the direct form, y[t] += w x0 into M0
    // and y[t+d] += w x1 into M3 (U3 is packed negated): two products instead of the zero-padded four.
    constexpr int S2 = (DIL == 1) ? 1 : 2 * DIL;      // distance x0 -> x2 (and x1 -> x3) in LDS words
    const float *xa[2] = {xa0, xa1}, *xb[2] = {xb0, xb1};
    float xc[2][4], xn[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        xc[j][0] = xa[j][0];
        xc[j][1] = xb[j][0];
        if constexpr (TAPS >= 2) xc[j][2] = xa[j][S2];
        if constexpr (TAPS == 3) xc[j][3] = xb[j][S2];
    }
#pragma unroll
    for (int cp = 0; cp < 4; ++cp) {
        if (cp + 1 < 4) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                xn[j][0] = xa[j][(cp + 1) * 2 * RP];
                xn[j][1] = xb[j][(cp + 1) * 2 * RP];
                if constexpr (TAPS >= 2) xn[j][2] = xa[j][(cp + 1) * 2 * RP + S2];
                if constexpr (TAPS == 3) xn[j][3] = xb[j][(cp + 1) * 2 * RP + S2];
            }
        }
        float v[4][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if constexpr (TAPS == 3) {
                v[0][j] = xc[j][0] - xc[j][2];
                v[1][j] = xc[j][1] + xc[j][2];
                v[2][j] = xc[j][2] - xc[j][1];
                v[3][j] = xc[j][1] - xc[j][3];
            } else if constexpr (TAPS == 2) {      // F(2,2): (x0 - x1) w0 -> M0, x1 (w0 + w1) -> M1, (x1 - x2) w1 -> M3
                v[0][j] = xc[j][0] - xc[j][1];
                v[1][j] = xc[j][1];
                v[2][j] = 0.f;
                v[3][j] = xc[j][1] - xc[j][2];
            } else {
                v[0][j] = xc[j][0];
                v[1][j] = 0.f;
                v[2][j] = 0.f;
                v[3][j] = xc[j][1];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int xi = 0; xi < 4; ++xi) {
            if constexpr (TAPS == 1) {
                if (xi == 1 || xi == 2) continue;          // (compile-time after unrolling)
            }
            if constexpr (TAPS == 2) {
                if (xi == 2) continue;
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[xi][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cp * 4 + xi], v[xi][j], acc[xi][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < TAPS + 1; ++q) xc[j][q] = xn[j][q];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Minimal-filtering (Winograd F(2,3)) variant of the engine for the stride-1 "same" convolutions with >= 3 taps
// (the HiFi-GAN resblock convs k in {3,7,11}, dilation {1,3,5}, decoder.py:72-87 -- 87 % of the synthesis FLOPs -- and the
// FFN k=9 convs, rel_transformer.py:332-333).  The taps are cut into groups of three; for one group and one pair of
// outputs (y[t], y[t+d]) the six products of the direct form become four:
//     V0 = x0 - x2, V1 = x1 + x2, V2 = x2 - x1, V3 = x1 - x3                 (x_j = x[t + (3g + j) d - pad])
//     U0 = w0, U1 = (w0 + w1 + w2)/2, U2 = (w0 - w1 + w2)/2, U3 = w2          (packed once, pack_wino_kernel)
//     M_xi += U_xi . V_xi  (contraction over input channels: the MFMA)        y[t] = M0+M1+M2, y[t+d] = M1-M2-M3
// so the matrix pipe does 4/6 of the direct work (k=9: 12/18; k=11: 16/22 and k=7: 12/14 with the zero-padded last group).  The
// transforms use the points {0, 1, -1, inf} only: coefficients 1 and 1/2, error growth ~2x an fp32 dot product.
// Same skeleton as conv_mfma_kernel: activations staged once per 16-channel chunk in LDS (the V's are formed per
// wave from four shifted LDS reads: 1 ds_read + 1 VALU per MFMA), weights as fragments from L2 through a 3-deep
// register ring, LDS-transposed vector epilogue.  A wave owns 32 rows x PW "pair columns" (c -> outputs t(c), t(c)+d
// with t(c) = (c / d) * 2d + c % d, a contiguous run of 2*PW outputs when d divides PW) x 4 xi = 8 accumulator tiles.
template <int DIL, int WAVES_M, int WAVES_N, int TG, int TT>
__global__ void __launch_bounds__(64 * WAVES_M * WAVES_N, 2) conv_wino_kernel(const ConvParams p) {
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int PW = (64 / DIL) * DIL;         // valid pair columns per wave (of 64)
    constexpr int NBW = 2 * PW;                  // outputs per wave
    constexpr int BN = NBW * WAVES_N;
    constexpr int MAXW = BN + MAX_SPAN;
    constexpr int RPW = CK / NW;
    constexpr int CIT = (MAXW + 63) / 64;
    constexpr int CWP = NBW + 8;                 // row pitch of the epilogue transposition buffer (+ dump columns)
    static_assert(CK % NW == 0, "CK must be a multiple of the wave count");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M;
    const int wn = wave / WAVES_M;
    const int b = blockIdx.z;
    const int n0 = blockIdx.x * BN;
    const int mt0 = blockIdx.y * WAVES_M + wm;
    const int W = p.W;
    const int G = p.KT;                          // tap groups
    // LDS row: dilation 1 -> even columns of the window at [0, Wh), odd columns at [H, H + Wh), H = 16 mod 32 (the staging
    // writes of a half-wave then cover all 32 banks); otherwise the window as it is.
    const int Wh = (W + 1) >> 1;
    const int H = ((Wh + 15) & ~31) + 16;
    const int RP = (DIL == 1) ? H + Wh : W;
    float *const buf0 = smem;
    float *const buf1 = smem + CK * RP;
    const float *const xb = p.x + (long long)b * p.x_bs;
    const float *const maskb = p.mask ? p.mask + (long long)b * p.Tin : nullptr;
    const int lhalf = lane >> 5;
    const int l31 = lane & 31;

    // M0 starts from the row's bias and M3 from its negative (y[t] = M0+M1+M2, y[t+d] = M1-M2-M3): see conv_mfma_kernel
    const float *const bbias = p.bias_b ? p.bias_b + (long long)b * p.bias_b_bs : nullptr;
    f32x16 acc[4][2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = mt0 * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
        float bv = p.biasp[row];
        if (bbias) bv += bbias[min(row, p.M - 1)];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[0][j][r] = bv;
            acc[1][j][r] = 0.f;
            acc[2][j][r] = 0.f;
            acc[3][j][r] = -bv;
        }
    }

    // pair column -> first output of the pair, relative to the wave's first output
    int posr[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = j * 32 + l31;
        const int t = (c / DIL) * (2 * DIL) + (c % DIL);
        posr[j] = (c < PW) ? t : 0;          // idle columns read a valid LDS address
    }

    float st[RPW][CIT];
    float mk[CIT];
    const int in_act = p.in_act;
    const __amdgpu_buffer_rsrc_t xsrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)xb, 0, (int)((long long)p.Cin * p.Tin * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t msrc =
        __builtin_amdgcn_make_buffer_rsrc((void *)(maskb ? maskb : xb), 0, p.Tin * 4, 0x00020000);
    auto stage_load = [&](int chunk) __attribute__((always_inline)) {
        const int nbase = n0 + p.lo + lane;
        if (in_act >= VS_IN_MASK) {
#pragma unroll
            for (int i = 0; i < CIT; ++i)
                mk[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(msrc, nbase * 4 + i * 256, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < RPW; ++j) {
            const int ci = min(chunk * CK + wave + NW * j, p.Cin - 1);
            const int voff = (ci * p.Tin + nbase) * 4;
#pragma unroll
            for (int i = 0; i < CIT; ++i)
                st[j][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xsrc, voff + i * 256, 0, 0));
        }
    };
    const bool time_edge = (n0 + p.lo < 0) || (n0 + p.lo + W > p.Tin);
    auto stage_store = [&](float *buf, int chunk) __attribute__((always_inline)) {
        auto run = [&](auto edge_tag, auto act_tag) __attribute__((always_inline)) {   // (see conv_mfma_kernel)
            constexpr bool EDGE = decltype(edge_tag)::value;
            constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
            for (int i = 0; i < CIT; ++i) {
                const int col = lane + 64 * i;
                const int n = n0 + p.lo + col;
                const bool okn = (n >= 0) && (n < p.Tin);
                const int idx = (DIL == 1) ? ((col & 1) ? H : 0) + (col >> 1) : col;
#pragma unroll
                for (int j = 0; j < RPW; ++j) {
                    float v = st[j][i];
                    if constexpr (EDGE) v = (okn && (chunk * CK + wave + NW * j < p.Cin)) ? v : 0.f;
                    if constexpr (ACT == VS_IN_LRELU || ACT == VS_IN_LRELU_MASK) v = fmaxf(v, 0.1f * v);
                    if constexpr (ACT >= VS_IN_MASK) v *= mk[i];
                    if (64 * (i + 1) <= BN || col < W) buf[(wave + NW * j) * RP + idx] = v;      // W >= BN
                }
            }
        };
        const bool edge = time_edge || (chunk * CK + CK > p.Cin);
        if (edge) {
            if (in_act == VS_IN_NONE) run(std::true_type{}, std::integral_constant<int, VS_IN_NONE>{});
            else if (in_act == VS_IN_LRELU) run(std::true_type{}, std::integral_constant<int, VS_IN_LRELU>{});
            else if (in_act == VS_IN_MASK) run(std::true_type{}, std::integral_constant<int, VS_IN_MASK>{});
            else run(std::true_type{}, std::integral_constant<int, VS_IN_LRELU_MASK>{});
        } else {
            if (in_act == VS_IN_NONE) run(std::false_type{}, std::integral_constant<int, VS_IN_NONE>{});
            else if (in_act == VS_IN_LRELU) run(std::false_type{}, std::integral_constant<int, VS_IN_LRELU>{});
            else if (in_act == VS_IN_MASK) run(std::false_type{}, std::integral_constant<int, VS_IN_MASK>{});
            else run(std::false_type{}, std::integral_constant<int, VS_IN_LRELU_MASK>{});
        }
    };

    // ------------------------------------------------------------------------------------------------ main loop
    // step s = ((chunk * G + g) * 2 + half): 4 channel pairs x 4 xi x 2 pair tiles = 32 MFMAs on 16 weight fragments,
    // which are contiguous in the packed array (one base pointer, immediate offsets).
    const int nsteps = p.nchunks * G * 2;
    // (the four xi fragments of a channel pair are interleaved per lane: one 16-byte load each, 1 KiB per wave-instruction)
    const float *const wbase = p.wp + (long long)mt0 * nsteps * (16 * 64) + lane * 4;
    float a0[16], a1[16], a2[16];
    auto load_a = [&](float (&dst)[16], int step_) __attribute__((always_inline)) {
        const float *src = wbase + (long long)step_ * (16 * 64);
#pragma unroll
        for (int cp = 0; cp < 4; ++cp) {
            const float4 t = *reinterpret_cast<const float4 *>(src + cp * 256);
            dst[cp * 4 + 0] = t.x; dst[cp * 4 + 1] = t.y; dst[cp * 4 + 2] = t.z; dst[cp * 4 + 3] = t.w;
        }
    };
    // ring depth: 3 slots (fragments requested two half-steps ahead), 2 for the widest workgroup shape (its 36 staging
    // registers do not leave room for the third slot)
    constexpr int RING = (WAVES_N == 4 || TG == 4) ? 2 : 3;
    if (nsteps > 0) load_a(a0, 0);
    if (RING == 3 && nsteps > 1) load_a(a1, 1);

    stamp(p, 0);
    stage_load(0);
    stage_store(buf0, 0);
    if (p.nchunks > 1) stage_load(1);
    __syncthreads();
    stamp(p, 1);

    int chunk = 0, g = 0, half = 0, s = 0;
    auto step = [&](auto taps_tag, float (&acur)[16], float (&apre)[16]) __attribute__((always_inline)) {
        constexpr int TAPS = decltype(taps_tag)::value;
        const float *cur = (chunk & 1) ? buf1 : buf0;
        if (s + (RING - 1) < nsteps && !((p.dbg & 1) && s > 3)) load_a(apre, s + (RING - 1));
        if (g == 0 && half == 0) {
            if (chunk + 1 < p.nchunks && !(p.dbg & 2)) stage_store((chunk & 1) ? buf0 : buf1, chunk + 1);
            if (chunk + 2 < p.nchunks && !(p.dbg & 2)) stage_load(chunk + 2);
        }
        const float *xq[4];
        {
            const float *rowp = cur + (half * 8 + lhalf) * RP;
            const int t3 = 3 * g;
            if constexpr (DIL == 1) {
                const int ga = (t3 & 1) ? H + (t3 >> 1) : (t3 >> 1);             // x0, x2
                const int gb = (t3 & 1) ? ((t3 + 1) >> 1) : H + (t3 >> 1);       // x1, x3
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int e = wn * PW + (posr[j] >> 1);
                    xq[2 * j] = rowp + e + ga;
                    xq[2 * j + 1] = rowp + e + gb;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    xq[2 * j] = rowp + wn * NBW + posr[j] + t3 * DIL;
                    xq[2 * j + 1] = xq[2 * j] + DIL;
                }
            }
        }
        wino_half_step<DIL, TAPS>(acc, acur, xq[0], xq[1], xq[2], xq[3], RP);
        ++s;
        if (++half == 2) {
            half = 0;
            if (++g == G) {
                __syncthreads();
                g = 0;
                ++chunk;
            }
        }
    };
    constexpr std::integral_constant<int, 3> F3{};
    if constexpr (TG == 3) {
        // three tap groups -> six half-steps per chunk, a multiple of the ring period: straight-line code.  k = 7 (TT = 1): the
        // last two half-steps in the direct form on M0 / M3; k = 9 (TT = 3): all six F(2,3).
        static_assert(RING == 3, "the k-specialised instances use the 3-slot ring");
        constexpr std::integral_constant<int, TT> TL{};
        for (int c = 0; c < p.nchunks; ++c) {
            step(F3, a0, a2); step(F3, a1, a0); step(F3, a2, a1); step(F3, a0, a2);
            step(TL, a1, a0); step(TL, a2, a1);
        }
    } else if constexpr (TG == 4) {
        // k = 11: groups (3, 3, 3, 2 taps) -> eight half-steps per chunk on the 2-slot ring, the last two as F(2,2)
        constexpr std::integral_constant<int, TT> TL{};
        for (int c = 0; c < p.nchunks; ++c) {
            step(F3, a0, a1); step(F3, a1, a0); step(F3, a0, a1); step(F3, a1, a0); step(F3, a0, a1); step(F3, a1, a0);
            step(TL, a0, a1); step(TL, a1, a0);
        }
    } else if constexpr (RING == 3) {
        while (s < nsteps) {
            step(F3, a0, a2);
            if (s < nsteps) step(F3, a1, a0);
            if (s < nsteps) step(F3, a2, a1);
        }
    } else {
        while (s < nsteps) {       // nsteps is even
            step(F3, a0, a1);
            step(F3, a1, a0);
        }
    }

    stamp(p, 2);
    // ------------------------------------------------------------------------------------------------- epilogue
    // output transform in place: acc[0] <- y[t(c)], acc[3] <- y[t(c) + d]
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float m1 = acc[1][j][r], m2 = acc[2][j][r];
            acc[0][j][r] = acc[0][j][r] + m1 + m2;
            acc[3][j][r] = m1 - m2 - acc[3][j][r];
        }

    const OutSpec o = p.out[0];
    const int tile_row0 = mt0 * 32;
    const bool has_res = o.res != nullptr, has_acc = o.acc != nullptr;
    const bool use_mask = (o.out_mask != 0);
    float *const yb = o.y + (long long)b * o.y_bs;
    const float *const resp = has_res ? o.res + (long long)b * o.res_bs : nullptr;
    const float *const accp = has_acc ? o.acc + (long long)b * o.acc_bs : nullptr;
    const int nw = n0 + wn * NBW;                // first output of this wave
    // pair column -> output position, recomputed from an opaque copy of the lane id (see below: keeps it out of the prologue)
    int lane_e = lane;
    asm volatile("" : "+v"(lane_e));
    int posw[2], pose[2];
    bool cvalid[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = j * 32 + (lane_e & 31);
        const int t = (c / DIL) * (2 * DIL) + (c % DIL);
        cvalid[j] = c < PW;
        posw[j] = cvalid[j] ? t : NBW;       // idle columns write to the dump columns of the transposition buffer
        pose[j] = cvalid[j] ? t : 0;
    }

    if (p.fast_epi && (n0 + BN <= p.N) && (tile_row0 + 32 <= p.M)) {
        constexpr int VEC = (DIL == 1) ? 4 : 2;
        constexpr int LPR = NBW / VEC;           // lanes per row
        constexpr int RPI = 64 / LPR;            // rows per wave-instruction
        constexpr int NIT = 8 / RPI;
        typedef float vecf __attribute__((ext_vector_type(VEC)));
        float *const Lw = smem + wave * 8 * CWP;
        // Everything below depends only on the lane and the launch parameters, so hipcc computes the 64-bit row addresses of
        // the epilogue BEFORE the main loop and spills them across it (17-48 dwords per lane = 1 KB of scratch traffic per
        // dword and workgroup, written and read back: +15..50 % of a workgroup's HBM traffic).  An opaque copy of the lane id
        // taken after the loop keeps that arithmetic here.
        const int lrow = lane_e / LPR;
        const int cv = (lane_e % LPR) * VEC;
        const bool active = lane_e < LPR * RPI;
        const int colg = nw + cv;
        vecf mv;
#pragma unroll
        for (int e = 0; e < VEC; ++e) mv[e] = 1.f;
        if (use_mask && active) mv = *reinterpret_cast<const vecf *>(maskb + colg);
        // Residual / accumulate reads: every 8-row pass needs one HBM round trip (2-3 us with the chip in its epilogues), and
        // four of them in sequence were 11 us of a 50 us workgroup at k=3 (tools/conv_stamps.py) -- so the reads of ALL
        // passes are issued before the first use (64 registers, free now that the fragment ring and the staging registers
        // are dead); with an accumulate input as well, two passes at a time.  Loads of a batch precede its stores and every
        // lane stores exactly the elements it loaded, so y may alias res / acc.
        // SIMPLE = no accumulate input, no scale, no activation, no mask (the inner resblock convs: 5 of 6 launches): the
        // per-element work is LDS read + residual add + store with no branch in it (every runtime `if` inside these unrolled
        // loops is a scalar branch per element group, and the epilogue's instruction stream is what it costs).
        auto run = [&](auto pb_tag, auto simple_tag, auto res_tag) __attribute__((always_inline)) {
            constexpr int PB = decltype(pb_tag)::value;
            constexpr bool SIMPLE = decltype(simple_tag)::value;
            constexpr bool RES = decltype(res_tag)::value;
#pragma unroll
            for (int pb = 0; pb < 4 / PB; ++pb) {
                vecf r4[PB][NIT], a4[PB][NIT];
#pragma unroll
                for (int u = 0; u < PB; ++u)
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const long long goff = (long long)(tile_row0 + 8 * (pb * PB + u) + it * RPI + lrow) * p.Tout + colg;
                        if (active) {
                            if constexpr (RES) r4[u][it] = *reinterpret_cast<const vecf *>(resp + goff);
                            if constexpr (!SIMPLE) {
                                if (has_acc) a4[u][it] = *reinterpret_cast<const vecf *>(accp + goff);
                            }
                        }
                    }
#pragma unroll
                for (int u = 0; u < PB; ++u) {
                    const int ps = pb * PB + u;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const float y0 = acc[0][j][4 * ps + q], y1 = acc[3][j][4 * ps + q];
                            if constexpr (DIL == 1) {      // the pair is adjacent: one 8-byte write, unit stride across lanes
                                *reinterpret_cast<float2 *>(Lw + (q + 4 * lhalf) * CWP + posw[j]) = make_float2(y0, y1);
                            } else {
                                Lw[(q + 4 * lhalf) * CWP + posw[j]] = y0;
                                Lw[(q + 4 * lhalf) * CWP + posw[j] + DIL] = y1;
                            }
                        }
                    }
                    if (active) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) {
                            const long long goff = (long long)(tile_row0 + 8 * ps + it * RPI + lrow) * p.Tout + colg;
                            vecf v = *reinterpret_cast<const vecf *>(Lw + (it * RPI + lrow) * CWP + cv);
                            if constexpr (RES) v += r4[u][it];
                            if constexpr (!SIMPLE) {
                                if (has_acc) v += a4[u][it];
                                v *= o.scale;
                                if (o.out_act != VS_OUT_NONE) {
#pragma unroll
                                    for (int e = 0; e < VEC; ++e) {
                                        if (o.out_act == VS_OUT_TANH) v[e] = tanh_fast(v[e]);
                                        else if (o.out_act == VS_OUT_RELU) v[e] = fmaxf(v[e], 0.f);
                                    }
                                }
                                v *= mv;
                            }
                            *reinterpret_cast<vecf *>(yb + goff) = v;
                        }
                    }
                }
            }
        };
        const bool simple = !has_acc && o.scale == 1.f && o.out_act == VS_OUT_NONE && !use_mask;
        if (simple) {
            if (has_res) run(std::integral_constant<int, 2>{}, std::true_type{}, std::true_type{});
            else run(std::integral_constant<int, 2>{}, std::true_type{}, std::false_type{});
        } else if (has_res) {
            run(std::integral_constant<int, 2>{}, std::false_type{}, std::true_type{});
        } else {
            run(std::integral_constant<int, 2>{}, std::false_type{}, std::false_type{});
        }
    } else {
        // edge workgroups (ragged last time tile): element-wise, predicated stores, clamped loads
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int col = nw + pose[j] + hh * DIL;
                const bool okc = cvalid[j] && (col < p.N);
                const int colc = min(col, p.Tout - 1);
                const float mval = use_mask ? maskb[colc] : 1.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = tile_row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane_e >> 5);
                    const int rowc = min(row, p.M - 1);
                    const long long off = (long long)rowc * p.Tout + colc;
                    float v = (hh == 0 ? acc[0][j][r] : acc[3][j][r]);
                    if (has_res) v += resp[off];
                    if (has_acc) v += accp[off];
                    v *= o.scale;
                    if (o.out_act == VS_OUT_TANH) v = tanh_fast(v);
                    else if (o.out_act == VS_OUT_RELU) v = fmaxf(v, 0.f);
                    v *= mval;
                    if (okc && row < p.M) yb[off] = v;
                }
            }
        }
    }
    if (p.stamps) {
        stamp(p, 6);                     // epilogue issued
        __builtin_amdgcn_s_waitcnt(0);   // all stores acknowledged
        stamp(p, 3);
    }
}

template <int DIL, int WAVES_M, int WAVES_N, int TG = 0, int TT = 3>
static int launch_wino(const ConvParams &p, hipStream_t s) {
    constexpr int NBW = 2 * ((64 / DIL) * DIL);
    constexpr int BN = NBW * WAVES_N;
    auto kern = conv_wino_kernel<DIL, WAVES_M, WAVES_N, TG, TT>;
    const int Wh = (p.W + 1) >> 1, H = ((Wh + 15) & ~31) + 16;
    const int RP = (DIL == 1) ? H + Wh : p.W;      // LDS row pitch, as computed by the kernel
    const size_t lds = sizeof(float) * std::max<size_t>((size_t)2 * CK * RP, (size_t)WAVES_M * WAVES_N * 8 * (NBW + 8));
    static bool attr_set = false;
    if (!attr_set) {
        VS_CHECK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    dim3 grid((unsigned)ceil_div(p.N, BN), (unsigned)ceil_div(p.MT, WAVES_M), (unsigned)p.B);
    hipLaunchKernelGGL(kern, grid, dim3(64 * WAVES_M * WAVES_N), lds, s, p);
    VS_CHECK_HIP(hipGetLastError());
    set_last_kernel("conv_wino_kernel<%d, %d, %d, %d, %d>", DIL, WAVES_M, WAVES_N, TG, TT);
    return VS_OK;
}

template <int DIL>
static int launch_wino_dil(ConvParams &p, int MT, int span_w, int spec, hipStream_t s) {
    // spec: 0 generic (zero-padded last group), 7 / 11: the k-specialised straight-line instances
    // (k = 9 through the same structure, TG = 3 / TT = 3, measured +1 %: not instantiated)
    constexpr int NBW = 2 * ((64 / DIL) * DIL);
    if (MT % 4 == 0) {
        p.W = NBW + span_w;
        if (spec == 7) return launch_wino<DIL, 4, 1, 3, 1>(p, s);
        if (spec == 11) return launch_wino<DIL, 4, 1, 4, 2>(p, s);
        return launch_wino<DIL, 4, 1>(p, s);
    }
    if (MT % 2 == 0) {
        p.W = 2 * NBW + span_w;
        if (spec == 7) return launch_wino<DIL, 2, 2, 3, 1>(p, s);
        if (spec == 11) return launch_wino<DIL, 2, 2, 4, 2>(p, s);
        return launch_wino<DIL, 2, 2>(p, s);
    }
    p.W = 4 * NBW + span_w;
    if (spec == 11 && DIL == 1) return launch_wino<1, 1, 4, 4, 2>(p, s);
    return launch_wino<DIL, 1, 4>(p, s);
}

// p as vs_conv_forward fills it for the direct engine, on a handle with wino_groups whose transform is packed (pack_wino_weights)
int launch_wino_conv(const vs_conv *h, const ConvParams &p, hipStream_t s) {
    ConvParams q = p;
    q.wp = h->wpw.as<float>();
    q.KT = h->wino_groups;
    q.lo = -h->pad;
    q.dbg = (int)opt(OPT_WINO_DBG);
    // the vector epilogue stores float4 (dilation 1) / float2 runs: same alignment preconditions as the direct engine's
    // (Tout % 4 == 0 of fast_epi covers both)
    const int span_w = 3 * h->wino_groups * h->dil;
    const int spec = h->wino_k7 ? 7 : (h->wino_k11 ? 11 : 0);
    if (h->dil == 1) return launch_wino_dil<1>(q, h->MT, span_w, spec, s);
    if (h->dil == 3) return launch_wino_dil<3>(q, h->MT, span_w, spec, s);
    return launch_wino_dil<5>(q, h->MT, span_w, spec, s);
}

}  // namespace vs
