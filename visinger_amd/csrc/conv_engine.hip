// conv_engine.hip -- the implicit-GEMM 1-D convolution engine of the VISinger hot path on gfx950.
//
// One kernel family serves every nn.Conv1d / nn.ConvTranspose1d of the path (reference sites listed in
// include/visinger_hip.h).  It is an implicit GEMM on the exact-fp32 matrix instruction
// v_mfma_f32_32x32x2_f32 (bit-identical to a k-ordered fmaf chain, 64 FLOP/clk/SIMD = the fp32 peak of the chip):
//
//     D[m, n] = sum_{tap} sum_{ci}  Wp[tap][m][ci] * f(x[b, ci, n + off(tap)])
//
//   * A operand = weights, pre-packed ONCE on the device into fragment order Wp[m_tile][tap][chunk][quad][64 lanes][4]
//     (lane l holds W[m_tile*32 + (l&31)][2*ci_pair + (l>>5)] for the four ci_pairs of the quad) so a wave fetches four
//     fragments with one coalesced 1-KiB load (served by L2/L1: the weights of a conv are <= 3 MB and shared by every
//     workgroup);
//   * B operand = activations, staged ONCE per (ci-chunk, time tile + halo) into LDS as Xs[ci][n]; every tap reads
//     a shifted window of the same LDS rows (conflict-free ds_read_b32: 32 consecutive dwords per half-wave), so
//     HBM/L2 sees each activation once per M-block no matter how many taps the conv has;
//   * transposed convs run as a polyphase conv over "virtual rows" m = phase*C_out + co with per-tile tap
//     ranges (no multiplies by structural zeros) and an interleaving store;
//   * the input transform (leaky-relu / mask) is applied while staging; bias, conditioning bias, residual add,
//     accumulate, scale, tanh, mask, WaveNet gate, res/skip split and the affine-coupling update (+ log-det
//     wave-shuffle reduction) are fused into the epilogue, so no elementwise kernel ever touches HBM.
//
// Tile: 4 waves (256 threads), each wave owns MT_W x NT_W accumulator tiles of 32x32 (16 VGPRs each); two
// workgroups per CU (2 waves/SIMD) hide the staging of one behind the MFMAs of the other.
#include "conv_common.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <type_traits>

namespace vs {

thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- dispatch switches: see vs_internal.h (enum Opt).  Read from the environment ONCE, when the library is loaded.
struct OptEntry { const char *name; long long dflt; long long value; };
static OptEntry g_opts[OPT_COUNT] = {
    {"VS_CONV_MATH", -1, -1}, {"VS_NO_SMALL_CONV", 0, 0}, {"VS_NO_FAST_EPI", 0, 0}, {"VS_WINO_FORCE", 0, 0}, {"VS_NO_WINO", 0, 0},
    {"VS_NO_WINO_K7", 0, 0}, {"VS_WINO_DBG", 0, 0},
    {"VS_NO_SMALL_GRID", 0, 0}, {"VS_SMALL_GRID_T6", 512, 512}, {"VS_CONV_CFG", -1, -1}, {"VS_SPLIT_DBG", 0, 0}, {"VS_TRACE", 0, 0},
    {"VS_NO_BF16_ATTN", 0, 0}, {"VS_NO_SPLIT_ATTN", 0, 0}, {"VS_NO_WGRAD_SPLIT", 0, 0}, {"VS_RB_TILE256", 0, 0},
    {"VS_NO_ATTN_KVPACK", 0, 0}, {"VS_NO_TR_EPI", 0, 0}, {"VS_NO_KTAP", 0, 0}, {"VS_NO_ATTN_DMA", 0, 0},
    {"VS_ATTN_DMA_ONE_WAVE", 0, 0}, {"VS_ATTN_SPLIT6", 0, 0}, {"VS_NO_T1_CONV", 0, 0},
};
static const bool g_opts_loaded = [] {
    for (OptEntry &e : g_opts) {
        const char *v = getenv(e.name);
        if (v && *v) {
            char *end = nullptr;
            const long long n = strtoll(v, &end, 10);
            e.value = (end != v) ? n : 1;          // (a non-numeric value counts as "set")
        }
    }
    return true;
}();
long long opt(Opt o) { return g_opts[o].value; }

// the table entry of `name`, or NULL with the error string set on behalf of the ABI function `fn`
static OptEntry *find_opt(const char *fn, const char *name) {
    for (OptEntry &e : g_opts)
        if (strcmp(e.name, name) == 0) return &e;
    set_error("%s: unknown option %s", fn, name);
    return nullptr;
}

thread_local char g_last_kernel[160] = "";
void set_last_kernel(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_kernel, sizeof(g_last_kernel), fmt, ap);
    va_end(ap);
}

// ---- cross-stream ordering of a handle's packed state: see vs_internal.h (StreamOrder).  Both functions touch the HIP runtime only when a
// stream meets a handle version for the first time; a launch on a known stream costs the comparison in order_read.
static bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) {
        (void)hipGetLastError();
        return true;                    // (cannot tell: leave the stream alone)
    }
    return st != hipStreamCaptureStatusNone;
}

// stream `waiter` waits for everything issued to stream `tail` so far
static int wait_for_tail(StreamOrder &o, hipStream_t waiter, hipStream_t tail) {
    if (!o.ev) VS_CHECK_HIP(hipEventCreateWithFlags(&o.ev, hipEventDisableTiming));
    VS_CHECK_HIP(hipEventRecord(o.ev, tail));
    VS_CHECK_HIP(hipStreamWaitEvent(waiter, o.ev, 0));      // (the wait holds the record made above: the event may be recorded again at once)
    return VS_OK;
}

int order_read_slow(vs_conv *h, hipStream_t s) {
    StreamOrder &o = h->order;
    for (hipStream_t k : o.known)
        if (k == s) {
            o.last = s;
            o.any = true;
            return VS_OK;
        }
    if (o.known.empty()) return VS_OK;          // nothing produced yet (the entry points refuse such a handle themselves)
    if (stream_capturing(s)) return VS_OK;
    VS_TRY(wait_for_tail(o, s, o.known[0]));
    o.known.push_back(s);
    o.last = s;
    o.any = true;
    return VS_OK;
}

int order_write(vs_conv *h, hipStream_t s) {
    StreamOrder &o = h->order;
    if (o.known.size() == 1 && o.known[0] == s) return VS_OK;
    if (!o.known.empty()) {
        if (stream_capturing(s)) return VS_OK;
        for (hipStream_t k : o.known)
            if (k != s) VS_TRY(wait_for_tail(o, s, k));
    }
    o.known.assign(1, s);
    o.last = s;
    o.any = true;
    return VS_OK;
}


template <int MT_W, int NT_W, int WAVES_M, int WAVES_N>
__global__ void __launch_bounds__(64 * WAVES_M * WAVES_N, 2) conv_mfma_kernel(const ConvParams p) {
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int BN = 32 * NT_W * WAVES_N;
    constexpr int MAXW = BN + MAX_SPAN;
    constexpr int RPW = CK / NW;                 // LDS rows staged per wave
    constexpr int CIT = (MAXW + 63) / 64;        // column iterations per row
    static_assert(CK % NW == 0, "CK must be a multiple of the wave count");
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WAVES_M;
    const int wn = wave / WAVES_M;
    const int b = blockIdx.z;
    const int n0 = blockIdx.x * BN;
    const int mt0 = (blockIdx.y * WAVES_M + wm) * MT_W;
    const int W = p.W;
    float *const buf0 = smem;
    float *const buf1 = smem + CK * W;
    const float *const xb = p.x + (long long)b * p.x_bs;
    const float *const maskb = p.mask ? p.mask + (long long)b * p.Tin : nullptr;

    // ---- tap range of this wave (polyphase transposed conv: skip the structurally-zero taps) ----
    int tap_b = 0, tap_e = p.KT;
    if (p.kind == VS_CONV_TRANSPOSE1D && (p.c_out & 31) == 0) {
        // every 32-row tile has one phase; MT_W tiles of a wave may differ -> union
        int lo_t = p.KT, hi_t = 0;
#pragma unroll
        for (int i = 0; i < MT_W; ++i) {
            const int phase = ((mt0 + i) * 32) / p.c_out;
            if (phase < p.up) {
                // delta range with 0 <= delta*up + phase + pad < K
                const int num_lo = -(phase + p.uppad);                    // delta >= ceil(num_lo / up)
                const int dlo = (num_lo >= 0) ? (num_lo + p.up - 1) / p.up : -((-num_lo) / p.up);
                const int num_hi = p.upK - 1 - phase - p.uppad;           // delta <= floor(num_hi / up)
                const int dhi = (num_hi >= 0) ? num_hi / p.up : -((-num_hi + p.up - 1) / p.up);
                lo_t = min(lo_t, dlo - p.dmin);
                hi_t = max(hi_t, dhi - p.dmin + 1);
            }
        }
        tap_b = max(0, lo_t);
        tap_e = min(p.KT, hi_t);
        // a wave whose tiles are all padding (M tiles rounded up to the workgroup) has no tap of its own, but it still owns
        // LDS rows of every chunk and a seat at every chunk barrier: give it one tap (its packed weights are zeros)
        if (tap_e <= tap_b) { tap_b = 0; tap_e = 1; }
    }

    // The accumulators start from the bias (+ the per-item conditioning bias) of their row instead of zero: the same 128
    // v_mov, and the epilogue loses one VALU add per element -- a VALU instruction of a wave in its epilogue waits for a gap
    // in the co-resident workgroup's MFMA stream (~one MFMA slot each, tools/conv_stamps.py), so epilogue time is
    // proportional to its VALU count.
    const float *const bbias = p.bias_b ? p.bias_b + (long long)b * p.bias_b_bs : nullptr;
    f32x16 acc[MT_W][NT_W];
#pragma unroll
    for (int i = 0; i < MT_W; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rt = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int m = (mt0 + i) * 32 + rt;                 // virtual row (biasp is zero-padded to whole tiles)
            float bv = p.biasp[m];
            if (bbias) {
                int row;
                if constexpr (MT_W == 2) {                     // paired rows: tile 2q -> c, tile 2q+1 -> Hh + c
                    row = (i & 1) * p.Hh + min((mt0 >> 1) * 32 + rt, p.Hh - 1);
                } else {
                    const int mc = min(m, p.M - 1);
                    row = (p.kind == VS_CONV_TRANSPOSE1D) ? mc % p.c_out : mc;
                }
                bv += bbias[row];
            }
#pragma unroll
            for (int j = 0; j < NT_W; ++j) acc[i][j][r] = bv;
        }

    float st[RPW][CIT];
    float mk[CIT];
    const int in_act = p.in_act;

    // Staging loads are UNCONDITIONAL buffer loads (one 32-bit offset VGPR per LDS row, the column iterations are
    // immediate offsets; out-of-range bytes of the item's [Cin, Tin] slab read as 0 by the descriptor's bounds check)
    // and the zero-fill of the halo is applied when the registers are written to LDS: a predicated load makes hipcc
    // branch around every load and drain vmcnt(0) per element, and 64-bit per-load addresses cost 2 VGPRs each.
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
    // The zero-fill of the halo only exists in the first / last time tiles and in a partial last channel chunk, and the input
    // transform is one of four: both are wave-uniform, so the per-element work of the common case (interior tile, leaky-relu)
    // is mul + max + ds_write instead of compare / select / compare / select / multiply-select / predicated write.
    const bool time_edge = (n0 + p.lo < 0) || (n0 + p.lo + W > p.Tin);
    auto stage_store = [&](float *buf, int chunk) __attribute__((always_inline)) {
        auto run = [&](auto edge_tag, auto act_tag) __attribute__((always_inline)) {
            constexpr bool EDGE = decltype(edge_tag)::value;
            constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
            for (int i = 0; i < CIT; ++i) {
                const int col = lane + 64 * i;
                const int n = n0 + p.lo + col;
                const bool okn = (n >= 0) && (n < p.Tin);
#pragma unroll
                for (int j = 0; j < RPW; ++j) {
                    float v = st[j][i];
                    if constexpr (EDGE) v = (okn && (chunk * CK + wave + NW * j < p.Cin)) ? v : 0.f;
                    if constexpr (ACT == VS_IN_LRELU || ACT == VS_IN_LRELU_MASK) v = fmaxf(v, 0.1f * v);
                    if constexpr (ACT >= VS_IN_MASK) v *= mk[i];
                    if (64 * (i + 1) <= BN || col < W) buf[(wave + NW * j) * W + col] = v;      // W >= BN
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

    const int lhalf = lane >> 5;
    const int l31 = lane & 31;

    // ---------------------------------------------------------------------------------------------- main loop
    // The K loop is flattened into steps s = (chunk, tap); a step is 8 groups (one per input-channel pair) of
    // MT_W*NT_W MFMAs.  Software pipeline (hipcc builds none by itself):
    //   * A fragments (packed weights, L2-resident): 3-deep register ring rotated by NAME (the step loop is unrolled
    //     by 3; a rotating copy would read the slot being prefetched); the slot of step s+2 is requested at step s;
    //   * activations: chunk c+2 is requested at the first tap of chunk c, right AFTER that step's A prefetch (vmcnt
    //     retires in issue order: whatever is issued behind them completes behind them) and stays in registers for a
    //     whole chunk; chunk c+1 is written to the other LDS buffer at the same point;
    //   * B fragments of group g+1 are read from LDS under the MFMAs of group g, pinned above them by sched_barrier
    //     (left alone hipcc sinks each ds_read next to its consumer: ds_read2 -> lgkmcnt(0) -> 2 MFMA).
    // Tried and measured worse (tools/conv_stamps.py, per-step shader cycles): inline-asm ring loads with hand-counted
    // vmcnt (same), staging pieces spread over the gaps between groups (+8 %: a lone wave hides only ~64 cycles of
    // non-MFMA issue per gap).
    const int ntaps = tap_e - tap_b;
    const int nsteps = p.nchunks * ntaps;
    const float *wbase[MT_W];
#pragma unroll
    for (int i = 0; i < MT_W; ++i) wbase[i] = p.wp + (long long)(mt0 + i) * p.KT * p.CP * 64 + lane * 4;
    float a0[MT_W][CK / 2], a1[MT_W][CK / 2], a2[MT_W][CK / 2];
    // (the 8 fragments of a step are stored as two lane-interleaved quads: two 16-byte loads, 1 KiB per wave-instruction)
    auto load_a = [&](float (&dst)[MT_W][CK / 2], int chunk, int tap) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MT_W; ++i) {
            const float *src = wbase[i] + ((long long)tap * p.nchunks + chunk) * (CK / 2) * 64;
#pragma unroll
            for (int qd = 0; qd < 2; ++qd) {
                const float4 t = *reinterpret_cast<const float4 *>(src + qd * 256);
                dst[i][qd * 4 + 0] = t.x; dst[i][qd * 4 + 1] = t.y; dst[i][qd * 4 + 2] = t.z; dst[i][qd * 4 + 3] = t.w;
            }
        }
    };
    // (chunk, tap) of the step two ahead of the current one
    int pc = 0, pt = tap_b;
    auto advance = [&]() __attribute__((always_inline)) { if (++pt == tap_e) { pt = tap_b; ++pc; } };
    if (nsteps > 0) { load_a(a0, pc, pt); advance(); }
    if (nsteps > 1) { load_a(a1, pc, pt); advance(); }

    stamp(p, 0);
    stage_load(0);
    stage_store(buf0, 0);
    if (p.nchunks > 1) stage_load(1);      // lives in registers during chunk 0
    __syncthreads();
    stamp(p, 1);

    int chunk = 0, tap = tap_b, s = 0;
    auto step = [&](float (&acur)[MT_W][CK / 2], float (&apre)[MT_W][CK / 2]) __attribute__((always_inline)) {
        const float *cur = (chunk & 1) ? buf1 : buf0;
        const bool more = (chunk + 1 < p.nchunks);
        if (s + 2 < nsteps) { load_a(apre, pc, pt); advance(); }
        if (tap == tap_b) {
            // chunk c+1 (requested one whole chunk ago) goes to the other LDS buffer, which every wave finished reading
            // at the barrier that ended chunk c-1; then chunk c+2 is requested: a full chunk of MFMAs hides its latency
            // whatever the tap count (with the request at the first tap and the store at the last one, a 1-tap conv
            // waited for HBM in every step)
            if (more) stage_store((chunk & 1) ? buf0 : buf1, chunk + 1);
            if (chunk + 2 < p.nchunks) stage_load(chunk + 2);
        }

        const float *xs = cur + lhalf * W + wn * (NT_W * 32) + l31 - p.lo + (p.off0 + tap * p.tstep);
        float bf[NT_W], bn[NT_W];
#pragma unroll
        for (int j = 0; j < NT_W; ++j) bf[j] = xs[j * 32];
#pragma unroll
        for (int cp = 0; cp < CK / 2; ++cp) {
            if (cp + 1 < CK / 2) {
#pragma unroll
                for (int j = 0; j < NT_W; ++j) bn[j] = xs[(cp + 1) * 2 * W + j * 32];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MT_W; ++i)
#pragma unroll
                for (int j = 0; j < NT_W; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(acur[i][cp], bf[j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NT_W; ++j) bf[j] = bn[j];
        }
        if (++tap == tap_e) {
            __syncthreads();
            tap = tap_b;
            ++chunk;
        }
        ++s;
    };
    while (s < nsteps) {
        step(a0, a2);
        if (s < nsteps) step(a1, a0);
        if (s < nsteps) step(a2, a1);
    }

    stamp(p, 2);
#include "conv_epilogue.inc"
    if (p.stamps) {
        __builtin_amdgcn_s_waitcnt(0);   // all stores acknowledged
        stamp(p, 3);
    }
}

// logdet[b] += sum of the item's per-tile partials, in a fixed order: lane l adds slots l, l + 64, ... sequentially, then a wavefront-shuffle
// butterfly (commutative per step: every lane ends with the same bits).  One wave per item; a few hundred slots.
__global__ void logdet_reduce_kernel(const float *__restrict__ part, int slots, float *__restrict__ logdet) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < slots; i += 64) s += part[(long long)b * slots + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) logdet[b] += s;
}

static inline int floor_div(int a, int b) { return (a >= 0) ? a / b : -((-a + b - 1) / b); }
static inline int ceil_div_i(int a, int b) { return -floor_div(-a, b); }

}  // namespace vs

// ---------------------------------------------------------------------------------------------------------------
// C ABI: errors and options, handles, vs_conv_forward.  (Weights and arithmetic of a handle: conv_pack.hip.)

unsigned long long *g_stamp_buf = nullptr;   // debug hook, see vs_debug_set_stamp_buffer (also read by resblock_pair_split.hip)

using namespace vs;

template <int MT_W, int NT_W, int WAVES_M, int WAVES_N>
static int launch_cfg(const ConvParams &p, hipStream_t s) {
    constexpr int BN = 32 * NT_W * WAVES_N;
    constexpr int BM_TILES = MT_W * WAVES_M;
    auto kern = conv_mfma_kernel<MT_W, NT_W, WAVES_M, WAVES_N>;
    const size_t lds = (size_t)2 * CK * p.W * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        VS_CHECK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    dim3 grid((unsigned)ceil_div(p.N, BN), (unsigned)ceil_div(p.MT, BM_TILES), (unsigned)p.B);
    hipLaunchKernelGGL(kern, grid, dim3(64 * WAVES_M * WAVES_N), lds, s, p);
    VS_CHECK_HIP(hipGetLastError());
    set_last_kernel("conv_mfma_kernel<%d, %d, %d, %d>", MT_W, NT_W, WAVES_M, WAVES_N);
    return VS_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// The stages of vs_conv_forward, in the order it calls them.  The routes in units of their own (conv_small.hip, conv_wino.hip,
// conv_ktap*.hip, conv_split.hip) are declared in conv_common.h.

// the io argument of the conv_ktap instance tables: bit 0 -- x, bit 1 -- y / res / acc hold bf16 elements
static int io_bits(const ConvParams &p) { return (p.x_bf16 ? 1 : 0) | (p.y_bf16 ? 2 : 0); }

// 1. validate the launch and fill the parameters every route starts from
static int fill_params(const vs_conv *h, const vs_conv_io_t *io, ConvParams &p) {
    VS_REQUIRE(h && io, "vs_conv_forward: NULL handle or io");
    VS_REQUIRE(h->weights_set, "vs_conv_forward: weights not set");
    VS_REQUIRE(io->x && io->B > 0 && io->T > 0, "vs_conv_forward: bad input");
    VS_REQUIRE(io->out[0].y, "vs_conv_forward: out[0].y is NULL");
    const int64_t Tout = vs_conv_out_len(h, io->T);
    VS_REQUIRE(Tout > 0, "vs_conv_forward: empty output");
    VS_REQUIRE(io->B <= 65535, "vs_conv_forward: B too large for grid.z");
    memset(&p, 0, sizeof(p));
    p.x = io->x;
    p.x_bs = io->x_bs ? io->x_bs : (long long)h->c_in * io->T;
    p.wp = h->wp.as<float>();
    p.biasp = h->biasp.as<float>();
    p.bias_b = io->bias_b;
    p.bias_b_bs = io->bias_b_bs ? io->bias_b_bs : h->c_out;
    p.mask = io->mask;
    p.logdet = io->logdet;
    p.kind = h->kind;
    p.pair_mode = io->pair_mode;
    p.in_act = io->in_act;
    p.B = (int)io->B; p.Cin = h->c_in; p.Tin = (int)io->T;
    p.M = h->M; p.MT = h->MT; p.c_out = h->c_out; p.Hh = h->Hh;
    p.Tout = (int)Tout;
    p.N = (h->kind == VS_CONV_TRANSPOSE1D) ? (int)ceil_div(Tout, h->dil) : (int)Tout;
    p.KT = h->KT; p.CP = h->CP; p.nchunks = h->nchunks;
    p.off0 = h->off0; p.tstep = h->tstep; p.lo = h->lo;
    p.stamps = g_stamp_buf;
    p.up = (h->kind == VS_CONV_TRANSPOSE1D) ? h->dil : 1;
    p.upK = h->k; p.uppad = h->pad; p.dmin = h->dmin;
    p.row_lo = 0;            // every row is stored (only the two passes of an odd split_row narrow the range: forward_tiles)
    p.row_hi = h->c_out;
    const int rows_out = (h->kind == VS_CONV1D_PAIRED) ? h->Hh : h->c_out;
    p.split_row = (io->split_row > 0 && io->split_row < rows_out && h->kind != VS_CONV1D_PAIRED) ? io->split_row : 0;
    VS_REQUIRE((io->x_dtype == VS_DTYPE_F32 || io->x_dtype == VS_DTYPE_BF16) && (io->y_dtype == VS_DTYPE_F32 || io->y_dtype == VS_DTYPE_BF16),
               "vs_conv_forward: unknown element type");
    p.x_bf16 = io->x_dtype == VS_DTYPE_BF16;
    p.y_bf16 = io->y_dtype == VS_DTYPE_BF16;
    if (p.x_bf16 || p.y_bf16) {
        VS_REQUIRE(h->math == VS_MATH_BF16, "vs_conv_forward: bf16-resident tensors need the plain-bf16 arithmetic (VS_MATH_BF16)");
        VS_REQUIRE(h->kind != VS_CONV1D_PAIRED && !p.split_row && (io->out[0].mode == VS_OUT_LINEAR || !p.y_bf16),
                   "vs_conv_forward: bf16-resident tensors go with plain LINEAR launches (no PAIRED kind, no split_row)");
    }
    bool need_mask = (io->in_act >= VS_IN_MASK);
    bool need_out_mask = false;      // a mask indexed by OUTPUT position: only defined where T_out == T (never for a transposed conv)
    VS_REQUIRE(io->in_act >= VS_IN_NONE && io->in_act <= VS_IN_LRELU_MASK, "vs_conv_forward: bad in_act");
    for (int s = 0; s < 2; ++s) {
        const vs_conv_out_t &o = io->out[s];
        OutSpec &d = p.out[s];
        const int rows = (s == 0) ? (p.split_row ? p.split_row : rows_out) : (rows_out - p.split_row);
        const long long dflt = (long long)rows * Tout;
        d.y = o.y; d.res = o.res; d.acc = o.acc;
        d.y_bs = o.y_bs ? o.y_bs : dflt; d.res_bs = o.res_bs ? o.res_bs : dflt; d.acc_bs = o.acc_bs ? o.acc_bs : dflt;
        d.scale = (o.scale == 0.f) ? 1.f : o.scale;   // 0 = unset
        d.out_act = o.out_act; d.out_mask = o.out_mask; d.mode = o.mode;
        d.rows = rows;
        if (s == 0 || p.split_row) {
            need_out_mask |= (o.out_mask != 0) || (o.mode != VS_OUT_LINEAR);
            VS_REQUIRE(o.mode == VS_OUT_LINEAR || o.res, "vs_conv_forward: coupling mode needs res (x1)");
        }
    }
    VS_REQUIRE(!p.split_row || io->out[1].y, "vs_conv_forward: split_row set but out[1].y is NULL");
    VS_REQUIRE(h->kind != VS_CONV_TRANSPOSE1D || (!io->out[0].res && !io->out[0].acc && !p.split_row),
               "vs_conv_forward: res / acc / split_row are not supported with a transposed conv");
    VS_REQUIRE((long long)h->c_in * io->T * 4 < (1ll << 31) && (long long)rows_out * Tout * 4 < (1ll << 31),
               "vs_conv_forward: one item's tensor exceeds the 2 GiB buffer-descriptor range");
    if (h->kind == VS_CONV1D_PAIRED) {
        VS_REQUIRE(io->pair_mode >= VS_PAIR_GATE && io->pair_mode <= VS_PAIR_COUPLING_INV, "bad pair_mode");
        if (io->pair_mode != VS_PAIR_GATE) {
            VS_REQUIRE(io->out[0].res, "vs_conv_forward: coupling pair mode needs out[0].res (x1)");
            need_out_mask = true;
        }
    }
    need_mask |= need_out_mask;
    VS_REQUIRE(!need_mask || io->mask, "vs_conv_forward: mask required but NULL");
    // (an INPUT mask -- VS_IN_MASK / VS_IN_LRELU_MASK, indexed by input frame while staging -- is fine with any kind)
    VS_REQUIRE(Tout == io->T || !need_out_mask, "vs_conv_forward: an output mask needs T_out == T (not with a transposed / unpadded conv)");
    return VS_OK;
}

// VS_TRACE (debug): one line per launch on stderr, before any route is taken
static void trace_launch(const vs_conv *h, const ConvParams &p) {
    fprintf(stderr, "[vs_conv_forward] kind %d %d->%d k%d d%d pad%d flags%u B%d T%d Tout%d in_act%d split%d mode%d,%d res%d acc%d "
                    "mask%d bias_b%d pair%d x%p y%p y1%p\n", h->kind, h->c_in, h->c_out, h->k, h->dil, h->pad, h->flags, p.B, p.Tin,
            p.Tout, p.in_act, p.split_row, p.out[0].mode, p.out[1].mode, p.out[0].res != nullptr, p.out[0].acc != nullptr,
            p.mask != nullptr, p.bias_b != nullptr, p.pair_mode, (const void *)p.x, (void *)p.out[0].y, (void *)p.out[1].y);
}

// 2., 3. the VALU conv and the single-frame conv: small_conv_applies / t1_conv_applies and their launchers (conv_small.hip)

// 4. VS_CONV1D_PAIRED, with the log-det partials and their reduce (fast_epi stays 0 here: the paired epilogues do not take it)
static int forward_paired(vs_conv *h, ConvParams &p, hipStream_t s) {
    const bool want_ld = (p.pair_mode == VS_PAIR_COUPLING_FWD) && p.logdet;
    if (want_ld) {
        // log-det = sum of logs over (channel, frame): every wave leaves the sum of its tile in its own slot, then one workgroup per item
        // adds the slots in index order onto logdet[b] -- the same bits every run (an atomicAdd per tile summed in retirement order)
        p.ld_nt = (int)ceil_div(p.N, 32) + 64;                      // (+64: first-tile indices of the trailing waves of the widest tile shape)
        p.ld_slots = p.ld_nt * (int)ceil_div(h->MT, 2);
        VS_TRY(h->ldpart.reserve((size_t)p.B * p.ld_slots * sizeof(float)));
        p.ld_part = h->ldpart.as<float>();
        VS_CHECK_HIP(hipMemsetAsync(p.ld_part, 0, (size_t)p.B * p.ld_slots * sizeof(float), s));
    }
    int rc;
    if (h->math) {
        p.wp = h->ws.as<float>();
        p.wscale = h->wsc.as<float>();
        if (!opt(OPT_NO_KTAP) && p.Cin % CK == 0 && ktap_pair_instance(h->math, h->KT, io_bits(p), p.in_act, h->MT))
            rc = launch_ktap_pair(p, h->math, s);      // (conv_ktap_pair.hip: taps unrolled, staging in the MFMA shadows; bit-identical)
        else
            rc = launch_split(p, (h->MT >= 4) ? 4 : 5, h->math, h->span, s);
    } else if (h->MT >= 4) {
        p.W = 128 + h->span;
        rc = launch_cfg<2, 2, 2, 2>(p, s);
    } else {
        p.W = 256 + h->span;
        rc = launch_cfg<2, 2, 1, 4>(p, s);
    }
    if (rc == VS_OK && want_ld) {
        hipLaunchKernelGGL(logdet_reduce_kernel, dim3((unsigned)p.B), dim3(64), 0, s, p.ld_part, p.ld_slots, p.logdet);
        VS_CHECK_HIP(hipGetLastError());
    }
    return rc;
}

// 5. host-checked preconditions of the LDS-transposed float4 epilogue
static int fast_epi_ok(const vs_conv *h, const ConvParams &p) {
    bool ok = (h->kind == VS_CONV1D) && (p.Tout % 4 == 0) && !opt(OPT_NO_FAST_EPI);
    for (int s2 = 0; s2 < (p.split_row ? 2 : 1) && ok; ++s2) {
        const OutSpec &d = p.out[s2];
        ok = ok && d.mode == VS_OUT_LINEAR && al16(d.y) && (d.y_bs % 4 == 0) && (!d.res || (al16(d.res) && d.res_bs % 4 == 0)) &&
             (!d.acc || (al16(d.acc) && d.acc_bs % 4 == 0));
    }
    ok = ok && (!p.mask || al16(p.mask)) && (!p.split_row || p.split_row % 32 == 0);
    return ok ? 1 : 0;
}

// 6. F(2,3) path where it measured faster than the direct engine (tools/conv_bench.py, B=32 production shapes): with an even
// number of 32-row tiles every dilation-1 conv (k=3: +10..17 %, k=7: +0..2 %, k=9: +36..44 %, k=11: +21..25 %) and the
// k >= 9 convs at any dilation (+7..16 %); with an odd tile count (C_out = 32: the 32 x 512 workgroup shape, 2-slot
// fragment ring) only k >= 9 at dilation 1 (+10 %).  The dilated k=3 / k=7 convs lose 2..25 % (idle pair columns, 8-byte
// epilogue runs, fewer MFMAs to hide the same staging behind) and stay on the direct engine.
// VS_WINO_FORCE=1 / VS_NO_WINO=1: test / A-B switches.
// k = 7 through the straight-line instances (direct-form last tap, 10/14 of the direct MFMAs): +11..22 % at every dilation;
// k = 11 likewise with an F(2,2) last group (15/22): another 6 %.
static bool wino_applies(const vs_conv *h, const ConvParams &p) {
    const bool wino_pays = (h->MT & 1) ? (h->k >= 9 && h->dil == 1) : (h->dil == 1 || h->k >= 9 || h->wino_k7);
    return !h->math && h->wino_groups && (wino_pays || opt(OPT_WINO_FORCE)) && !p.split_row && p.out[0].mode == VS_OUT_LINEAR && !opt(OPT_NO_WINO);
}

// 7. the tile shape of the direct engine -- 0: <1,8,4,1> 128x256   1: <1,8,2,2> 64x512   2: <1,4,1,4> 32x512   3: <1,4,2,2> 64x256   6: 32x128 (split
// engines only) -- a function of the handle, the filled parameters and the options alone
static int choose_cfg(const vs_conv *h, const ConvParams &p) {
    // 128-row blocks unless that would leave a half-empty M block (6 tiles = 192 rows: the q/k/v/o, FFN-out,
    // coupling `pre` and last res/skip convs) AND the launch is short (T_mel-sized): there 64 x 256 blocks waste no MFMA
    // rows and give 1.5x the workgroups (a 256-workgroup launch fills only one slot per CU)
    // (6 tiles on a LONG launch -- the stride-3 stage of the hop-300 generator, 192 virtual rows: 64 x 512 blocks, three in M)
    int cfg;
    if (h->MT >= 3) cfg = ((h->MT % 4) == 2) ? (((long long)p.N * p.B <= 65536) ? 3 : 1) : 0;
    else cfg = (h->MT == 2) ? 1 : 2;
    const bool bf16_io = p.x_bf16 || p.y_bf16;
    // Short launches (single utterances, T_mel-sized tensors): a 128 x 256 tile grid of fewer workgroups than CUs leaves most of
    // the chip idle while each workgroup runs its full K loop -- the launch lasts as long as ONE workgroup.  On the bf16-pipe
    // engine take 64-row (then 32-row) tiles until the grid covers the CUs: the same kernel family, 2x / 4x the workgroups, each
    // with half / a quarter of the MFMAs per wave (B=1, T_mel=1024 synthesis latency: DESIGN.md 4.2).
    if (h->math && !opt(OPT_NO_SMALL_GRID) && !bf16_io) {      // (bf16-resident tensors: the 128-row instance only)
        const long long ncol = ceil_div(p.N, 256) * p.B;
        if (cfg == 0 && ncol * ceil_div(h->MT, 4) < 256) cfg = 3;
        if (cfg == 3 && ncol * ceil_div(h->MT, 2) < 256 && (long long)p.N * p.B <= 65536) cfg = 2;
        if (cfg == 2 && ncol * h->MT < opt(OPT_SMALL_GRID_T6) && h->kind != VS_CONV_TRANSPOSE1D) cfg = 6;     // 128-column tiles: twice the workgroups again
    }
    const long long forced = opt(OPT_CONV_CFG);      // A/B switch (tools/ktap_tile_sweep.py for 2 and 6)
    if (forced >= 0 && h->MT >= 3) cfg = (forced == 3) ? 3 : (forced == 1 ? 1 : 0);
    if ((forced == 2 || forced == 6) && !bf16_io && h->kind != VS_CONV_TRANSPOSE1D) cfg = (int)forced;
    // (plain bf16 behind a MASKED input transform: a launch whose chosen tile shape has no conv_ktap instance takes another shape that has one before it falls back to
    //  the tile kernel -- round 5 did this for safety, the tile kernel's masked instances gave wrong lanes then; round 6 root-caused and fixed that, DESIGN.md 4.5,
    //  tests/test_conv_mask_race_gpu.py, and the preference stays because the conv_ktap instances are faster)
    if (h->math == VS_MATH_BF16 && p.in_act >= VS_IN_MASK && h->kind == VS_CONV1D && !opt(OPT_NO_KTAP) && p.Cin % CK == 0 && !bf16_io &&
        !ktap_instance(h->math, cfg, h->KT, 0, p.in_act)) {
        for (int alt : {3, 6, 0})
            if (ktap_instance(h->math, alt, h->KT, 0, p.in_act)) { cfg = alt; break; }
    }
    return cfg;
}

// 8. the conv_ktap routes.  The wide stride-1 convs of the split-f16 arithmetic (generator resblocks at 128 / 256 channels, conv_pre, FFN conv_1): taps unrolled, the
// staging of the next chunk dealt out over the MFMA gaps of the current one (conv_ktap.inc; bit-identical to the tile kernels, VS_NO_KTAP=1: A/B); likewise the
// plain-bf16 arithmetic (BASELINE configs[4]: the hidden-512 transformer convs on fp32 tensors, the generator's wide convs on bf16-resident tensors)
// ... and the 64 x 256 / 32 x 128 tiles of short launches (T_mel-sized tensors, the training step): conv_ktap_small.hip
static bool ktap_applies(const vs_conv *h, const ConvParams &p, int cfg) {
    return (h->math == VS_MATH_SPLIT3 || h->math == VS_MATH_BF16) && h->kind == VS_CONV1D && !opt(OPT_NO_KTAP) && p.Cin % CK == 0 &&
           ktap_instance(h->math, cfg, h->KT, io_bits(p), p.in_act) && !(p.split_row && (p.split_row % 32) != 0);
}
// the generator's upsamplers (k = 2 * stride): conv_ktap.inc, IO bit 2
static bool ktap_tr_applies(const vs_conv *h, const ConvParams &p, int cfg) {
    return h->kind == VS_CONV_TRANSPOSE1D && !opt(OPT_NO_KTAP) && !opt(OPT_NO_TR_EPI) && ktap_tr_instance(p, h->math, cfg);
}

// 9. the tile kernels of the handle's engine in shape cfg
static int launch_tiles(const vs_conv *h, const ConvParams &q, int cfg, hipStream_t s) {
    if (h->math) return launch_split(q, cfg, h->math, h->span, s);
    switch (cfg) {
        case 0: return launch_cfg<1, 8, 4, 1>(q, s);
        case 1: return launch_cfg<1, 8, 2, 2>(q, s);
        case 3: return launch_cfg<1, 4, 2, 2>(q, s);
        default: return launch_cfg<1, 4, 1, 4>(q, s);
    }
}
static int forward_tiles(const vs_conv *h, ConvParams &p, int cfg, hipStream_t s) {
    p.W = ((cfg == 0 || cfg == 3) ? 256 : 512) + h->span;
    if (!(p.split_row && (p.split_row % 32) != 0)) return launch_tiles(h, p, cfg, s);
    // a 32-row tile would straddle the two destinations: store them in two passes (odd sizes only; the
    // production split is hidden_channels = 192 = 6 tiles)
    ConvParams q = p;
    q.fast_epi = 0;
    q.split_row = 0;
    q.row_hi = p.split_row;
    VS_TRY(launch_tiles(h, q, cfg, s));
    q.out[0] = p.out[1];
    q.row_lo = p.split_row;
    q.row_hi = h->c_out;
    // rows are addressed relative to split_row in the second destination
    q.out[0].rows = h->c_out;
    q.out[0].y -= (long long)p.split_row * p.Tout;
    if (q.out[0].res) q.out[0].res -= (long long)p.split_row * p.Tout;
    if (q.out[0].acc) q.out[0].acc -= (long long)p.split_row * p.Tout;
    return launch_tiles(h, q, cfg, s);
}

extern "C" {

const char *vs_last_error(void) { return g_err; }
const char *vs_last_kernel_name(void) { return g_last_kernel; }
int vs_abi_version(void) { return 7; }

int vs_set_option(const char *name, long long value) {
    VS_REQUIRE(name, "vs_set_option: NULL name");
    OptEntry *e = find_opt("vs_set_option", name);
    if (!e) return VS_EINVAL;
    e->value = value;
    return VS_OK;
}
int vs_get_option(const char *name, long long *value) {
    VS_REQUIRE(name && value, "vs_get_option: NULL argument");
    const OptEntry *e = find_opt("vs_get_option", name);
    if (!e) return VS_EINVAL;
    *value = e->value;
    return VS_OK;
}
int vs_reset_option(const char *name) {          /* back to the built-in default (not to the environment's value) */
    VS_REQUIRE(name, "vs_reset_option: NULL name");
    OptEntry *e = find_opt("vs_reset_option", name);
    if (!e) return VS_EINVAL;
    e->value = e->dflt;
    return VS_OK;
}

int vs_device_info(char *buf, size_t n) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) cnt = 0;
    if (buf && n) {
        buf[0] = 0;
        if (cnt > 0) {
            hipDeviceProp_t pr;
            if (hipGetDeviceProperties(&pr, 0) == hipSuccess) snprintf(buf, n, "%s (%s)", pr.name, pr.gcnArchName);
        }
    }
    return cnt;
}

// Debug only (not part of the public header): per-workgroup phase stamps of the next conv launches are written
// to buf[64 * n_workgroups] (s_memrealtime, 100 MHz): [0] start, [1] first chunk staged, [2] main loop done, [3] epilogue
// issued, [7] HW ids.  NULL disables.
__attribute__((visibility("default"))) void vs_debug_set_stamp_buffer(void *buf) { g_stamp_buf = (unsigned long long *)buf; }

int vs_conv_create(vs_conv_t **out, int kind, int c_in, int c_out, int k, int dil, int pad, unsigned flags) {
    VS_REQUIRE(out, "vs_conv_create: out is NULL");
    *out = nullptr;
    VS_REQUIRE(kind >= VS_CONV1D && kind <= VS_CONV1D_PAIRED, "vs_conv_create: unknown kind %d", kind);
    VS_REQUIRE(c_in > 0 && c_out > 0 && k > 0 && dil > 0 && pad >= 0, "vs_conv_create: bad dims");
    VS_REQUIRE(kind != VS_CONV1D_PAIRED || (c_out % 2 == 0), "vs_conv_create: PAIRED needs even c_out");
    VS_REQUIRE((flags & ~(VS_CONV_FLIP_IN | VS_CONV_FLIP_OUT | VS_CONV_ADJOINT)) == 0, "vs_conv_create: unknown flags %u", flags);
    VS_REQUIRE(!(flags & VS_CONV_ADJOINT) || (kind == VS_CONV1D && !(flags & (VS_CONV_FLIP_IN | VS_CONV_FLIP_OUT))),
               "vs_conv_create: VS_CONV_ADJOINT goes with a plain VS_CONV1D");
    vs_conv *h = new (std::nothrow) vs_conv();
    if (!h) { set_error("out of host memory"); return VS_ENOMEM; }
    h->kind = kind; h->c_in = c_in; h->c_out = c_out; h->k = k; h->dil = dil; h->pad = pad; h->flags = flags;
    h->Hh = c_out / 2;
    if (kind == VS_CONV_TRANSPOSE1D) {
        const int u = dil;
        h->M = u * c_out;
        h->dmin = ceil_div_i(-(u - 1) - pad, u);
        const int dmax = floor_div(k - 1 - pad, u);
        h->KT = dmax - h->dmin + 1;
        h->off0 = -h->dmin;      // x index = q - delta = q - dmin - tap
        h->tstep = -1;
    } else {
        h->M = (kind == VS_CONV1D_PAIRED) ? 2 * 32 * (int)ceil_div(h->Hh, 32) : c_out;
        h->KT = k;
        h->off0 = -pad;
        h->tstep = dil;
        h->dmin = 0;
    }
    const int off_last = h->off0 + (h->KT - 1) * h->tstep;
    h->lo = std::min(h->off0, off_last);
    h->span = std::max(h->off0, off_last) - h->lo;
    if (h->span > MAX_SPAN) {
        set_error("vs_conv_create: receptive span %d exceeds the LDS window (%d)", h->span, MAX_SPAN);
        delete h;
        return VS_EUNSUPPORTED;
    }
    h->MT = (int)ceil_div(h->M, 32);
    h->MT_alloc = (int)ceil_div(h->MT, MT_ALLOC) * MT_ALLOC;
    h->nchunks = (int)ceil_div(c_in, CK);
    h->CP = h->nchunks * (CK / 2);
    // F(2,3) minimal-filtering path: stride-1 "same" convs with >= 3 taps, dilation 1/3/5, whole 32-row tiles
    if (kind == VS_CONV1D && k >= 3 && (k & 1) && (dil == 1 || dil == 3 || dil == 5) && pad == dil * (k - 1) / 2 &&
        c_out % 32 == 0 && 3 * (int)ceil_div(k, 3) * dil <= MAX_SPAN)
        h->wino_groups = (int)ceil_div(k, 3);
    h->wino_k7 = h->wino_groups == 3 && k == 7 && (h->MT % 2 == 0) && !opt(OPT_NO_WINO_K7);
    h->wino_k11 = h->wino_groups == 4 && k == 11 && ((h->MT & 1) == 0 || dil == 1) && !opt(OPT_NO_WINO_K7);
    // Default arithmetic: the split-f16 x3 engine (two f16 planes under a power-of-two scale per staged tile, three cross products) --
    // measured x1.3 .. x1.45 the rate of the split-bf16 x6 engine on the 128- / 256-channel convs (tools/conv_bench.py) and CLOSER to the
    // fp64 result than it and than the fp32 MFMA on every case of tools/split3_check.py / tools/conv_accuracy.py (half the products summed
    // in fp32).  VS_CONV_MATH=0 / 1 / 3 / 6: process-wide A/B switch for handles created from here on.
    h->math = VS_MATH_SPLIT3;
    {
        const int m = (int)opt(OPT_CONV_MATH);
        if (m == VS_MATH_F32 || m == VS_MATH_BF16 || m == VS_MATH_SPLIT6 || m == VS_MATH_SPLIT3) h->math = m;
    }
    *out = h;
    return VS_OK;
}

void vs_conv_destroy(vs_conv_t *h) { delete h; }

int64_t vs_conv_out_len(const vs_conv_t *h, int64_t T) {
    if (!h) return -1;
    if (h->kind == VS_CONV_TRANSPOSE1D) return (T - 1) * h->dil - 2 * h->pad + h->k;
    return T + 2 * h->pad - (int64_t)h->dil * (h->k - 1);
}

int vs_conv_forward(vs_conv_t *h, const vs_conv_io_t *io, void *stream) {
    ConvParams p;
    VS_TRY(fill_params(h, io, p));
    hipStream_t s = as_stream(stream);
    VS_TRY(order_read(h, s));
    if (opt(OPT_TRACE)) trace_launch(h, p);
    if (small_conv_applies(h, p)) return launch_small_conv(h, p, s);
    if (t1_conv_applies(h, p)) return launch_t1_conv(h, p, s);
    if (h->kind == VS_CONV1D_PAIRED) return forward_paired(h, p, s);
    p.fast_epi = fast_epi_ok(h, p);
    if (wino_applies(h, p)) {
        VS_TRY(pack_wino_weights(h, s));
        return launch_wino_conv(h, p, s);
    }
    const int cfg = choose_cfg(h, p);
    if (h->math) {       // the split engines read the plane fragments Ws in place of Wp
        p.wp = h->ws.as<float>();
        p.dbg = (int)opt(OPT_SPLIT_DBG);
    }
    p.wscale = h->wsc.as<float>();
    if (ktap_applies(h, p, cfg)) return h->math == VS_MATH_SPLIT3 ? launch_ktap(p, cfg, s) : launch_ktap_bf16(p, cfg, s);
    if (ktap_tr_applies(h, p, cfg)) return launch_ktap_tr(p, s);
    return forward_tiles(h, p, cfg, s);
}

}  // extern "C"
