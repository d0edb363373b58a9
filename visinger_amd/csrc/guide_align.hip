// guide_align.hip -- the score timed to a recording: which frames of a guide f0 curve belong to which token of the score (include/visinger_hip.h "f7",
// DESIGN.md 4.12).  Not in the reference (its inference replays the score's own timing; alignment is an offline host tool there).  A monotonic Viterbi
// alignment in integers, ONE workgroup per item, one launch for the batch:
//   prologue   tokens with dur > 0 compacted to columns 0 .. S-1 by a workgroup scan (their count, a_s and L come out of the same scan); thread s owns column s.
//   forward    sequential over the G frames, parallel over the columns.  D(t-1, s) lives in a register; D(t-1, s-1) comes from the lane below by a DPP
//              wave shift, across a wave boundary through a double-buffered LDS slot -- one workgroup barrier a frame, none when S <= 64 (one wave runs alone).
//              (the local cost is branch-free across the lanes, its drift term in 32 bits when L < 2^31.)  q_t and u_t are staged into LDS 256 frames at a time, a chunk ahead, so the barrier of the frames publishes them.  The backpointers are one bit
//              per (t, s): a wave's ballot is the packed word; in LDS when G ceil(S / 64) words fit, else in the caller's workspace by plain vector stores.
//   backtrack  wave 0, 64 rows at a time: lane l fetches row t0 - l of the current word column and of its left neighbour, the chain is resolved on
//              read-lane values (s moves by at most one a frame, so two columns cover a block).
//   runs       flags, three scans and a prefix max: E_i - i = max(0, max_{j <= i}(R_j - j)) inside a run.
// Everything after the two quantisations is integer: bit-reproducible, and a row's result depends on that row only.  No atomics, no host synchronisation.
#include "vs_internal.h"
#include "pitch_quant.h"                                // ga_quant, GA_NONE: the frame quantiser, shared with pitch_path.hip

#include <climits>
#include <cmath>

namespace vs {

constexpr int GA_MAX_TOKENS = 1024;                     // columns = threads of the largest workgroup
constexpr int GA_MAX_FRAMES = 65536;
constexpr int GA_CHUNK = 256;                           // frames staged at a time
constexpr int GA_LDS_WORDS = VS_GUIDE_ALIGN_LDS_WORDS;  // backpointer words kept in LDS (40 KiB of the 64)
constexpr int GA_INF = (1 << 30) - 1;
constexpr long long GA_MAX_DUR = (1ll << 24) - 1;
constexpr int GA_WEIGHT_MAX = 4096;

struct GaWeights {
    int cap, w_voiced_rest, w_unvoiced_note, drift, drift_cap, octave_fold;
};

struct GaStage {                                        // the forward pass: q_t, u_t of two chunks
    long long u[2][GA_CHUNK];
    int q[2][GA_CHUNK];
};
struct GaRuns {                                         // the run pass: m + off by column, then the inclusive sums of n; the last column of the run that starts at [s]
    int pn[GA_MAX_TOKENS];
    int run_end[GA_MAX_TOKENS];
};
struct GaShared {
    unsigned long long bp[GA_LDS_WORDS];
    long long pd[GA_MAX_TOKENS];                        // a_s by column (prologue), then the inclusive sums of d over the columns (run pass)
    int start[GA_MAX_TOKENS + 2];                       // first frame of each column (backtrack), then E (run pass)
    union {
        GaStage st;
        GaRuns rp;
    } x;
    unsigned short idx[GA_MAX_TOKENS];                  // column -> token
    long long wave_tot[16][2];
    long long total[2];                                 // S, L
    int slot[2][16];                                    // D(t, last column of wave w), double-buffered by t & 1
};
static_assert(sizeof(GaShared) <= 65536, "the workgroup's LDS");

// inclusive sums over the threads <= this one of the workgroup, two at a time
__device__ __forceinline__ void ga_scan_add2(long long &a, long long &b, long long (*wave_tot)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long oa = __shfl_up(a, d), ob = __shfl_up(b, d);
        if (lane >= d) {
            a += oa;
            b += ob;
        }
    }
    if (lane == 63) {
        wave_tot[w][0] = a;
        wave_tot[w][1] = b;
    }
    __syncthreads();
    for (int i = 0; i < w; ++i) {
        a += wave_tot[i][0];
        b += wave_tot[i][1];
    }
    __syncthreads();
}

// inclusive max over the threads <= this one of the workgroup
__device__ __forceinline__ long long ga_scan_max(long long v, long long (*wave_tot)[2]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(v, d);
        if (lane >= d) v = max(v, o);
    }
    if (lane == 63) wave_tot[w][0] = v;
    __syncthreads();
    for (int i = 0; i < w; ++i) v = max(v, wave_tot[i][0]);
    __syncthreads();
    return v;
}

__device__ __forceinline__ long long ga_dur(long long d) { return d < 0 ? 0 : (d > GA_MAX_DUR ? GA_MAX_DUR : d); }

// what a column brings to c(t, s): its pitch (0 on a rest, never read there), what an unvoiced frame costs on it, and its span [a, e] in the score
template <typename Pos>
struct GaColumn {
    int mo, pitched, unvoiced_cost;
    Pos a, e;
};

// c(t, s), branch-free across the lanes (voiced and the fold are uniform).  Pos is int when L < 2^31 -- a, e, u and their differences then fit -- else int64.
template <typename Pos>
__device__ __forceinline__ int ga_cost(int q, Pos u, const GaColumn<Pos> &col, const GaWeights &wt) {
    int pc = col.unvoiced_cost;
    if (q != GA_NONE) {
        int dl = abs(q - col.mo);
        if (wt.octave_fold) {
            dl %= 192;
            dl = min(dl, 192 - dl);
        }
        pc = col.pitched ? min(dl, wt.cap) : wt.w_voiced_rest;
    }
    const Pos gap = max(max(col.a - u, u - col.e), (Pos)0);
    // (gap drift) >> 8 reaches drift_cap <= 4096 at gap = 2^20 whatever drift >= 1 is, and drift = 0 gives 0 either way: 32 x 32 -> 64 bits is exact
    const unsigned long long p = ((unsigned long long)(unsigned)min(gap, (Pos)(1 << 20)) * (unsigned)wt.drift) >> 8;
    return pc + (int)min(p, (unsigned long long)wt.drift_cap);
}

// the forward pass of one item.  MULTI: every wave of the workgroup is here and meets at one barrier a frame; otherwise wave 0 alone, no barrier.
// Columns at or beyond S run along on a rest of span [0, -1]: nothing reads them (a lane reads the lane below only, the backtrack starts at S - 1).
// Returns D(G - 1, s) of this thread's column.
template <bool MULTI, typename Pos>
__device__ __forceinline__ int ga_forward(GaShared &sh, const float *__restrict__ f0, int G, int S, long long L, const GaColumn<Pos> &col,
                                          const GaWeights &wt, unsigned long long *__restrict__ bpg, bool use_lds, int stride) {
    const int s = threadIdx.x, lane = s & 63, w = s >> 6, nw = (S + 63) >> 6;
    const int nstage = MULTI ? (int)blockDim.x : 64;
    auto stage = [&](int c) {
        for (int j = s; j < GA_CHUNK; j += nstage) {
            const int t = c * GA_CHUNK + j;
            if (t < G) {
                sh.x.st.q[c & 1][j] = ga_quant(f0[t]);
                sh.x.st.u[c & 1][j] = ((long long)t * L) / G;                 // the floor division itself, once per frame
            }
        }
    };
    stage(0);
    int D = GA_INF;
    if (s == 0) D = min(GA_INF, ga_cost<Pos>(ga_quant(f0[0]), (Pos)0, col, wt));
    if (MULTI) {
        if (lane == 63) sh.slot[0][w] = D;
        __syncthreads();                                                      // publishes chunk 0 and D(0, .)
    }
    int qn = GA_NONE;
    Pos un = 0;
    if (G > 1) {
        qn = sh.x.st.q[0][1];
        un = (Pos)sh.x.st.u[0][1];
    }
    for (int c = 0; c * GA_CHUNK < G; ++c) {
        // the next chunk goes into the buffer whose last reader passed the barrier of the previous chunk's last frame; the barriers of this chunk's frames
        // publish it (wave 0 alone: LDS operations of one wave complete in order)
        if ((c + 1) * GA_CHUNK < G) stage(c + 1);
        const int t_end = min(G, (c + 1) * GA_CHUNK);
        for (int t = max(1, c * GA_CHUNK); t < t_end; ++t) {
            const int q = qn;
            const Pos u = un;
            if (t + 1 < G) {                                                  // the next frame's pair, fetched under this frame's arithmetic
                qn = sh.x.st.q[((t + 1) / GA_CHUNK) & 1][(t + 1) % GA_CHUNK];
                un = (Pos)sh.x.st.u[((t + 1) / GA_CHUNK) & 1][(t + 1) % GA_CHUNK];
            }
            if (w < nw) {
                const int c_ts = ga_cost<Pos>(q, u, col, wt);                 // (does not wait for the exchange)
                int below = GA_INF;
                if (MULTI && w > 0) below = sh.slot[(t - 1) & 1][w - 1];
                // wave_shr:1 -- lane l reads lane l - 1; lane 0 has no source and keeps `below`.  Column 0 reads INF: INF < D never holds, so it never advances
                const int left = __builtin_amdgcn_update_dpp(below, D, 0x138, 0xf, 0xf, false);
                const bool adv = left < D;                                    // a tie stays
                const unsigned long long word = __ballot(adv);
                D = min(GA_INF, c_ts + (adv ? left : D));
                if (lane == 0) {
                    if (use_lds) sh.bp[t * stride + w] = word;
                    else bpg[(long long)t * stride + w] = word;
                }
                if (MULTI && lane == 63) sh.slot[t & 1][w] = D;
            }
            if (MULTI) __syncthreads();
        }
    }
    return D;
}

__global__ void __launch_bounds__(GA_MAX_TOKENS) guide_align_kernel(const float *__restrict__ f0_hz, const long long *__restrict__ g_len,
                                                                    const float *__restrict__ note_midi, const long long *__restrict__ dur,
                                                                    const float *__restrict__ offset_cents, GaWeights wt, long long *__restrict__ dur_new,
                                                                    int *__restrict__ cost, int *__restrict__ status, unsigned long long *__restrict__ work,
                                                                    long long B, int Tg, int T_ph) {
    __shared__ GaShared sh;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int words_row = (T_ph + 63) >> 6;
    for (long long row = blockIdx.x; row < B; row += gridDim.x) {
        // ---- prologue: thread i reads token i; the active tokens become columns
        const bool in = tid < T_ph;
        const long long d_raw = in ? dur[row * T_ph + tid] : 0;
        const long long d_tok = ga_dur(d_raw);
        long long cnt = d_tok > 0 ? 1 : 0, sum = d_tok;
        ga_scan_add2(cnt, sum, sh.wave_tot);
        if (d_tok > 0) {
            sh.idx[cnt - 1] = (unsigned short)tid;
            sh.pd[cnt - 1] = sum - d_tok;
        }
        if (tid == (int)blockDim.x - 1) {
            sh.total[0] = cnt;
            sh.total[1] = sum;
        }
        __syncthreads();
        const int S = (int)sh.total[0];
        const long long L = sh.total[1];
        long long g = g_len ? g_len[row] : (long long)Tg;
        const int G = (int)(g < 0 ? 0 : (g > Tg ? (long long)Tg : g));
        if (S == 0 || G < S) {
            if (in) dur_new[row * T_ph + tid] = d_raw < 0 ? 0 : d_raw;
            if (tid == 0) {
                cost[row] = -1;
                status[row] = 1;
            }
            __syncthreads();
            continue;
        }
        // thread s takes column s
        int tok = 0, mo = GA_NONE;
        long long a = 0, d_col = 0;
        if (tid < S) {
            tok = sh.idx[tid];
            a = sh.pd[tid];
            d_col = ga_dur(dur[row * T_ph + tok]);
            const float note = note_midi[row * T_ph + tok];
            if (note > 0.f && note < INFINITY) {
                float oc = offset_cents ? offset_cents[row] : 0.f;
                if (!(fabsf(oc) < INFINITY)) oc = 0.f;
                const int off = (int)rintf(fminf(fmaxf(oc * 0.16f, -1048576.f), 1048576.f));
                mo = (int)rintf(fminf(16.f * note, 1048576.f)) + off;
            }
        }
        const int nw = (S + 63) >> 6;
        const bool use_lds = (long long)G * nw <= GA_LDS_WORDS;
        const int stride = use_lds ? nw : words_row;
        unsigned long long *bpg = use_lds ? nullptr : work + row * Tg * words_row;
        const float *f0 = f0_hz + row * Tg;
        int D;
        if (L <= INT_MAX) {                                                   // the drift term in 32 bits
            const GaColumn<int> col = {mo == GA_NONE ? 0 : mo, mo != GA_NONE, mo == GA_NONE ? 0 : wt.w_unvoiced_note, (int)a, (int)(a + d_col - 1)};
            D = S > 64 ? ga_forward<true, int>(sh, f0, G, S, L, col, wt, bpg, use_lds, stride)
                       : (w == 0 ? ga_forward<false, int>(sh, f0, G, S, L, col, wt, bpg, use_lds, stride) : GA_INF);
        } else {
            const GaColumn<long long> col = {mo == GA_NONE ? 0 : mo, mo != GA_NONE, mo == GA_NONE ? 0 : wt.w_unvoiced_note, a, a + d_col - 1};
            D = S > 64 ? ga_forward<true, long long>(sh, f0, G, S, L, col, wt, bpg, use_lds, stride)
                       : (w == 0 ? ga_forward<false, long long>(sh, f0, G, S, L, col, wt, bpg, use_lds, stride) : GA_INF);
        }
        if (tid == S - 1) cost[row] = D;
        __threadfence_block();                                                // the backpointer words, LDS or workspace, to wave 0: the workgroup sits on one CU
        __syncthreads();

        // ---- backtrack: wave 0
        if (w == 0) {
            if (lane == 0) {
                sh.start[0] = 0;
                sh.start[S] = G;
            }
            int s = __builtin_amdgcn_readfirstlane(S - 1);
            for (int t0 = G - 1; t0 >= 1 && s > 0; t0 -= 64) {
                const int t = t0 - lane, c = s >> 6;
                unsigned long long wc = 0, wl = 0;                            // row t of word column c and of c - 1
                if (t >= 1) {
                    if (use_lds) {
                        wc = sh.bp[t * stride + c];
                        if (c > 0) wl = sh.bp[t * stride + c - 1];
                    } else {
                        wc = bpg[(long long)t * stride + c];
                        if (c > 0) wl = bpg[(long long)t * stride + c - 1];
                    }
                }
                const int wc_lo = (int)(unsigned)wc, wc_hi = (int)(unsigned)(wc >> 32), wl_lo = (int)(unsigned)wl, wl_hi = (int)(unsigned)(wl >> 32);
#pragma unroll
                for (int l = 0; l < 64; ++l) {                                // rows before frame 1 hold 0: no step
                    const bool cur = (s >> 6) == c;
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane(cur ? wc_lo : wl_lo, l);
                    const unsigned hi = (unsigned)__builtin_amdgcn_readlane(cur ? wc_hi : wl_hi, l);
                    const unsigned half = (s & 32) ? hi : lo;
                    if ((half >> (s & 31)) & 1u) {
                        if (lane == 0) sh.start[s] = t0 - l;
                        --s;
                    }
                }
            }
        }
        __syncthreads();

        // ---- runs: the frames of a run shared out again by the score's durations
        const bool act = tid < S;
        const long long n_col = act ? (long long)(sh.start[tid + 1] - sh.start[tid]) : 0;
        sh.x.rp.pn[tid] = act ? mo : 0;
        __syncthreads();
        const bool head = act && (tid == 0 || sh.x.rp.pn[tid - 1] != mo);
        const bool tail = act && (tid == S - 1 || sh.x.rp.pn[tid + 1] != mo);
        const int r0 = (int)ga_scan_max(head ? (long long)tid : -1ll, sh.wave_tot);       // the first column of this column's run
        long long pn = n_col, pd = act ? d_col : 0;
        ga_scan_add2(pn, pd, sh.wave_tot);
        if (act) {
            sh.x.rp.pn[tid] = (int)pn;
            sh.pd[tid] = pd;
        }
        if (tail) sh.x.rp.run_end[r0] = tid;
        __syncthreads();
        long long key = -1;
        int i = 0;
        if (act) {
            const int re = sh.x.rp.run_end[r0];
            const long long pn0 = r0 ? (long long)sh.x.rp.pn[r0 - 1] : 0, pd0 = r0 ? sh.pd[r0 - 1] : 0;
            const long long n = sh.x.rp.pn[re] - pn0, Dr = sh.pd[re] - pd0, C = pd - pd0;
            const int k = re - r0 + 1;
            i = tid - r0 + 1;
            const long long R = min((2 * C * n + Dr) / (2 * Dr), n - (k - i));
            key = ((long long)r0 << 32) + (R - i + 65536);                    // r0 never decreases along the columns: the prefix max stays inside the run
        }
        key = ga_scan_max(key, sh.wave_tot);
        const int E = i + max(0, (int)(key & 0xffffffffll) - 65536);
        if (act) sh.start[tid] = E;
        __syncthreads();
        if (act) dur_new[row * T_ph + tok] = E - (head ? 0 : sh.start[tid - 1]);
        if (in && d_tok == 0) dur_new[row * T_ph + tid] = 0;
        if (tid == 0) status[row] = 0;
        __syncthreads();
    }
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_guide_align(const float *f0_hz, const int64_t *g_len, const float *note_midi, const int64_t *dur, const float *offset_cents, int cap,
                   int w_voiced_rest, int w_unvoiced_note, int drift, int drift_cap, int octave_fold, int reserved, int64_t *dur_new, int32_t *cost,
                   int32_t *status, void *workspace, size_t workspace_bytes, int64_t B, int64_t Tg, int64_t T_ph, void *stream) {
    VS_REQUIRE(f0_hz && note_midi && dur && dur_new && cost && status, "vs_guide_align: f0_hz, note_midi, dur, dur_new, cost and status must not be NULL");
    VS_REQUIRE(dur_new != dur && dur_new != g_len && cost != status && (const void *)f0_hz != (const void *)note_midi,
               "vs_guide_align: the buffers must be distinct");
    VS_REQUIRE(B >= 1 && T_ph >= 1 && T_ph <= GA_MAX_TOKENS && Tg >= 1 && Tg <= GA_MAX_FRAMES,
               "vs_guide_align: B >= 1, 1 <= T_ph <= %d and 1 <= Tg <= %d are required (got %lld, %lld, %lld)", GA_MAX_TOKENS, GA_MAX_FRAMES, (long long)B,
               (long long)T_ph, (long long)Tg);
    const int ws[5] = {cap, w_voiced_rest, w_unvoiced_note, drift, drift_cap};
    for (int v : ws) VS_REQUIRE(v >= 0 && v <= GA_WEIGHT_MAX, "vs_guide_align: a weight of %d is not in [0, %d]", v, GA_WEIGHT_MAX);
    VS_REQUIRE(octave_fold == 0 || octave_fold == 1, "vs_guide_align: octave_fold = %d is not 0 or 1", octave_fold);
    VS_REQUIRE(reserved == 0, "vs_guide_align: the reserved argument must be 0 (got %d)", reserved);
    const int64_t words_row = ceil_div(T_ph, 64);
    if (Tg * words_row > GA_LDS_WORDS) {                                      // an item of this shape may not fit the LDS: the workspace must be there
        VS_REQUIRE(B <= INT64_MAX / (Tg * words_row * 8), "vs_guide_align: B = %lld is out of range", (long long)B);
        const size_t need = (size_t)(B * Tg * words_row * 8);
        VS_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0,
                   "vs_guide_align: Tg ceil(T_ph / 64) = %lld words exceed %d: an 8-byte aligned workspace of B Tg ceil(T_ph / 64) 8 = %zu bytes is needed (got %zu)",
                   (long long)(Tg * words_row), GA_LDS_WORDS, need, workspace ? workspace_bytes : (size_t)0);
    }
    const GaWeights wt = {cap, w_voiced_rest, w_unvoiced_note, drift, drift_cap, octave_fold};
    const unsigned threads = (unsigned)(ceil_div(T_ph, 64) * 64);
    hipLaunchKernelGGL(guide_align_kernel, dim3((unsigned)(B < 65535 ? B : 65535)), dim3(threads), 0, as_stream(stream), f0_hz, (const long long *)g_len,
                       note_midi, (const long long *)dur, offset_cents, wt, (long long *)dur_new, (int *)cost, (int *)status, (unsigned long long *)workspace,
                       (long long)B, (int)Tg, (int)T_ph);
    VS_CHECK_HIP(hipGetLastError());
    return VS_OK;
}

}  // extern "C"
