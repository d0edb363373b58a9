// Micro-benchmark: v_mfma_f32_16x16x32_bf16 against v_mfma_f32_32x32x16_bf16 under the conv engine's operand pattern (random bf16
// operands in registers, 128 accumulator registers per wave, six cross products per accumulator tile), whole chip, two workgroups
// per CU, with the DISTANCE between two MFMAs on the same accumulator as the parameter (DIST = 1: six back-to-back dependent MFMAs
// per tile as conv_split_kernel issues them; 2 / 4: tiles interleaved so that a tile's next MFMA is the 2nd / 4th after it).
// Reports TFLOP/s by wall clock and the shader clock the loop ran at (s_memtime / s_memrealtime).  Each arm counts its OWN FLOPs: per iteration the 32x32x16 arm
// issues 8 tiles x 6 = 48 MFMAs of 32768 FLOP, the 16x16x32 arm 32 tiles x 6 = 192 MFMAs of 16384 FLOP = 96 x 32768 (six K = 32 products per output against six
// K = 16 products: twice the work on the same outputs).
// The second half (kf) is the fused resblock's operand pattern on f16 (csrc/resblock_f16.hip): a 32-row x 128-column output tile per wave in 128 accumulator
// registers, per accumulator three cross products in the order lh, hl, hh, the B fragments of both planes re-read from an LDS tile
// [plane][group of 8 channels][column][8 f16] by ds_read_b128 (each feeds two 16-row tiles or one 32-row tile), the A fragments from global memory one step ahead.
// The 16x16x32 arm interleaves the four accumulators that share a pair of B fragments, so no MFMA follows one on the same accumulator.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/mfma_shape_rate.hip -o /tmp/mfma_shape_rate && /tmp/mfma_shape_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int SHAPE, int DIST>   // SHAPE 0: 32x32x16, 1: 16x16x32
__global__ void __launch_bounds__(256, 2) k(const u32x4 *in, float *out, unsigned long long *clk, int iters) {
    u32x4 a[6], b[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) a[i] = in[(threadIdx.x * 7 + i * 131 + blockIdx.x) & 4095];
#pragma unroll
    for (int i = 0; i < 3; ++i) b[i] = in[(threadIdx.x * 11 + i * 977 + 5 * blockIdx.x) & 4095];
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
    if constexpr (SHAPE == 0) {
        f32x16 acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int j0 = 0; j0 < 8; j0 += DIST)
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int j = j0; j < j0 + DIST; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t % 3]), __builtin_bit_cast(bf16x8, b[(t + j) % 3]), acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) s += acc[j][r];
    } else {
        f32x4 acc[32];     // the same 128 accumulator registers: 32 tiles of 16x16 = 2 row tiles x 16 column tiles
#pragma unroll
        for (int j = 0; j < 32; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int j0 = 0; j0 < 32; j0 += DIST)
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int j = j0; j < j0 + DIST; ++j)   // tile j: row tile j & 1 (its own A fragments), column tile j >> 1
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[(t % 3) + 3 * (j & 1)]), __builtin_bit_cast(bf16x8, b[(t + (j >> 1)) % 3]), acc[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 32; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) s += acc[j][r];
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) { clk[2 * blockIdx.x] = t1 - t0; clk[2 * blockIdx.x + 1] = r1 - r0; }
}

template <int SHAPE, int DIST>
static void run(const char *name, const u32x4 *in, float *out, unsigned long long *clk, int blocks, int iters) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int w = 0; w < 3; ++w) hipLaunchKernelGGL((k<SHAPE, DIST>), dim3(blocks), dim3(256), 0, 0, in, out, clk, iters);
    hipEventRecord(e0);
    const int reps = 10;
    for (int w = 0; w < reps; ++w) hipLaunchKernelGGL((k<SHAPE, DIST>), dim3(blocks), dim3(256), 0, 0, in, out, clk, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h(2 * blocks);
    hipMemcpy(h.data(), clk, sizeof(unsigned long long) * 2 * blocks, hipMemcpyDeviceToHost);
    double cyc = 0, rt = 0;
    for (int i = 0; i < blocks; ++i) { cyc += h[2 * i]; rt += h[2 * i + 1]; }
    const double units = SHAPE == 0 ? 48.0 : 96.0;      // 32768-FLOP units per iteration and wave: 48 MFMAs of 32x32x16, 192 of 16x16x32 (16384 FLOP each)
    const double flop = (double)reps * blocks * 4 /*waves*/ * iters * units * 32768.0;
    printf("bf16 regs %-9s dist %d  %8.1f TFLOP/s   shader clock %.3f GHz   %.2f cycles per 32768 FLOP per wave\n", name, DIST,
           flop / (ms * 1e-3) / 1e12, cyc / rt * 0.1, cyc / blocks / ((double)iters * units));
}

// ---- the fused resblock's pattern: f16 planes, B from LDS, A from global memory one step ahead
constexpr int F_KG = 8, F_WT = 128 + 8, F_TPL = F_KG * F_WT * 4;      // 64 channels x (128 columns + a margin for the taps); dwords per plane

template <int SHAPE>   // 0: 32x32x16 (twelve K = 16 steps per iteration), 1: 16x16x32 (six K = 32 steps): 144 x 32768 FLOP per iteration and wave either way
__global__ void __launch_bounds__(256, 2) kf(const u32x4 *in, float *out, unsigned long long *clk, int iters) {
    __shared__ __attribute__((aligned(16))) unsigned Tb[2 * F_TPL];
    const int lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < 2 * F_KG * F_WT; e += 256) *reinterpret_cast<u32x4 *>(Tb + e * 4) = in[(e * 13 + blockIdx.x * 7) & 4095];
    __syncthreads();
    const u32x4 *const ab = in + lane;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    float s = 0.f;
    if constexpr (SHAPE == 0) {
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        const unsigned *const xl = Tb + ((lane >> 5) * F_WT + (lane & 31)) * 4;
        u32x4 a[2][2];      // [buffer][plane]: lane = row + 32 * (K group of 8)
        a[0][0] = ab[0]; a[0][1] = ab[64];
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int st = 0; st < 12; ++st) {
                const int chunk = st / 3, tap = st % 3, cur = st & 1;
                const int nx = ((it * 12 + st + 1) * 128) & 4095;
                a[cur ^ 1][0] = ab[nx]; a[cur ^ 1][1] = ab[nx + 64];
                const unsigned *const xs = xl + (2 * chunk * F_WT + tap) * 4;
                u32x4 bf[2], bn[2];
                bf[0] = *reinterpret_cast<const u32x4 *>(xs); bf[1] = *reinterpret_cast<const u32x4 *>(xs + F_TPL);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j + 1 < 4) { bn[0] = *reinterpret_cast<const u32x4 *>(xs + (j + 1) * 128); bn[1] = *reinterpret_cast<const u32x4 *>(xs + F_TPL + (j + 1) * 128); }
                    __builtin_amdgcn_sched_barrier(0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[cur][1]), __builtin_bit_cast(f16x8, bf[0]), acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[cur][0]), __builtin_bit_cast(f16x8, bf[1]), acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[cur][0]), __builtin_bit_cast(f16x8, bf[0]), acc[j], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    bf[0] = bn[0]; bf[1] = bn[1];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) s += acc[j][r];
    } else {
        f32x4 acc[2][8];    // [16-row tile][16-column tile]
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[rt][j][r] = 0.f;
        const unsigned *const xl = Tb + ((lane >> 4) * F_WT + (lane & 15)) * 4;
        u32x4 a[2][2][2];   // [buffer][row tile][plane]: lane = row + 16 * (K group of 8)
#pragma unroll
        for (int q = 0; q < 4; ++q) a[0][q >> 1][q & 1] = ab[64 * q];
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int st = 0; st < 6; ++st) {
                const int chunk = st / 3, tap = st % 3, cur = st & 1;
                const int nx = ((it * 6 + st + 1) * 256) & 4095;
#pragma unroll
                for (int q = 0; q < 4; ++q) a[cur ^ 1][q >> 1][q & 1] = ab[nx + 64 * q];
                const unsigned *const xs = xl + (4 * chunk * F_WT + tap) * 4;
                u32x4 bf[2][2], bn[2][2];   // [column tile of the pair][plane]
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) bf[ct][pl] = *reinterpret_cast<const u32x4 *>(xs + pl * F_TPL + ct * 64);
#pragma unroll
                for (int jp = 0; jp < 4; ++jp) {
                    if (jp + 1 < 4) {
#pragma unroll
                        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                            for (int pl = 0; pl < 2; ++pl) bn[ct][pl] = *reinterpret_cast<const u32x4 *>(xs + pl * F_TPL + (jp + 1) * 128 + ct * 64);
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < 3; ++t)       // lh, hl, hh: each product on the four accumulators in turn
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int rt = q & 1, ct = q >> 1;
                            acc[rt][2 * jp + ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a[cur][rt][t == 0 ? 1 : 0]),
                                                                                         __builtin_bit_cast(f16x8, bf[ct][t == 1 ? 1 : 0]), acc[rt][2 * jp + ct], 0, 0, 0);
                        }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) { bf[ct][0] = bn[ct][0]; bf[ct][1] = bn[ct][1]; }
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) s += acc[rt][j][r];
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (threadIdx.x == 0) { clk[2 * blockIdx.x] = t1 - t0; clk[2 * blockIdx.x + 1] = r1 - r0; }
}

template <int SHAPE>
static void runf(const char *name, const u32x4 *in, float *out, unsigned long long *clk, int blocks, int iters) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int w = 0; w < 3; ++w) hipLaunchKernelGGL((kf<SHAPE>), dim3(blocks), dim3(256), 0, 0, in, out, clk, iters);
    hipEventRecord(e0);
    const int reps = 10;
    for (int w = 0; w < reps; ++w) hipLaunchKernelGGL((kf<SHAPE>), dim3(blocks), dim3(256), 0, 0, in, out, clk, iters);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h(2 * blocks);
    hipMemcpy(h.data(), clk, sizeof(unsigned long long) * 2 * blocks, hipMemcpyDeviceToHost);
    double cyc = 0, rt = 0;
    for (int i = 0; i < blocks; ++i) { cyc += h[2 * i]; rt += h[2 * i + 1]; }
    const double flop = (double)reps * blocks * 4 /*waves*/ * iters * 144.0 * 32768.0;
    printf("f16 LDS-fed %-9s  %8.1f TFLOP/s   shader clock %.3f GHz   %.2f cycles per 32768 FLOP per wave   (%.3f ms per launch)\n", name,
           flop / (ms * 1e-3) / 1e12, cyc / rt * 0.1, cyc / blocks / ((double)iters * 144.0), ms / reps);
}

int main() {
    const int blocks = 512 * 8, iters = 400;
    std::vector<unsigned> hin(4096 * 4);
    srand(1);
    for (auto &v : hin) {       // random finite bf16 pairs
        unsigned lo = (rand() & 0x807f) | (((rand() % 16) + 120) << 7), hi = (rand() & 0x807f) | (((rand() % 16) + 120) << 7);
        v = lo | (hi << 16);
    }
    std::vector<unsigned> hf(4096 * 4);
    for (auto &v : hf) {        // random finite f16 pairs: any sign and mantissa, exponents 2^-8 .. 2^-1
        unsigned lo = (rand() & 0x83ff) | (((rand() % 8) + 7) << 10), hi = (rand() & 0x83ff) | (((rand() % 8) + 7) << 10);
        v = lo | (hi << 16);
    }
    u32x4 *in; float *out; unsigned long long *clk;
    hipMalloc(&in, hin.size() * 4); hipMalloc(&out, (size_t)blocks * 256 * 4); hipMalloc(&clk, (size_t)blocks * 16);
    hipMemcpy(in, hin.data(), hin.size() * 4, hipMemcpyHostToDevice);
    u32x4 *inf;
    hipMalloc(&inf, hf.size() * 4);
    hipMemcpy(inf, hf.data(), hf.size() * 4, hipMemcpyHostToDevice);
    for (int rep = 0; rep < 2; ++rep) {
        run<0, 1>("32x32x16", in, out, clk, blocks, iters);
        run<0, 2>("32x32x16", in, out, clk, blocks, iters);
        run<1, 1>("16x16x32", in, out, clk, blocks, iters);
        run<1, 2>("16x16x32", in, out, clk, blocks, iters);
        run<1, 4>("16x16x32", in, out, clk, blocks, iters);
        run<1, 8>("16x16x32", in, out, clk, blocks, iters);
    }
    for (int rep = 0; rep < 6; ++rep) {      // interleaved: the two shapes of the fused resblock's pattern, same output tile per wave
        runf<0>("32x32x16", inf, out, clk, blocks, iters);
        runf<1>("16x16x32", inf, out, clk, blocks, iters);
    }
    return 0;
}
