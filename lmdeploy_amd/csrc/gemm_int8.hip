// INT8 x INT8 linear (W8A8) on the CDNA4 int8 matrix cores (v_mfma_i32_32x32x32_i8): int8 weight codes with one fp32 scale per
// output column, activations quantised on the fly with one scale per token.
//
// Replaces: the reference's PyTorch-engine W8A8 path (pytorch/models/q_modules.py: per_token_quant_int8 with eps 1e-7, then
//           matmul_kernel_dynamic_quant; pytorch/kernels/cuda/w8a8_triton_kernels.py:83-87, 225-260) for checkpoints written by
//           `lmdeploy lite smooth_quant` or published as compressed-tensors "int-quantized"; its TurboMind engine refuses the form.
// Arithmetic (tests/int8_reference.py restates it):
//   activation, per fp16 row in fp32: absmax = max(max|x|, 1e-7), sx = absmax / 127, q = clamp(round_half_away(x / sx), -127, 127)
//     (x / sx is the IEEE division, not a product with a reciprocal);
//   y[m, n] = h((float(acc) * sx[m]) * sw[n]),  acc = sum over ALL of K of xq[m, k] * wq[k, n] in int32 (exact: K <= 32768),
//     float() rounds to nearest even, h = the fp16 store or the gated-SiLU epilogue on the scaled fp32 values.
//   Departure from the reference: its quantiser is fused into RMSNorm without the eps (an all-zero row gives NaN); here the quantiser is
//   a launch of its own on the fp16 norm output and always clamps at 1e-7.
//
// MI355X design -- the channel-scaled arm of gemm_fp8.hip with the int8 data path:
//   * the weight image is the "P8" image of gemm_fp8.hip, unchanged (the codes are opaque bytes), with the N column scales behind
//     its last unit.  The 16-byte vector v a lane holds per unit (the 16-k steps 2v and 2v + 1) is ONE A operand of the K = 32
//     instruction; the B operand is the two matching 8-byte x pieces.  Inside a lane half the matrix core pairs byte i of A with
//     byte i of B, so which k a byte is does not matter as long as both operands agree: lane half h, byte i < 8 is
//     k = 32v + 8h + i, byte i >= 8 is k = 32v + 16 + 8h + (i - 8) on both sides.  D as for every 32x32 form: lane = x row
//     (l & 31), register r = weight column (r & 3) + 8 (r >> 2) + 4 (l >> 5);
//   * x codes global -> LDS by LDS-DMA in swizzled stages, weights HBM -> registers -> MFMA, CG column groups x WK k-phases, the
//     k-phase partial tiles summed through LDS as int32;
//   * split-K: the slices store RAW int32 accumulators, and one reduce kernel sums them as integers, converts once, scales and
//     applies the epilogue -- the result is the same bits for every split.  The slabs never leave this file: the engine's deferred
//     reduce carries fp32 slabs, so an int8 linear always reduces itself.
#include "tm_common.h"
#include "tm_kernels.h"
#include <algorithm>
#include <type_traits>

namespace tmk {

typedef int intx4 __attribute__((ext_vector_type(4)));
typedef int intx16 __attribute__((ext_vector_type(16)));

// ---- per-token activation quantiser -----------------------------------------------------------------------------------
// The shape of quant_fp8_token_kernel: one workgroup = one row, the row in registers, absmax by DPP and through LDS, one pass over HBM.
template<int NV>
__global__ __launch_bounds__(256) void quant_int8_token_kernel(uint8_t* __restrict__ xq, float* __restrict__ sx, const half_t* __restrict__ x,
                                                               int ldx, int K)
{
    __shared__ float wmax[4];
    const int     m  = blockIdx.x;
    const int     nv = K / 8;
    const half_t* xr = x + (size_t)m * ldx;
    half8_t       v[NV];
    float         amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + threadIdx.x;
        if (c < nv) {
            v[i] = *(const half8_t*)(xr + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                amax = fmaxf(amax, fabsf((float)v[i][e]));
            }
        }
    }
    amax = group_max<64>(amax);
    if ((threadIdx.x & 63) == 0) {
        wmax[threadIdx.x >> 6] = amax;
    }
    __syncthreads();
    amax           = fmaxf(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])), 1e-7f);
    const float sc = amax / 127.0f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + threadIdx.x;
        if (c < nv) {
            uint32_t w[2] = {0, 0};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // correctly rounded division (|q| reaches 127.00001), ties away from zero, then the clamp
                const float r = fminf(fmaxf(__builtin_roundf((float)v[i][e] / sc), -127.0f), 127.0f);
                w[e >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (e & 3));
            }
            *(u32x2*)(xq + (size_t)m * K + c * 8) = u32x2{w[0], w[1]};
        }
    }
    if (threadIdx.x == 0) {
        sx[m] = sc;
    }
}

int launch_quant_int8_token(uint8_t* xq, float* sx, const half_t* x, int ldx, int M, int K, hipStream_t st)
{
    TM_REQUIRE(K % 128 == 0 && ldx % 8 == 0 && K <= kFp8TokenMaxK, "int8 per-token quantiser: K % 128 == 0, K <= 32768, 16-byte aligned rows");
    if (M == 0) {
        return 0;
    }
    if (K <= 4 * 2048) {
        quant_int8_token_kernel<4><<<M, 256, 0, st>>>(xq, sx, x, ldx, K);
    }
    else {
        quant_int8_token_kernel<16><<<M, 256, 0, st>>>(xq, sx, x, ldx, K);
    }
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- load-time repack ---------------------------------------------------------------------------------------------------
// The P8 image of gemm_fp8.hip (unit scale words unused) followed by the N fp32 column scales.  No weight-only image.
int linear_weight_prepare_int8(LinearWeight& w, const uint8_t* weight, const float* scales, hipStream_t st)
{
    TM_REQUIRE(w.K % 128 == 0 && w.N % 32 == 0 && w.K <= kFp8TokenMaxK, "int8 linear: K % 128 == 0, K <= 32768 and N % 32 == 0");
    TM_REQUIRE(p8_bytes(w.K, w.N) + (size_t)w.N * sizeof(float) < ((size_t)1 << 31), "int8 linear: its image reaches 2^31 bytes (32-bit offsets)");
    TM_REQUIRE(!w.packed && !w.packed32, "int8 linear: the handle already holds a weight of another format");
    w.type          = 4;
    w.group         = 128;
    w.packed8_bytes = p8_bytes(w.K, w.N) + (size_t)w.N * sizeof(float);
    if (!w.packed8) {
        TM_HIP_CHECK(hipMalloc(&w.packed8, w.packed8_bytes));
    }
    w.cscale = (float*)((char*)w.packed8 + p8_bytes(w.K, w.N));
    TM_HIP_CHECK(hipMemcpyAsync(w.cscale, scales, (size_t)w.N * sizeof(float), hipMemcpyDeviceToDevice, st));
    return launch_repack_p8(w.packed8, weight, nullptr, w.K, w.N, false, st);
}

bool int8_prepared(const LinearWeight& w)
{
    return w.fmt == LinearFormat::INT8_CHANNEL && w.type == 4 && w.packed8 != nullptr && w.cscale != nullptr;
}

// ---- GEMM -----------------------------------------------------------------------------------------------------------------
struct Int8Params {
    const uint8_t* xq;  // [M][K] int8 codes
    const float*   sx;  // [M] one scale per token
    const void*    wp;  // P8 units, then the N column scales
    half_t*        y;
    int            ldy;
    int*           partial;  // [splits][M][N] raw accumulators
    int            M, N, K, KB, ncg;
    int            kb_per_split;
    int            epilogue;  // 0 fp16, 1 gated SiLU fp16, 2 int32 slab of split blockIdx.y
};

template<int N, class F, int I = 0>
__device__ __forceinline__ void static_for_i8(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for_i8<N, F, I + 1>(static_cast<F&&>(f));
    }
}

// the one conversion and scaling of four adjacent columns of row m, and the store: shared by the GEMM's own epilogue and the split-K
// reduce, so both give the same bits
__device__ __forceinline__ void int8_scale_store(half_t* y, int ldy, size_t m, int n, intx4 acc, float rsx, floatx4 sw, bool gated)
{
    floatx4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = ((float)acc[i] * rsx) * sw[i];  // int32 -> fp32 rounds to nearest even; the reference's order of the two scales
    }
    if (gated) {
        const float s0 = a[0] / (1.0f + __builtin_expf(-a[0]));
        const float s1 = a[2] / (1.0f + __builtin_expf(-a[2]));
        half2_t     o  = {(half_t)(s0 * a[1]), (half_t)(s1 * a[3])};
        *(half2_t*)(y + m * ldy + (n >> 1)) = o;
    }
    else {
        half4_t o = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3]};
        *(half4_t*)(y + m * ldy + n) = o;
    }
}

// gemm_fp8_kernel<MH, CG, WK, S, false, true> with int8 operands: the same stages, ring, swizzle and wait counts; one MFMA per 16-byte
// weight vector instead of two, int32 accumulators chained over every k-block of the slice
template<int MH, int CG, int WK, int S>
__global__ __launch_bounds__(CG* WK * 64) void gemm_int8_kernel(Int8Params p)
{
    constexpr int WAVES = CG * WK;
    constexpr int T     = WAVES * 64;
    constexpr int ROWS  = 32 * MH;
    constexpr int KBB   = ROWS * 128;  // LDS bytes of one k-block of codes
    constexpr int STG   = S * KBB;
    constexpr int BPS   = S / WK;
    constexpr int PF    = 2 * BPS;       // ring = two stages
    constexpr int NPC   = S * ROWS / 8;  // 1-KiB DMA pieces (8 rows x 128 B) per stage
    constexpr int DR    = (NPC + WAVES - 1) / WAVES;
    static_assert(S % WK == 0, "tile parameters");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cgl  = wave % CG;
    const int wk   = wave / CG;
    const int l31  = lane & 31;
    const int half = lane >> 5;

    const int m0   = blockIdx.z * ROWS;
    const int Mloc = min(ROWS, p.M - m0);
    const int cg   = blockIdx.x * CG + cgl;
    const int cgc  = min(cg, p.ncg - 1);
    const int kb0  = blockIdx.y * p.kb_per_split;
    const int nkb  = min(p.kb_per_split, p.KB - kb0);
    const int nst  = (nkb + S - 1) / S;

    const int  wbytes = p.KB * p.ncg * kP8Unit;  // < 2^31: linear_weight_prepare_int8
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, wbytes, 0x00020000);
    const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.xq, 0, (int)((size_t)p.M * p.K), 0x00020000);
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)p.sx, 0, p.M * 4, 0x00020000);
    const auto rs_c = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)p.wp + wbytes), 0, p.N * 4, 0x00020000);

    // x / sx row of local row m (clamped duplicates past Mloc only feed rows that are never stored)
    auto xrow = [&](int m) { return m0 + min(m, Mloc - 1); };

    intx16 acc[MH];
#pragma unroll
    for (int h = 0; h < MH; ++h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[h][r] = 0;
        }
    }
    // B piece of 16-k step j: row (l & 31) [+ 32h], 16-byte unit j XOR-swizzled by (row >> 1) & 7, 8-byte half (l >> 5)
    int coff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        coff[j] = l31 * 128 + ((j ^ ((l31 >> 1) & 7)) << 4) + half * 8;
    }
    // DMA pieces of a stage: piece pc = r * WAVES + wave = k-block pc / (ROWS / 8), rows 8 (pc % (ROWS / 8)) + (lane >> 3);
    // lane L lands at slot L & 7 of its row and therefore fetches unit (L & 7) ^ ((row >> 1) & 7)
    int            doff[DR];
    const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)smem);
#pragma unroll
    for (int r = 0; r < DR; ++r) {
        const int pc  = min(r * WAVES + wave, NPC - 1);
        const int kbi = pc / (ROWS / 8);
        const int row = (pc % (ROWS / 8)) * 8 + (lane >> 3);
        const int u   = (lane & 7) ^ ((row >> 1) & 7);
        doff[r]       = xrow(row) * p.K + kbi * 128 + u * 16;
    }
    const int my_dr = NPC % WAVES == 0 ? DR : (wave < NPC - (DR - 1) * WAVES ? DR : DR - 1);  // wave-uniform
#define I8_DMA_X(t, buf)                                                                                          \
    _Pragma("unroll") for (int r = 0; r < DR; ++r)                                                                \
    {                                                                                                             \
        if (r < my_dr) {                                                                                          \
            unsigned       keep_;                                                                                 \
            const unsigned dst_ = lds0 + (buf)*STG + (r * WAVES + wave) * 1024;                                   \
            const int      so_  = (kb0 + (t)*S) * 128;                                                            \
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"                                       \
                         "buffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"                               \
                         : "=&s"(keep_)                                                                           \
                         : "v"(doff[r]), "s"(rs_x), "s"(dst_), "s"(so_)                                           \
                         : "memory");                                                                             \
        }                                                                                                         \
    }

    u32x4     ring[PF][4];
    const int vw = lane * 16;
#define I8_LOAD_W(slot, b)                                                                                        \
    {                                                                                                             \
        const int kbx_ = kb0 + min((b), nkb - 1);                                                                 \
        const int uo_  = (kbx_ * p.ncg + cgc) * kP8Unit;                                                          \
        _Pragma("unroll") for (int v = 0; v < 4; ++v)                                                             \
        {                                                                                                         \
            ring[slot][v] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, vw + v * 1024, uo_, /*nt*/ 2);            \
        }                                                                                                         \
    }
    constexpr int LPB = 4;  // loads per ring slot (the vmcnt arithmetic below counts them)

    if (nst > 0) {
        I8_DMA_X(0, 0);
#pragma unroll
        for (int q = 0; q < PF; ++q) {
            I8_LOAD_W(q, (q / BPS) * S + wk + (q % BPS) * WK);
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(LPB * PF) : "memory");  // everything older than the ring: x(0)
        __syncthreads();

        auto stage = [&](auto U, const int t) __attribute__((always_inline)) {
            constexpr int u   = decltype(U)::value;
            const int     buf = u & 1;
            // make hipcc wait for this stage's ring slots HERE, then start the (invisible to its waitcnt pass) DMA of x(t+1)
#pragma unroll
            for (int i = 0; i < BPS; ++i) {
                asm volatile("" ::"v"(ring[u * BPS + i][0]), "v"(ring[u * BPS + i][3]));
            }
            if (t + 1 < nst) {  // uniform; a DMA behind the last stage could land on the reduction image
                I8_DMA_X(t + 1, buf ^ 1);
            }
#pragma unroll
            for (int i = 0; i < BPS; ++i) {
                const int   slot = u * BPS + i;
                const int   kbi  = wk + i * WK;
                const char* xb   = smem + buf * STG + kbi * KBB;
                if (t * S + kbi < nkb) {  // wave-uniform; a k-block past the slice contributes nothing (its operands are clamped re-reads)
                    static_for_i8<4>([&](auto V) {
                        constexpr int v = decltype(V)::value;
                        const intx4   a = bit_cast<intx4>(ring[slot][v]);
#pragma unroll
                        for (int h = 0; h < MH; ++h) {
                            const u32x2 b0 = *(const u32x2*)(xb + h * 4096 + coff[2 * v]);
                            const u32x2 b1 = *(const u32x2*)(xb + h * 4096 + coff[2 * v + 1]);
                            const intx4 b  = {(int)b0[0], (int)b0[1], (int)b1[0], (int)b1[1]};
                            acc[h]         = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[h], 0, 0, 0);
                        }
                    });
                }
            }
#pragma unroll
            for (int i = 0; i < BPS; ++i) {
                I8_LOAD_W(u * BPS + i, (t + 2) * S + wk + i * WK);
            }
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(LPB * BPS) : "memory");  // my DMA pieces of x(t+1) have landed
            __syncthreads();
        };
        int t0 = 0;
        for (; t0 + 2 <= nst; t0 += 2) {
            static_for_i8<2>([&](auto U) { stage(U, t0 + decltype(U)::value); });
        }
        if (t0 < nst) {
            stage(std::integral_constant<int, 0>{}, t0);
        }
    }
#undef I8_DMA_X
#undef I8_LOAD_W

    // ---- k-phase reduction (int32) + whole-row stores -----------------------------------------------------------------------
    {
        constexpr int C4  = CG * 8;
        intx4*        red = (intx4*)smem;
#pragma unroll
        for (int h = 0; h < MH; ++h) {
            const int m = 32 * h + l31;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int c4 = cgl * 8 + 2 * g4 + half;
                red[(wk * ROWS + m) * C4 + (c4 ^ (m & 7))] = intx4{acc[h][4 * g4], acc[h][4 * g4 + 1], acc[h][4 * g4 + 2], acc[h][4 * g4 + 3]};
            }
        }
        __syncthreads();
        constexpr int NE    = ROWS * C4;
        const int     ncol0 = blockIdx.x * CG * 32;
#pragma unroll
        for (int e0 = 0; e0 < NE; e0 += T) {
            const int e = e0 + tid;
            if (NE % T != 0 && e >= NE) {
                break;
            }
            const int m  = e / C4;
            const int c4 = e % C4;
            intx4     a  = red[m * C4 + (c4 ^ (m & 7))];
#pragma unroll
            for (int k = 1; k < WK; ++k) {
                a += red[(k * ROWS + m) * C4 + (c4 ^ (m & 7))];
            }
            const int n = ncol0 + c4 * 4;
            if (m >= Mloc || n >= p.N) {
                continue;
            }
            const size_t mg = (size_t)m0 + m;
            if (p.epilogue == 2) {
                *(intx4*)(p.partial + ((size_t)blockIdx.y * p.M + mg) * p.N + n) = a;
                continue;
            }
            const float rsx = bit_cast<float>(__builtin_amdgcn_raw_buffer_load_b32(rs_s, (m0 + m) * 4, 0, 0));
            const u32x4 cs  = __builtin_amdgcn_raw_buffer_load_b128(rs_c, n * 4, 0, 0);
            int8_scale_store(p.y, p.ldy, mg, n, a, rsx, bit_cast<floatx4>(cs), p.epilogue == 1);
        }
    }
}

// y = epilogue(scale(sum_s partial[s])): the integer sum of the slices' raw accumulators, then the one conversion; 4 columns per thread
__global__ __launch_bounds__(256) void int8_splitk_reduce_kernel(half_t* __restrict__ y, int ldy, const int* __restrict__ partial, int splits,
                                                                 const float* __restrict__ sx, const float* __restrict__ sw, int M, int N,
                                                                 int gated)
{
    const size_t idx   = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)M * N / 4;
    if (idx >= total) {
        return;
    }
    const int m = idx / (N / 4);
    const int n = (idx - (size_t)m * (N / 4)) * 4;
    intx4     a = {0, 0, 0, 0};
    for (int s = 0; s < splits; ++s) {
        a += *(const intx4*)(partial + ((size_t)s * M + m) * N + n);
    }
    int8_scale_store(y, ldy, (size_t)m, n, a, sx[m], *(const floatx4*)(sw + n), gated != 0);
}

template<int MH, int CG, int WK>
static int launch_int8_one(const Int8Params& p, dim3 grid, hipStream_t st)
{
    constexpr int S     = 4;
    constexpr int stage = 2 * S * 32 * MH * 128;
    constexpr int red   = WK * 32 * MH * CG * 128;
    constexpr int lds   = stage > red ? stage : red;
    if (const int rc = ensure_dynamic_lds((const void*)gemm_int8_kernel<MH, CG, WK, S>, lds)) {
        return rc;
    }
    gemm_int8_kernel<MH, CG, WK, S><<<grid, CG * WK * 64, lds, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// y = int8 x int8 linear of PRE-QUANTISED activations (xq, sx from launch_quant_int8_token).  splits = 0: the fp8 kernel's heuristic;
// workspace = room for 16 int32 slabs [M][N], or nullptr: one slice.  A split launch is reduced here; y always holds the result.
int launch_linear_int8(const LinearWeight& w, const uint8_t* xq, const float* sx, half_t* y, int ldy, int M, bool gated_silu, int splits,
                       void* workspace, hipStream_t st)
{
    TM_REQUIRE(int8_prepared(w), "int8 linear: a weight prepared by linear_weight_prepare_int8");
    TM_REQUIRE(splits >= 0 && splits <= 16, "int8 linear: 0 <= splits <= 16");
    if (M == 0) {
        return 0;
    }
    TM_REQUIRE((size_t)M * w.K < ((size_t)1 << 31), "int8 linear: M * K reaches 2^31 (the x codes are addressed with 32-bit offsets)");
    Int8Params p{};
    p.xq = xq, p.sx = sx, p.wp = w.packed8, p.y = y, p.ldy = ldy, p.partial = (int*)workspace;
    p.M = M, p.N = w.N, p.K = w.K, p.KB = w.K / 128, p.ncg = w.N / 32;
    const int rows_per = M <= 32 ? 32 : 64;
    const int zb       = (M + rows_per - 1) / rows_per;
    TM_REQUIRE(zb <= 65535, "int8 linear: row blocks exceed grid.z (65535): split the forward into fewer tokens");
    const int col_wgs  = (p.ncg + 3) / 4 * zb;
    int       sp       = workspace ? fp8_splits(col_wgs, p.KB, splits) : 1;
    int       per      = (p.KB + sp - 1) / sp;
    per                = std::min((per + 3) / 4 * 4, p.KB);
    sp                 = (p.KB + per - 1) / per;
    p.kb_per_split     = per;
    p.epilogue         = sp > 1 ? 2 : (gated_silu ? 1 : 0);
    dim3 grid((p.ncg + 3) / 4, sp, zb);
    if (const int rc = M <= 32 ? launch_int8_one<1, 4, 4>(p, grid, st) : launch_int8_one<2, 4, 2>(p, grid, st)) {
        return rc;
    }
    if (sp > 1) {
        const size_t total = (size_t)M * w.N / 4;
        int8_splitk_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(y, ldy, p.partial, sp, sx, w.cscale, M, w.N, gated_silu ? 1 : 0);
        TM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace tmk
