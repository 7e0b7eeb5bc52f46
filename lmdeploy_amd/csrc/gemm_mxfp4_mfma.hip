// MXFP4 x MXFP4 ("W4A4") dense linear on the CDNA4 block-scaled matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4, both operands e2m1):
// e2m1 weights with one e8m0 scale byte per 32 k, activations quantised on the fly per row and group of 32 by the same rule.
//
// Arithmetic (tests/mxfp4_dense_reference.py):
//   activation: amax over the 32 channels, e = floor(log2(amax)) - 2 (-127 for a zero group), scale byte e + 127,
//               code = e2m1_rne_sat(x / 2^e) (ties to the even mantissa, |v| > 6 -> 6, the sign of zero kept);
//   y[m, n] = h( sum_g 2^(sx[m, g] - 127) 2^(sw[n, g] - 127) sum_{k in g} xq[m, k] wq[n, k] )
//   with the whole sum over K chained in the fp32 accumulator of the matrix core: both scale bytes are operands of the instruction,
//   there is no per-group fma and no epilogue scale.
//
// What the hardware does (established with exact data on an MI355X):
//   * v_mfma_scale_f32_32x32x64_f8f6f4, cbsz = blgp = 4 (FP4): lane l holds the 32 k-contiguous elements k = 32 (l >> 5) .. + 32 of row
//     (A) / column (B) l & 31 in the first 4 of its 8 operand VGPRs, element k in nibble k & 7 of dword k >> 3 (low nibble first);
//     the byte `op_sel` of the lane's scale VGPR scales those 32 elements; C / D as every 32x32 MFMA
//     (column = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)).
//   * v_cvt_scalef32_pk_fp4_f16 DIVIDES by its fp32 scale operand, rounds to nearest with ties to the even mantissa, saturates to +-6,
//     keeps the sign of zero and converts fp16 subnormals; source element 0 lands in the low nibble of the byte `byte_sel`.  That is the
//     contract for every finite input, so no input class is rounded on the VALU.
//
// Layout "P4": unit (kb, cg) = 32 columns x 128 k = 2048 B of codes in A-operand order (16-byte vector v = the MFMA of k 64 v .. + 64,
// lane l: column 32 cg + (l & 31), k = 128 kb + 64 v + 32 (l >> 5) .. + 32) followed by 32 dwords = the four scale bytes of each
// column's k-groups 4 kb .. + 4 -- 2176-byte units, k-block-major, one descriptor, HBM -> operand registers with no VALU in between
// (a lane shifts its column's scale dword by 8 (l >> 5) so that op_sel 0 / 2 address the groups of the two MFMAs).
//
// Kernel: CG column groups x WK k-phases per workgroup, MH 32-row blocks; a wave streams its units and the x codes / x scale bytes of
// its rows through buffer loads into the operands, k-phases are summed through LDS, whole-row stores (fp16, gated SiLU, fp32 split-K
// slabs) as gemm_fp8.hip.  x is read from L2 by every wave that needs it: staging it by LDS-DMA is not built.
#include "tm_common.h"
#include "tm_kernels.h"
#include <algorithm>

namespace tmk {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef int   intx8 __attribute__((ext_vector_type(8)));

constexpr int kP4Unit = 2048 + 128;

// ---- activation quantiser -----------------------------------------------------------------------------------------------
// 4 lanes = one (row, group of 32): 8 halves per lane, absmax by DPP inside the quad, 8 codes (one dword) per lane.
__global__ __launch_bounds__(256) void quant_mxfp4_rows_kernel(uint8_t* __restrict__ xq, uint8_t* __restrict__ sx, const half_t* __restrict__ x,
                                                               int ldx, int M, int K)
{
    const int     groups = K / 32;
    const int64_t total  = (int64_t)M * groups;
    const int64_t gid    = (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);  // (row, group) index
    const int     l4     = threadIdx.x & 3;
    const bool    ok     = gid < total;
    const int64_t gc     = ok ? gid : total - 1;
    const int     m      = (int)(gc / groups);
    const int     g      = (int)(gc - (int64_t)m * groups);
    const half8_t v      = *(const half8_t*)(x + (size_t)m * ldx + g * 32 + l4 * 8);
    float         amax   = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        amax = fmaxf(amax, fabsf((float)v[e]));
    }
    amax = fmaxf(amax, dpp_f32<DPP_XOR1>(amax));
    amax = fmaxf(amax, dpp_f32<DPP_XOR2>(amax));
    // every finite fp16 is a normal fp32: its exponent field is floor(log2(amax)) + 127
    const int   sb    = amax == 0.f ? 0 : (int)(bit_cast<uint32_t>(amax) >> 23) - 2;  // scale byte e + 127
    const float scale = amax == 0.f ? 1.0f : bit_cast<float>((uint32_t)sb << 23);     // 2^e (a zero group holds +-0 only)
    uint32_t    w     = 0;
    w                 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(w, half2_t{v[0], v[1]}, scale, 0);
    w                 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(w, half2_t{v[2], v[3]}, scale, 1);
    w                 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(w, half2_t{v[4], v[5]}, scale, 2);
    w                 = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(w, half2_t{v[6], v[7]}, scale, 3);
    if (ok) {
        *(uint32_t*)(xq + (size_t)m * (K / 2) + g * 16 + l4 * 4) = w;
        if (l4 == 0) {
            sx[(size_t)m * groups + g] = (uint8_t)sb;
        }
    }
}

int launch_quant_mxfp4_rows(uint8_t* xq, uint8_t* sx, const half_t* x, int ldx, int M, int K, hipStream_t st)
{
    TM_REQUIRE(K > 0 && K % 128 == 0 && ldx % 8 == 0 && ldx >= K, "mxfp4 row quantiser: K % 128 == 0, 16-byte aligned rows, ldx >= K");
    if (M <= 0) {
        return 0;
    }
    const int64_t n = (int64_t)M * (K / 32);
    TM_REQUIRE((n + 63) / 64 < ((int64_t)1 << 31), "mxfp4 row quantiser: M * K / 32 groups exceed the grid");
    quant_mxfp4_rows_kernel<<<(unsigned)((n + 63) / 64), 256, 0, st>>>(xq, sx, x, ldx, M, K);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- load-time repack -------------------------------------------------------------------------------------------------------
// blocks [N][K/2] (byte j of row n: k = 2j low nibble, 2j + 1 high nibble), scales [N][K/32] -> P4 units.  One thread = one dword.
__global__ void repack_p4_kernel(uint32_t* __restrict__ out, const uint8_t* __restrict__ blocks, const uint8_t* __restrict__ scales, int K, int N)
{
    const size_t idx   = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int    ncg   = N / 32;
    const size_t total = (size_t)(K / 128) * ncg * (kP4Unit / 4);
    if (idx >= total) {
        return;
    }
    const size_t unit = idx / (kP4Unit / 4);
    const int    d    = (int)(idx % (kP4Unit / 4));
    const int    cg   = (int)(unit % ncg);
    const int    kb   = (int)(unit / ncg);
    if (d >= 512) {  // the four scale bytes of column d - 512
        const int n = cg * 32 + (d - 512);
        out[idx]    = *(const uint32_t*)(scales + (size_t)n * (K / 32) + kb * 4);
        return;
    }
    // dword d: vector v = d >> 8, lane = (d >> 2) & 63, dword-in-vector dd = d & 3 -> k = 128 kb + 64 v + 32 (lane >> 5) + 8 dd .. + 8
    const int v    = d >> 8;
    const int lane = (d >> 2) & 63;
    const int dd   = d & 3;
    const int n    = cg * 32 + (lane & 31);
    const int k0   = kb * 128 + 64 * v + 32 * (lane >> 5) + 8 * dd;
    out[idx]       = *(const uint32_t*)(blocks + (size_t)n * (K / 2) + k0 / 2);
}

// the fp16 [N][K] image rebuilt from the units: lut[code] * 2^(s - 127).  One thread = one dword of codes (8 k).
__global__ void dequant_p4_f16_kernel(half_t* __restrict__ out, const uint32_t* __restrict__ units, int K, int N)
{
    const size_t idx   = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int    ncg   = N / 32;
    const size_t total = (size_t)(K / 128) * ncg * 512;
    if (idx >= total) {
        return;
    }
    const size_t    unit = idx / 512;
    const int       d    = (int)(idx % 512);
    const int       cg   = (int)(unit % ncg);
    const int       kb   = (int)(unit / ncg);
    const int       v    = d >> 8;
    const int       lane = (d >> 2) & 63;
    const int       dd   = d & 3;
    const int       n    = cg * 32 + (lane & 31);
    const int       kl   = 64 * v + 32 * (lane >> 5) + 8 * dd;  // k inside the k-block
    const uint32_t* u    = units + unit * (kP4Unit / 4);
    const uint32_t  c    = u[d];
    const int       s    = (int)((u[512 + (lane & 31)] >> (8 * (kl >> 5))) & 255);
    const float     lut[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
    half8_t         o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t q = (c >> (4 * e)) & 15;
        const float    f = ldexpf(lut[q & 7], s - 127);
        o[e]             = (half_t)((q & 8) ? -f : f);
    }
    *(half8_t*)(out + (size_t)n * K + kb * 128 + kl) = o;
}

size_t p4_bytes(int K, int N)
{
    return (size_t)(K / 128) * (N / 32) * kP4Unit;
}

static const char* const kMx4Limits = "mxfp4 dense linear: K % 128 == 0, N % 32 == 0 and K * N / 2 < 2^31";

int linear_weight_prepare_mxfp4_dense(LinearWeight& w, const uint8_t* blocks, const uint8_t* scales, hipStream_t st)
{
    TM_REQUIRE(w.type == 3, "mxfp4 dense linear: a TM_WEIGHT_MXFP4 handle");
    w.group = 32;
    TM_REQUIRE(w.K % 128 == 0 && w.N % 32 == 0 && (size_t)w.K * w.N / 2 < ((size_t)1 << 31), kMx4Limits);
    TM_REQUIRE(!w.packed, "mxfp4 dense linear: the handle already holds an expert weight");
    w.packed8_bytes = p4_bytes(w.K, w.N);
    if (!w.packed8) {
        TM_HIP_CHECK(hipMalloc(&w.packed8, w.packed8_bytes));
    }
    const size_t total = w.packed8_bytes / 4;
    repack_p4_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((uint32_t*)w.packed8, blocks, scales, w.K, w.N);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

bool mxfp4_dense_prepared(const LinearWeight& w)
{
    return w.type == 3 && w.packed8 != nullptr && !w.packed;
}

int launch_dequant_p4_f16(half_t* out_nk, const LinearWeight& w, hipStream_t st)
{
    TM_REQUIRE(mxfp4_dense_prepared(w), "mxfp4 dense linear: weight not prepared (tm_linear_prepare_mxfp4)");
    const size_t total = (size_t)(w.K / 128) * (w.N / 32) * 512;
    dequant_p4_f16_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(out_nk, (const uint32_t*)w.packed8, w.K, w.N);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- GEMM ---------------------------------------------------------------------------------------------------------------------
struct Mx4Params {
    const uint8_t* xq;  // [M][K/2] e2m1 codes
    const uint8_t* sx;  // [M][K/32] e8m0 scale bytes
    const void*    wp;  // P4 units
    half_t*        y;
    int            ldy;
    float*         partial;
    int            M, N, K, KB, ncg;
    int            kb_per_split;
    int            epilogue;  // 0 fp16, 1 gated SiLU fp16, 2 fp32 slab of split blockIdx.y
};

template<int MH, int CG, int WK>
__global__ __launch_bounds__(CG* WK * 64) void gemm_mxfp4_mfma_kernel(Mx4Params p)
{
    constexpr int T    = CG * WK * 64;
    constexpr int ROWS = 32 * MH;

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

    // every load goes through a descriptor: an offset past the image reads zero instead of faulting
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, (int)((size_t)p.KB * p.ncg * kP4Unit), 0x00020000);
    const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.xq, 0, (int)((size_t)p.M * (p.K / 2)), 0x00020000);
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)p.sx, 0, (int)((size_t)p.M * (p.K / 32)), 0x00020000);

    floatx16 acc[MH];
    int      xoff[MH], soff[MH];
#pragma unroll
    for (int h = 0; h < MH; ++h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[h][r] = 0.f;
        }
        const int row = m0 + min(32 * h + l31, Mloc - 1);  // clamped duplicates past Mloc only feed rows that are never stored
        xoff[h]       = row * (p.K / 2) + 16 * half;
        soff[h]       = row * (p.K / 32);
    }
    const int vw = lane * 16;
    const int sh = 8 * half;  // op_sel 0 / 2 then address the scale bytes of k-groups (half, 2 + half) of the k-block

    for (int kb = wk; kb < nkb; kb += WK) {
        const int   kbx = kb0 + kb;
        const int   uo  = (kbx * p.ncg + cgc) * kP4Unit;
        const u32x4 w0  = __builtin_amdgcn_raw_buffer_load_b128(rs_w, vw, uo, /*nt*/ 2);
        const u32x4 w1  = __builtin_amdgcn_raw_buffer_load_b128(rs_w, vw + 1024, uo, /*nt*/ 2);
        const int   ws  = (int)((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_w, 2048 + l31 * 4, uo, 0) >> sh);
        const intx8 a0  = {(int)w0[0], (int)w0[1], (int)w0[2], (int)w0[3], 0, 0, 0, 0};
        const intx8 a1  = {(int)w1[0], (int)w1[1], (int)w1[2], (int)w1[3], 0, 0, 0, 0};
#pragma unroll
        for (int h = 0; h < MH; ++h) {
            const u32x4 x0 = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff[h], kbx * 64, 0);
            const u32x4 x1 = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff[h] + 32, kbx * 64, 0);
            const int   xs = (int)((uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs_s, soff[h], kbx * 4, 0) >> sh);
            const intx8 b0 = {(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], 0, 0, 0, 0};
            const intx8 b1 = {(int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3], 0, 0, 0, 0};
            acc[h]         = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b0, acc[h], 4, 4, 0, ws, 0, xs);
            acc[h]         = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b1, acc[h], 4, 4, 2, ws, 2, xs);
        }
    }

    // ---- k-phase reduction + whole-row stores (as gemm_fp8.hip) ----------------------------------------------------------
    {
        constexpr int C4  = CG * 8;
        floatx4*      red = (floatx4*)smem;
#pragma unroll
        for (int h = 0; h < MH; ++h) {
            const int m = 32 * h + l31;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int c4 = cgl * 8 + 2 * g4 + half;
                red[(wk * ROWS + m) * C4 + (c4 ^ (m & 7))] =
                    floatx4{acc[h][4 * g4], acc[h][4 * g4 + 1], acc[h][4 * g4 + 2], acc[h][4 * g4 + 3]};
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
            floatx4   a  = red[m * C4 + (c4 ^ (m & 7))];
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
                *(floatx4*)(p.partial + ((size_t)blockIdx.y * p.M + mg) * p.N + n) = a;
            }
            else if (p.epilogue == 1) {
                const float s0 = a[0] / (1.0f + __builtin_expf(-a[0]));
                const float s1 = a[2] / (1.0f + __builtin_expf(-a[2]));
                half2_t     o  = {(half_t)(s0 * a[1]), (half_t)(s1 * a[3])};
                *(half2_t*)(p.y + mg * p.ldy + (n >> 1)) = o;
            }
            else {
                half4_t o = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3]};
                *(half4_t*)(p.y + mg * p.ldy + n) = o;
            }
        }
    }
}

template<int MH, int CG, int WK>
static int launch_mx4_one(const Mx4Params& p, dim3 grid, hipStream_t st)
{
    constexpr int lds = WK * 32 * MH * CG * 128;
    if (const int rc = ensure_dynamic_lds((const void*)gemm_mxfp4_mfma_kernel<MH, CG, WK>, lds)) {
        return rc;
    }
    gemm_mxfp4_mfma_kernel<MH, CG, WK><<<grid, CG * WK * 64, lds, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

size_t mxfp4_act_workspace_bytes(int rows, int K)
{
    // codes [rows][K/2] + scale bytes [rows][K/32]
    return (size_t)rows * (K / 2) + (size_t)rows * (K / 32) + 256;
}

static int mx4_splits(int col_wgs, int KB, int want)
{
    if (want > 0) {
        return want;
    }
    int splits = 1;
    for (int s = 2; s <= 16; ++s) {
        const int per = (KB + s - 1) / s;
        if ((KB + per - 1) / per == s && col_wgs * s <= 256 && per >= 4) {
            splits = s;
        }
    }
    return splits;
}

// y = MXFP4 x MXFP4 linear of PRE-QUANTISED activations (xq, sx from launch_quant_mxfp4_rows).  splits = 0: heuristic.  Two row
// regimes: M <= 128 is one weight-streaming tile of 32 / 64 / 128 rows (every unit is read once) with split-K over the CUs;
// larger M runs 128-row tiles over grid.z.
int launch_linear_mxfp4(const LinearWeight& w, const uint8_t* xq, const uint8_t* sx, half_t* y, int ldy, int M, bool gated_silu, int splits,
                        float* workspace, int* slabs_out, hipStream_t st)
{
    TM_REQUIRE(mxfp4_dense_prepared(w), "mxfp4 dense linear: weight not prepared (tm_linear_prepare_mxfp4)");
    TM_REQUIRE((size_t)M * (w.K / 2) < ((size_t)1 << 31), "mxfp4 dense linear: M * K / 2 < 2^31");
    if (slabs_out) {
        *slabs_out = 1;
    }
    if (M <= 0) {
        return 0;
    }
    Mx4Params p{};
    p.xq = xq, p.sx = sx, p.wp = w.packed8, p.y = y, p.ldy = ldy, p.partial = workspace;
    p.M = M, p.N = w.N, p.K = w.K, p.KB = w.K / 128, p.ncg = w.N / 32;
    const int rows_per = M <= 32 ? 32 : M <= 64 ? 64 : 128;
    const int zb       = (M + rows_per - 1) / rows_per;
    const int col_wgs  = (p.ncg + 3) / 4 * zb;
    int       sp       = workspace ? (M <= 128 || splits > 0 ? mx4_splits(col_wgs, p.KB, splits) : 1) : 1;
    const int per      = (p.KB + sp - 1) / sp;
    sp                 = (p.KB + per - 1) / per;
    p.kb_per_split     = per;
    p.epilogue         = sp > 1 ? 2 : (gated_silu ? 1 : 0);
    dim3 grid((p.ncg + 3) / 4, sp, zb);
    int  rc;
    if (rows_per == 32) {
        rc = launch_mx4_one<1, 4, 4>(p, grid, st);
    }
    else if (rows_per == 64) {
        rc = launch_mx4_one<2, 4, 2>(p, grid, st);
    }
    else if (M <= 128) {
        rc = launch_mx4_one<4, 4, 2>(p, grid, st);
    }
    else {
        rc = launch_mx4_one<4, 4, 1>(p, grid, st);
    }
    if (rc) {
        return rc;
    }
    if (slabs_out) {
        *slabs_out = sp;
    }
    return 0;
}

}  // namespace tmk
