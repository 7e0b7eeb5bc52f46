// MXFP4 expert weights (gpt-oss) and the gpt-oss gated epilogue: grouped GEMM over experts for gfx950.
//
// Replaces: the e2m1 dequant transform with ue8m0 group scales (kernels/gemm/transform.h:83-90), AdjustUe8m0ScaleForHalf
//           (kernels/gemm/cast.cu:220-227), the gpt-oss activation (kernels/activation.cu:17-24) fused with the per-expert bias of the
//           w1w3 linear (models/llama/moe_ffn_layer.cc:272-275) into the GEMM epilogue.
//
// Format at the boundary (the published checkpoint layout): blocks uint8 [N][K/2], the low nibble of a byte is the even k; scales
// uint8 [N][K/32], one ue8m0 byte per 32 k.  Code c: sign c >> 3, magnitude {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7]; scale byte s: the fp16
// with exponent field f = clamp(s - 112, 0, 30) (s <= 112 flushes to +0, s >= 142 is 2^15, else 2^(s - 127)); w = h(value * scale), one fp16
// multiply, exact whenever finite.  y = h(sum_k f32(x) * f32(w)) with fp32 accumulation on the MFMA: from the operand on, the arithmetic
// of the fp16 tiles of gemm_kernel (gemm_w4a16.hip).
//
// Image: the k-block-major MFMA-fragment order repack_u4_kernel documents -- dword ((kb * N/16 + nt) * 64 + lane) * 4 + j holds the eight
// codes n = 16 nt + (lane & 15), k = 128 kb + 32 j + 8 (lane >> 4) + 0..7 -- so one 16-byte lane load is 4 MFMA k-steps = four 32-wide scale
// groups, and ONE u32 of four scale bytes per (k-block, column) goes with it where u4 has one (s, -z*s) pair: 4.25 bits per weight, as AWQ
// g128.  Inside a dword the codes keep the checkpoint's byte order (byte b = k 2b in the low, k 2b + 1 in the high nibble): that is the
// operand order of v_cvt_scalef32_pk_f16_fp4, which turns one byte into the packed fp16 pair (exact, scale 1.0).  The scale bytes are
// stored adjusted, 4 f: byte j moved to bits 8..15 and 24..31 is the packed fp16 pair (f << 10, f << 10) -- one byte permute -- and one
// v_pk_mul_f16 per pair applies it.  9 VALU per dword of codes (4 converts, 4 multiplies, 1 permute; the u4 path: 13).
//
// The kernel is gemm_kernel's grouped form (GemmGroup descriptors, seg / row_idx, zper row blocks; one k-block per barrier, no k-phases)
// with two operand types -- MXFP4 and fp16 -- and three epilogues: plain, gated SiLU, and the gated gpt-oss one with a per-expert bias.
// fp16 experts come here only for the gpt-oss epilogue; their plain and SiLU forms stay in gemm_kernel.
#include "tm_common.h"
#include "tm_kernels.h"
#include <algorithm>

namespace tmk {

// ---- load-time repack ----------------------------------------------------------------------------------------------------------
__global__ void repack_mxfp4_kernel(uint32_t* __restrict__ out, const uint8_t* __restrict__ blocks, int K, int N)
{
    // one thread per output dword: idx = ((kb*NTILES + nt)*64 + lane)*4 + j
    const size_t idx   = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)K * N / 8;
    if (idx >= total) {
        return;
    }
    const int    NTILES = N / 16;
    const int    j      = idx & 3;
    const int    lane   = (idx >> 2) & 63;
    const size_t tile   = idx >> 8;
    const int    nt     = tile % NTILES;
    const int    kb     = tile / NTILES;
    const int    n      = nt * 16 + (lane & 15);
    const int    k0     = kb * 128 + j * 32 + (lane >> 4) * 8;
    out[idx]            = *(const uint32_t*)(blocks + (size_t)n * (K / 2) + k0 / 2);  // K % 128 == 0: 4-byte aligned
}

// out[kb * N + n] = the four adjusted scale bytes of column n, k-block kb (byte j: the 32 k of MFMA step j)
__global__ void repack_mxfp4_scales_kernel(uint32_t* __restrict__ out, const uint8_t* __restrict__ scales, int KB, int N)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)KB * N) {
        return;
    }
    const int kb = (int)(idx / N);
    const int n  = (int)(idx % N);
    uint32_t  o  = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s = scales[(size_t)n * (KB * 4) + kb * 4 + j];
        const int f = min(max(s - 112, 0), 30);  // the fp16 exponent field, applied once here
        o |= (uint32_t)(f << 2) << (8 * j);
    }
    out[idx] = o;
}

int linear_weight_prepare_mxfp4(LinearWeight& w, const uint8_t* blocks, const uint8_t* scales, hipStream_t st)
{
    TM_REQUIRE(w.K % 128 == 0 && w.N % 16 == 0, "K % 128 == 0 and N % 16 == 0");
    TM_REQUIRE(gemm_general_image_bytes(w.K, w.N, 0) < kGeneralImageLimit, "mxfp4 linear: the packed image reaches 2^31 bytes");
    w.type         = 3;
    w.group        = 32;
    w.packed_bytes = (size_t)w.K * w.N / 2;
    w.sz_bytes     = (size_t)(w.K / 128) * w.N * 4;
    if (!w.packed) {
        TM_HIP_CHECK(hipMalloc(&w.packed, w.packed_bytes));
        TM_HIP_CHECK(hipMalloc((void**)&w.sz, w.sz_bytes));
    }
    const size_t nd = (size_t)w.K * w.N / 8;
    repack_mxfp4_kernel<<<(nd + 255) / 256, 256, 0, st>>>((uint32_t*)w.packed, blocks, w.K, w.N);
    TM_HIP_CHECK(hipGetLastError());
    const size_t ns = (size_t)(w.K / 128) * w.N;
    repack_mxfp4_scales_kernel<<<(ns + 255) / 256, 256, 0, st>>>(w.sz, scales, w.K / 128, w.N);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- operand -------------------------------------------------------------------------------------------------------------------
// the eight fp16 weights of image dword `w` (MFMA step j of its k-block) under the k-block's scale word `su`
template<int J>
__device__ __forceinline__ half8_t mx_dequant8(uint32_t w, uint32_t su)
{
    // bytes (0, su.byte[J], 0, su.byte[J]) = (4f << 8) | (4f << 24): v_perm_b32 selectors 0..3 take a byte of the second source, 0x0c is 0x00
    const half2_t s2 = bit_cast<half2_t>(__builtin_amdgcn_perm(0u, su, 0x000c000cu | (uint32_t)J << 8 | (uint32_t)J << 24));
    const half2_t  p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0) * s2;
    const half2_t  p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1) * s2;
    const half2_t  p2 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2) * s2;
    const half2_t  p3 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3) * s2;
    return half8_t{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
__device__ __forceinline__ half8_t mx_dequant8(uint32_t w, uint32_t su, int j)
{
    return j == 0 ? mx_dequant8<0>(w, su) : j == 1 ? mx_dequant8<1>(w, su) : j == 2 ? mx_dequant8<2>(w, su) : mx_dequant8<3>(w, su);
}

// the operand of every (k, n) as the GEMM builds it, written as fp16 [K][N]: one thread per image dword
__global__ void dequant_mxfp4_image_kernel(half_t* __restrict__ out, const uint32_t* __restrict__ img, const uint32_t* __restrict__ sz,
                                           int K, int N)
{
    const size_t idx   = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)K * N / 8;
    if (idx >= total) {
        return;
    }
    const int     NTILES = N / 16;
    const int     j      = idx & 3;
    const int     lane   = (idx >> 2) & 63;
    const size_t  tile   = idx >> 8;
    const int     nt     = tile % NTILES;
    const int     kb     = tile / NTILES;
    const int     n      = nt * 16 + (lane & 15);
    const int     k0     = kb * 128 + j * 32 + (lane >> 4) * 8;
    const half8_t v      = mx_dequant8(img[idx], sz[(size_t)kb * N + n], j);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        out[(size_t)(k0 + e) * N + n] = v[e];
    }
}

int launch_dequant_mxfp4_f16(half_t* out_kn, const LinearWeight& w, hipStream_t st)
{
    TM_REQUIRE(w.type == 3 && w.packed && w.sz, "mxfp4 dequant: a prepared MXFP4 linear");
    const size_t nd = (size_t)w.K * w.N / 8;
    dequant_mxfp4_image_kernel<<<(nd + 255) / 256, 256, 0, st>>>(out_kn, (const uint32_t*)w.packed, w.sz, w.K, w.N);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- grouped GEMM ----------------------------------------------------------------------------------------------------------------
struct MxGroup {  // = GemmGroup of gemm_w4a16.hip: what moe_build_groups writes
    const void* wq;
    const void* sz;
};

struct MxParams {
    const half_t*  x;
    int            ldx;
    half_t*        y;
    int            ldy;
    int            M, N, K;   // M: cap of rows per expert
    int            KB;        // K / 128
    int            epilogue;  // 0: fp16 store  1: gated SiLU  3: gated gpt-oss (+ bias)
    const MxGroup* groups;    // device [experts]
    const int*     seg;       // device [experts + 1]
    const int*     row_idx;   // device [flat rows] or nullptr
    int            zper;      // row blocks per expert
    int            x_rows;    // rows of x (bounds of the activation buffer descriptor)
    const half_t*  bias;      // device [experts][N] (epilogue 3; column order of the weights) or nullptr
};

// One workgroup = WN waves of NT column tiles (16 columns each) x MT row tiles (16 rows each) of ONE expert, over all of K, one k-block
// (128 k) per iteration: the structure of gemm_kernel<.., WK = 1, KS = 1, .., GRP = true> -- per-wave weight ring PF k-blocks deep,
// activations through a double-buffered XOR-swizzled LDS stage, one barrier per iteration, the operand of the next 32-k step built
// while the MFMAs of the current one run.  WT: 3 = MXFP4 (one 16-byte load + one scale word per tile and k-block), 1 = fp16 (four loads).
template<int WT, int MT, int NT, int WN, int PF>
__global__ __launch_bounds__(WN * 64) void gemm_mx_kernel(MxParams p)
{
    static_assert(PF % 2 == 0, "ring depth must be even (LDS stages alternate)");
    static_assert(WT == 1 || WT == 3, "fp16 or MXFP4 operands");
    constexpr int  MB      = 16 * MT;
    constexpr int  THREADS = WN * 64;
    constexpr int  ROWB    = 256;        // one k-block of one row
    constexpr int  BUFB    = MB * ROWB;  // one LDS stage
    constexpr int  NCHUNK  = MB * 16;    // 16-B chunks per stage
    constexpr int  XR      = (NCHUNK + THREADS - 1) / THREADS;
    constexpr int  WV      = WT == 3 ? 1 : 4;  // u32x4 per (tile, k-block) per lane
    constexpr bool XFULL   = NCHUNK % THREADS == 0;

    extern __shared__ __attribute__((aligned(16))) char smem[];  // 2 * BUFB

    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wn   = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16  = lane & 15;
    const int g    = lane >> 4;

    const int ntiles = p.N / 16;
    const int nt0    = (blockIdx.x * WN + wn) * NT;
    const int e      = blockIdx.z / p.zper;
    const int m0     = (blockIdx.z - e * p.zper) * MB;
    const int row0   = p.seg[e];
    const int Mloc   = min(p.seg[e + 1] - row0, p.M);
    if (m0 >= Mloc) {
        return;  // no rows for this block (whole workgroup, before any barrier)
    }
    const int nit = p.KB;

    // buffer descriptors + per-lane 32-bit byte offsets + scalar k-block offsets; tiles past the edge are clamped: loads stay in
    // bounds, stores are skipped
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.groups[e].wq, 0, (int)((size_t)p.KB * ntiles * 1024 * WV), 0x00020000);
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void*)p.groups[e].sz, 0, WT == 3 ? p.KB * ntiles * 64 : 0, 0x00020000);
    const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)(((size_t)(p.x_rows - 1) * p.ldx + p.K) * 2), 0x00020000);
    int woff[NT], soff[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int nt = min(nt0 + t, ntiles - 1);
        woff[t]      = (nt * 64 * WV + lane) * 16;
        soff[t]      = (nt * 16 + i16) * 4;
    }
    const int wstride = ntiles * 1024 * WV;  // bytes per k-block of packed weights
    const int sstride = ntiles * 64;         // bytes per k-block of scale words

    floatx4 acc[NT][MT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            acc[t][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
    }

    u32x4    ring[PF][NT][WV];
    uint32_t sring[PF][NT];
    u32x4    xs[PF][XR];

    // x chunk q of a stage: row q / 16, 16-B chunk q % 16.  Loads are unconditional (clamped); rows past Mloc only feed output rows
    // that are never stored.
    int xoff[XR];
    int xlds[XR];
#pragma unroll
    for (int r = 0; r < XR; ++r) {
        const int q  = tid + THREADS * r;
        const int qc = min(q, NCHUNK - 1);
        const int m  = qc >> 4;
        const int ci = qc & 15;
        int       xrow = row0 + min(m0 + m, Mloc - 1);
        if (p.row_idx) {
            xrow = p.row_idx[xrow];
        }
        xoff[r] = (xrow * p.ldx + ci * 8) * 2;
        xlds[r] = q < NCHUNK ? m * ROWB + ((ci ^ (m & 15)) << 4) : -1;
    }
    const int last = nit - 1;  // iteration indices are clamped to `last`: the ring tail re-loads harmlessly

#define TM_LOAD_W(slot, i)                                                                                            \
    {                                                                                                                 \
        const int kb_ = min((i), last);                                                                               \
        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                                \
        {                                                                                                             \
            _Pragma("unroll") for (int v = 0; v < WV; ++v)                                                            \
            {                                                                                                         \
                ring[slot][t][v] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, woff[t] + v * 1024, kb_ * wstride, 2); \
            }                                                                                                         \
            if constexpr (WT == 3) {                                                                                  \
                sring[slot][t] = __builtin_amdgcn_raw_buffer_load_b32(rs_s, soff[t], kb_ * sstride, 0);               \
            }                                                                                                         \
        }                                                                                                             \
    }
#define TM_LOAD_X(set, i)                                                                             \
    {                                                                                                 \
        const int kb_ = min((i), last);                                                               \
        _Pragma("unroll") for (int r = 0; r < XR; ++r)                                                \
        {                                                                                             \
            xs[set][r] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xoff[r], kb_ * 256, 0);          \
        }                                                                                             \
    }
#define TM_STORE_X(set, buf)                                        \
    _Pragma("unroll") for (int r = 0; r < XR; ++r)                  \
    {                                                               \
        if (XFULL || xlds[r] >= 0) {                                \
            *(u32x4*)(smem + (buf)*BUFB + xlds[r]) = xs[set][r];    \
        }                                                           \
    }

    // VMEM loads return in order: x(i) is issued right before w(i), PF iterations ahead of its use (see gemm_kernel)
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        TM_LOAD_X(u, u);
        TM_LOAD_W(u, u);
        __builtin_amdgcn_sched_barrier(0);  // pin the issue order: the loop's waits then never drain the whole ring
    }
    TM_STORE_X(0, 0);
    __syncthreads();

    // iterations past nit (ring padding) contract zeroed weights, so they add exactly 0
    auto dq = [&](int slot, int t, int j, bool live) -> half8_t {
        if constexpr (WT == 3) {
            return mx_dequant8(ring[slot][t][0][j], sring[slot][t] & (live ? ~0u : 0u), j);  // scale bytes 0 -> w = +-0
        }
        else {
            const u32x4 wv = ring[slot][t][j];
            return bit_cast<half8_t>(live ? wv : u32x4{0u, 0u, 0u, 0u});
        }
    };
    auto ldx = [&](const char* stage, int j, int mt) -> half8_t {
        return *(const half8_t*)(stage + (mt * 16 + i16) * ROWB + (((j * 4 + g) ^ i16) << 4));
    };
    half8_t wfn[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        wfn[t] = dq(0, t, 0, true);
    }
    for (int base = 0; base < nit; base += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int   i         = base + u;
            const bool  live      = i < nit;  // wave-uniform
            const bool  live_next = i + 1 < nit;
            const char* stage     = smem + (u & 1) * BUFB;
            half8_t     xf[MT], xfn[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                xf[mt] = ldx(stage, 0, mt);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // 32-k steps of this k-block
                half8_t wf[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    wf[t] = wfn[t];
                }
                // produce the next step (or step 0 of the next iteration) while the MFMAs below are in flight
                if (j + 1 < 4) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        wfn[t] = dq(u, t, j + 1, live);
                    }
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        xfn[mt] = ldx(stage, j + 1, mt);
                    }
                }
                else {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        wfn[t] = dq((u + 1) % PF, t, 0, live_next);
                    }
                }
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[t], xf[mt], acc[t][mt], 0, 0, 0);
                    }
                }
                if (j + 1 < 4) {
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        xf[mt] = xfn[mt];
                    }
                }
            }
            TM_STORE_X((u + 1) % PF, (u + 1) & 1);  // x(i+1), issued PF-1 iterations ago, -> the other LDS stage
            TM_LOAD_X(u, i + PF);                   // refill slot u: x first, then w
            TM_LOAD_W(u, i + PF);
            __syncthreads();
        }
    }
#undef TM_LOAD_W
#undef TM_LOAD_X
#undef TM_STORE_X

    // ---- epilogue: lane holds y[m = m0+16mt+i16][n = 16(nt0+t) + 4g + r], r = 0..3 ------------------
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (nt0 + t >= ntiles) {
            continue;
        }
        const int n = (nt0 + t) * 16 + g * 4;
        half4_t   b = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
        if (p.epilogue == 3 && p.bias) {
            b = *(const half4_t*)(p.bias + (size_t)e * p.N + n);
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (m0 + mt * 16 + i16 >= Mloc) {
                continue;
            }
            const int     m = row0 + m0 + mt * 16 + i16;  // flat output row
            const floatx4 a = acc[t][mt];
            if (p.epilogue == 3) {
                // columns (2j, 2j+1) = (gate_j, up_j): the reference's unfused order of roundings -- the GEMM's fp16 output, the fp16 bias
                // add, the clamps, then gate * sigmoid(1.702 gate) * (1 + up) in fp32
                half4_t v = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3]};
                if (p.bias) {
                    v = v + b;
                }
                const float g0 = __builtin_fminf((float)v[0], 7.0f), g1 = __builtin_fminf((float)v[2], 7.0f);
                const float u0 = __builtin_fmaxf(-7.0f, __builtin_fminf((float)v[1], 7.0f));
                const float u1 = __builtin_fmaxf(-7.0f, __builtin_fminf((float)v[3], 7.0f));
                const float o0 = g0 / (1.0f + __builtin_expf(-1.702f * g0)) * (1.0f + u0);
                const float o1 = g1 / (1.0f + __builtin_expf(-1.702f * g1)) * (1.0f + u1);
                half2_t     o  = {(half_t)o0, (half_t)o1};
                *(half2_t*)(p.y + (size_t)m * p.ldy + (n >> 1)) = o;
            }
            else if (p.epilogue == 1) {
                const float s0 = a[0] / (1.0f + __builtin_expf(-a[0]));
                const float s1 = a[2] / (1.0f + __builtin_expf(-a[2]));
                half2_t     o  = {(half_t)(s0 * a[1]), (half_t)(s1 * a[3])};
                *(half2_t*)(p.y + (size_t)m * p.ldy + (n >> 1)) = o;
            }
            else {
                half4_t o = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3]};
                *(half4_t*)(p.y + (size_t)m * p.ldy + n) = o;
            }
        }
    }
}

template<int WT, int MT, int NT, int WN, int PF>
static int launch_mx(const MxParams& p, dim3 grid, hipStream_t st)
{
    constexpr int lds_need = 2 * 16 * MT * 256;
    // a grid of <= 256 eight-wave workgroups must land one per CU (launch_one, gemm_w4a16.hip): ask for more than half of the LDS
    const int lds = (WN >= 8 && grid.x * grid.y * grid.z <= 256) ? 84 * 1024 : lds_need;
    if (const int rc = ensure_dynamic_lds((const void*)gemm_mx_kernel<WT, MT, NT, WN, PF>, 84 * 1024)) {
        return rc;
    }
    gemm_mx_kernel<WT, MT, NT, WN, PF><<<grid, WN * 64, lds, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// launch_linear_grouped's arm for MXFP4 experts (every epilogue) and for fp16 experts with the gpt-oss epilogue; same tile choice:
// this thread's override, then the measured table (kind kGenGrouped + type), then twice the expected rows per expert
int launch_linear_grouped_mx(const LinearWeight& proto, const void* d_groups, int E, const half_t* x, int ldx, int x_rows, half_t* y,
                             int ldy, int m_cap, int m_hint, int epilogue, const half_t* bias, const int* seg, const int* row_idx,
                             hipStream_t st)
{
    TM_REQUIRE(proto.type == 3 || (proto.type == 1 && epilogue == 3),
               "grouped GEMM: the gpt-oss activation and expert biases are built for fp16 and MXFP4 experts only");
    TM_REQUIRE(epilogue == 0 || epilogue == 1 || epilogue == 3, "grouped GEMM: epilogue");
    TM_REQUIRE(ldx % 8 == 0 && (epilogue == 0 || proto.N % 32 == 0) && proto.K % 128 == 0 && proto.N % 16 == 0, "grouped GEMM: alignment");
    TM_REQUIRE(bias == nullptr || epilogue == 3, "grouped GEMM: a bias goes with the gpt-oss epilogue");
    if (m_cap == 0 || E == 0) {
        return 0;
    }
    MxParams p{};
    p.x        = x;
    p.ldx      = ldx;
    p.y        = y;
    p.ldy      = ldy;
    p.M        = m_cap;
    p.N        = proto.N;
    p.K        = proto.K;
    p.KB       = proto.K / 128;
    p.epilogue = epilogue;
    p.groups   = (const MxGroup*)d_groups;
    p.seg      = seg;
    p.row_idx  = row_idx;
    p.x_rows   = x_rows;
    p.bias     = bias;
    const int  ntiles = proto.N / 16;
    const bool mx     = proto.type == 3;
    if (m_cap <= 64) {
        const int want = std::min(m_cap, std::max(1, 2 * m_hint));
        int       mt   = want <= 16 ? 1 : (want <= 32 ? 2 : 4);
        int       tv[4];
        if (const int forced = gen_grouped_rows_forced(proto.K, proto.N)) {
            mt = forced / 16;
        }
        else if (gen_table_get(kGenGrouped + proto.type, 0, proto.K, proto.N, dec32_m_bucket(m_cap), tv)) {
            mt = tv[0] / 16;
        }
        p.zper = (m_cap + 16 * mt - 1) / (16 * mt);
        TM_REQUIRE((int64_t)E * p.zper <= 65535, "grouped linear: experts x row blocks exceed grid.z (65535): split the forward into fewer tokens");
        // MXFP4: 8 waves of one column tile each (the u4 form); fp16: 4 waves
        dim3 grid(mx ? (ntiles + 7) / 8 : (ntiles + 3) / 4, 1, E * p.zper);
        if (mx) {
            return mt == 1 ? launch_mx<3, 1, 1, 8, 4>(p, grid, st) : mt == 2 ? launch_mx<3, 2, 1, 8, 4>(p, grid, st) : launch_mx<3, 4, 1, 8, 4>(p, grid, st);
        }
        return mt == 1 ? launch_mx<1, 1, 1, 4, 4>(p, grid, st) : mt == 2 ? launch_mx<1, 2, 1, 4, 4>(p, grid, st) : launch_mx<1, 4, 1, 4, 4>(p, grid, st);
    }
    // prefill: 64-row blocks x 2 tiles per wave; blocks past an expert's segment exit at once
    p.zper = (m_cap + 63) / 64;
    TM_REQUIRE((int64_t)E * p.zper <= 65535, "grouped linear: experts x row blocks exceed grid.z (65535): split the forward into fewer tokens");
    dim3 grid(mx ? (ntiles + 15) / 16 : (ntiles + 7) / 8, 1, E * p.zper);
    return mx ? launch_mx<3, 4, 2, 8, 4>(p, grid, st) : launch_mx<1, 4, 2, 4, 2>(p, grid, st);
}

}  // namespace tmk
