// Device side of kv_cache.hip: the RoPE + quantise-and-store kernel and the dequantising flatten kernel, as templates.  In a header so that
// the FP8 instantiations can live in a translation unit of their own (kv_cache_fp8.hip), built without packed fp32 instructions, while
// kv_cache.hip keeps instantiating -- and building -- the 16 / 8 / 4 / 42 kernels exactly as before.
#pragma once
#include "tm_common.h"
#include "tm_kernels.h"
#include "turboquant.h"
#include <tuple>

namespace tmk {

__device__ __forceinline__ int find_seq(const int* cu, int batch, int token)
{
    // largest b with cu[b] <= token   (cu has batch+1 entries, cu[0] = 0)
    int lo = 0, hi = batch;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cu[mid] <= token) {
            lo = mid;
        }
        else {
            hi = mid;
        }
    }
    return lo;
}

// max over the LPR (8 | 16) lanes of one head row
template<int LPR>
__device__ __forceinline__ float row_max(float v)
{
    static_assert(LPR == 8 || LPR == 16, "head rows of 8 or 16 lanes");
    v = fmaxf(v, dpp_f32<DPP_XOR1>(v));
    v = fmaxf(v, dpp_f32<DPP_XOR2>(v));
    v = fmaxf(v, dpp_f32<DPP_HMIRR>(v));
    if constexpr (LPR == 16) {
        v = fmaxf(v, dpp_f32<DPP_ROR8>(v));
    }
    return v;
}

// 8 halves -> 8 e4m3fn code bytes of the FP8 cache: cvt_pk_fp8_f32(clamp(f32(x) / scale, -448, 448)), the IEEE fp32 division, RNE.
// The one quantiser of every FP8 store (kv_rope_store_kernel below, the MLA latent store of attention_mla_fp8.hip).
__device__ __forceinline__ u32x2 f8_quant8(half8_t x, float scale)
{
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        y[e] = fminf(fmaxf((float)x[e] / scale, -448.0f), 448.0f);
    }
    u32x2 w;
    w[0] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
    w[0] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], (int)w[0], true);
    w[1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
    w[1] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], (int)w[1], true);
    return w;
}

// QKX: the Qwen prologue (per-head RMSNorm of q / k, then the q / k / v bias; either may be nullptr) in front of RoPE.
// One 16-lane row holds one 128-wide head of one token, so the head's sum of squares is a row DPP reduction like row_max.  The norm
// exists at D = 128 only (head_norm8 fixes 1/128 and the 16-partial tree); the launcher refuses it at D = 64, the bias works there.
// SEQ: per-sequence RoPE tables (dynamic NTK) -- sequence b reads the rows [rope_row0[b], rope_row0[b] + max_pos) of cos_sin; the
// position is clamped first, so a position past the end stays inside the sequence's own region.  Without SEQ rope_row0 is not read.
// MROPE: multimodal RoPE in sections (Qwen2-VL; the reference's kChunked mode, rotary_embedding.h:112-193).  Frequency pair j of a head
// takes its table row from one of three coordinates: t for j < sec_t, h for j < sec_th = sec_t + sec_h, w behind; the row is
// clamp(c, 0, max_pos - 1), the (cos, sin) is entry j of that row, the rotation is the one below.  mrope_pos [total_tokens][3] holds
// the coordinates of this launch's rows; nullptr: every row's three coordinates are its linear position + pos_delta[b] (decode, and
// pos_delta == nullptr is a delta of 0).  The K/V row still lands at the LINEAR position.  A lane owns pairs [4 lane, 4 lane + 4):
// when they lie in one section (always, for boundaries that are multiples of 4) it reads one 16-byte vector as the plain arm does,
// a lane that straddles a boundary reads its four pairs one by one.  The variant's arguments are the pack M, empty without MROPE:
// those instantiations keep the kernel arguments they had before the variant existed.
template<int BITS, bool QKX, bool SEQ = false, int D = 128, bool MROPE = false, typename... M>
__global__ __launch_bounds__(256) void kv_rope_store_kernel(half_t* __restrict__ qkv,
                                                            int q_heads,
                                                            const int* __restrict__ cu_q_len,
                                                            const int* __restrict__ k_len,
                                                            int batch,
                                                            int total_tokens,
                                                            const half2_t* __restrict__ cos_sin,
                                                            int         max_pos,
                                                            KvCacheView cache,
                                                            const half_t* __restrict__ qkv_bias,
                                                            const half_t* __restrict__ q_norm,
                                                            const half_t* __restrict__ k_norm,
                                                            float qk_eps,
                                                            const int* __restrict__ rope_row0,
                                                            M... mr)
{
    static_assert(D == 64 || D == 128, "head_dim 64 or 128");
    static_assert(sizeof...(M) == (MROPE ? 4 : BITS == kKvBitsFp8 ? 2 : 0),
                  "MROPE: (const int* mrope_pos, const int* pos_delta, int sec_t, int sec_th); FP8: (float k_scale, float v_scale)");
    static_assert(!MROPE || (!SEQ && D == 128 && BITS != kTqBits && BITS != kKvBitsFp8), "MROPE: one table, head_dim 128, KV bits 16 / 8 / 4");
    constexpr int  LPR     = D / 8;  // lanes per head row
    const KvLayout L       = cache.layout;
    const int      lane16  = threadIdx.x & (LPR - 1);  // lane inside the head row (0..7 at D = 64)
    const int      token   = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int      head    = blockIdx.y;  // [0,Hq): q   [Hq,Hq+Hkv): k   [Hq+Hkv, Hq+2Hkv): v
    const int      kv_heads = L.kv_heads;
    if (token >= total_tokens) {
        return;  // whole head rows (LPR lanes, one token) exit together; the DPP reductions stay inside a head row
    }
    const int stride = (q_heads + 2 * kv_heads) * D;
    half_t*   src    = qkv + (size_t)token * stride + (size_t)head * D + lane16 * 8;
    half8_t   x      = *(const half8_t*)src;

    const int b       = find_seq(cu_q_len, batch, token);
    const int q_len   = cu_q_len[b + 1] - cu_q_len[b];
    const int history = k_len[b] - q_len;
    const int pos     = history + (token - cu_q_len[b]);

    const bool is_q = head < q_heads;
    const bool is_k = !is_q && head < q_heads + kv_heads;

    if constexpr (QKX) {
        if constexpr (D == 128) {
            if (q_norm != nullptr) {  // grid-uniform; V rows reduce too (whole rows stay in step) and keep x
                const float   ss = group_sum<16>(sumsq8(x));
                const half8_t w  = *(const half8_t*)((is_q ? q_norm : k_norm) + lane16 * 8);
                if (is_q || is_k) {
                    x = head_norm8(x, ss, w, qk_eps);
                }
            }
        }
        if (qkv_bias != nullptr) {
            x = x + *(const half8_t*)(qkv_bias + (size_t)head * D + lane16 * 8);
        }
    }

    if ((is_q || is_k) && cos_sin != nullptr) {
        // interleaved pairs (x[2i], x[2i+1]); c,s already cast to fp16; fp16 mul/sub/add, no fma
        const int     p  = pos < max_pos ? pos : max_pos - 1;
        size_t        row = (size_t)p;
        if constexpr (SEQ) {
            row += (size_t)rope_row0[b];  // 64-bit: max_batch x (session_len + 1) rows of 2 D bytes pass 2 GiB
        }
        half8_t       cs;
        if constexpr (MROPE) {
            const auto mt        = std::tuple<const int*, const int*, int, int>(mr...);
            const int* mrope_pos = std::get<0>(mt);
            const int* pos_delta = std::get<1>(mt);
            const int  sec_t = std::get<2>(mt), sec_th = std::get<3>(mt);
            int c[3];
            if (mrope_pos != nullptr) {  // grid-uniform
                c[0] = mrope_pos[(size_t)token * 3];
                c[1] = mrope_pos[(size_t)token * 3 + 1];
                c[2] = mrope_pos[(size_t)token * 3 + 2];
            }
            else {
                c[0] = c[1] = c[2] = pos + (pos_delta != nullptr ? pos_delta[b] : 0);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                c[a] = c[a] < 0 ? 0 : (c[a] < max_pos ? c[a] : max_pos - 1);
            }
            const int  j0   = lane16 * 4;  // this lane's first frequency pair
            const auto axis = [&](int j) { return j < sec_t ? 0 : (j < sec_th ? 1 : 2); };
            const int  a0   = axis(j0);
            if (a0 == axis(j0 + 3)) {
                const int r = a0 == 0 ? c[0] : (a0 == 1 ? c[1] : c[2]);
                cs          = *(const half8_t*)(cos_sin + (size_t)r * (D / 2) + j0);
            }
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int     ai = axis(j0 + i);
                    const int     r  = ai == 0 ? c[0] : (ai == 1 ? c[1] : c[2]);
                    const half2_t e  = cos_sin[(size_t)r * (D / 2) + j0 + i];
                    cs[2 * i]        = e[0];
                    cs[2 * i + 1]    = e[1];
                }
            }
        }
        else {
            cs = *(const half8_t*)(cos_sin + row * (D / 2) + lane16 * 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const half_t c  = cs[2 * i];
            const half_t s  = cs[2 * i + 1];
            const half_t x0 = x[2 * i];
            const half_t x1 = x[2 * i + 1];
            const half_t a0 = c * x0;
            const half_t a1 = s * x1;
            const half_t b0 = c * x1;
            const half_t b1 = s * x0;
            x[2 * i]        = a0 - a1;
            x[2 * i + 1]    = b0 + b1;
        }
    }
    if (is_q) {
        *(half8_t*)src = x;
        return;
    }

    const int kv_head = is_k ? head - q_heads : head - q_heads - kv_heads;
    const int blk     = pos / L.block_len;
    const int ti      = pos - blk * L.block_len;
    char*     block   = (char*)cache.block_ptrs[cache.cu_block_nums[b] + blk] + cache.layer_offset;
    int       doff;
    if constexpr (BITS == kTqBits) {
        doff = is_k ? L.tq_k_data(kv_head, ti) : L.tq_v_data(kv_head, ti);
    }
    else if constexpr (BITS == kKvBitsFp8) {
        doff = is_k ? L.f8_k_data(kv_head, ti) : L.f8_v_data(kv_head, ti);
    }
    else {
        doff = is_k ? L.k_data(kv_head, ti) : L.v_data(kv_head, ti);
    }

    if constexpr (BITS == 16) {
        *(half8_t*)(block + doff + lane16 * 16) = x;
    }
    else if constexpr (BITS == kKvBitsFp8) {
        const auto  sc    = std::tuple<float, float>(mr...);
        const float scale = is_k ? std::get<0>(sc) : std::get<1>(sc);
        *(u32x2*)(block + doff + lane16 * 8) = f8_quant8(x, scale);  // the row's LPR lanes: D consecutive bytes
    }
    else if constexpr (BITS == kTqBits) {
        // TurboQuant (turboquant.h): the row's 16 lanes rotate, code and pack it; whole rows got here together
        static_assert(D == 128, "TurboQuant KV: head_dim 128");
        char* par = block + (is_k ? L.tq_k_param(kv_head, ti) : L.tq_v_param(kv_head, ti));
        if (is_k) {
            tq_store_row<true>(x, lane16, block + doff, par);
        }
        else {
            tq_store_row<false>(x, lane16, block + doff, par);
        }
    }
    else {
        float mx = -INFINITY, mnn = -INFINITY;  // mnn tracks max(-x)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)x[e];
            mx            = fmaxf(mx, f);
            mnn           = fmaxf(mnn, -f);
        }
        mx             = row_max<LPR>(mx);
        mnn            = row_max<LPR>(mnn);
        const float mn = -mnn;
        // fp16 min/max are exact in f32
        const float  inv_q_max = 1.0f / (float)((1 << BITS) - 1);
        const half_t scale     = (half_t)((mx - mn) * inv_q_max);
        const half_t zero      = (half_t)mn;
        const half_t inv       = (half_t)(1.0f / (float)scale);
        uint32_t     q[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const half_t d = x[e] - zero;
            const half_t y = d * inv;
            float        r = __builtin_rintf((float)y);  // RNE
            r              = (r == r) ? r : 0.0f;        // cvt.rni.sat of NaN -> 0
            r              = fminf(fmaxf(r, 0.0f), BITS == 8 ? 255.0f : 15.0f);
            q[e]           = (uint32_t)r;
        }
        if constexpr (BITS == 8) {
            u32x2 w;
            w[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            w[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
            *(u32x2*)(block + doff + lane16 * 8) = w;
        }
        else {
            // nibble i of the word = element [0,2,4,6,1,3,5,7][i]   (quantization.h:459-471)
            const uint32_t w = q[0] | (q[2] << 4) | (q[4] << 8) | (q[6] << 12) | (q[1] << 16) | (q[3] << 20)
                               | (q[5] << 24) | (q[7] << 28);
            *(uint32_t*)(block + doff + lane16 * 4) = w;
        }
        if (lane16 == 0) {
            const int poff = is_k ? L.k_param(kv_head, ti) : L.v_param(kv_head, ti);
            half2_t   pr   = {scale, zero};
            *(half2_t*)(block + poff) = pr;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Flatten: one workgroup = 64 cached tokens (one block) of one (sequence, kv head).
//   K -> k_out[head][cu_k_off[b] + t][D];  V -> v_out[head][...][D] or transposed v_out[head][d][cu_k_off[b]+t]
// Dequant (two roundings, quantization.h:565-573,694-703): h(h(h(q)*scale) + zero).
// ------------------------------------------------------------------------------------------------
template<int BITS>
__device__ __forceinline__ half8_t load_dequant_flatten(const char* data, const char* param, int lane16)
{
    // returns dims [8*lane16, 8*lane16+8) of one token
    if constexpr (BITS == 16) {
        return *(const half8_t*)(data + lane16 * 16);
    }
    else {
        const half2_t pr = *(const half2_t*)param;
        const half_t  s = pr[0], z = pr[1];
        half8_t       o;
        if constexpr (BITS == 8) {
            const u32x2 w = *(const u32x2*)(data + lane16 * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t qv = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
                const half_t   t  = (half_t)(float)qv * s;
                o[e]              = t + z;
            }
        }
        else {
            const uint32_t w = *(const uint32_t*)(data + lane16 * 4);
            constexpr int  nib_of[8] = {0, 4, 1, 5, 2, 6, 3, 7};  // element e sits in nibble nib_of[e]
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const uint32_t qv = (w >> (4 * nib_of[e])) & 0xfu;
                const half_t   t  = (half_t)(float)qv * s;
                o[e]              = t + z;
            }
        }
        return o;
    }
}

// WIN = true: the sliding-window variant (launch_flatten_kv_window).  The prefill kernel behind it starts its key loop at
// kbeg_wg = max(hist + bx * 64 - window + 1, 0) / 64 * 64 (attention_prefill.hip), smallest for query block bx = 0, and stages K
// rows and V^T columns [ks, ks + 64) from there on only: a 64-token tile that ends at or below max(hist - window + 1, 0),
// hist = k_len - q_len, is read by no workgroup.  Such a tile returns here before it loads anything and its part of the scratch is
// left as it was (not zero-filled).  The variant's two arguments (cu_q_len [batch + 1], window) are the pack W, empty for
// WIN = false: those instantiations keep the kernel arguments -- and with them, register for register, the code -- they had before
// the variant existed (an unused or empty trailing argument still moves the kernarg segment and the SGPR count).
// dims [8 lane16, 8 lane16 + 8) of one FP8 token row: f16(f32(code) * scale); f32(code) = f32(the widened half) * 2^8, exact
__device__ __forceinline__ half8_t load_dequant_flatten_f8(const char* data, int lane16, float scale)
{
    const u32x2 w = *(const u32x2*)(data + lane16 * 8);
    half8_t     o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const half2_t c = bit_cast<half2_t>(f8_widen2(w[j >> 1], j & 1));
        o[2 * j]        = (half_t)(((float)c[0] * 256.0f) * scale);
        o[2 * j + 1]    = (half_t)(((float)c[1] * 256.0f) * scale);
    }
    return o;
}

template<int BITS, bool VT, int D = 128, bool WIN = false, typename... W>
__global__ __launch_bounds__(256) void flatten_kv_kernel(half_t* __restrict__ k_out,
                                                         half_t* __restrict__ v_out,
                                                         const int* __restrict__ cu_k_off,
                                                         const int* __restrict__ k_len,
                                                         int         k_stride,
                                                         KvCacheView cache,
                                                         W... win)
{
    static_assert(sizeof...(W) == (WIN ? 2 : 0) + (BITS == kKvBitsFp8 ? 2 : 0), "[FP8: float k_scale, float v_scale,] [WIN: const int* cu_q_len, int window]");
    static_assert(D == 64 || D == 128, "head_dim 64 or 128");
    constexpr int  LPR  = D / 8;      // lanes per token row (as in kv_rope_store_kernel)
    constexpr int  ROWS = 256 / LPR;  // token rows per pass: 16 | 32
    const KvLayout L  = cache.layout;
    const int      b  = blockIdx.z;
    const int      hd = blockIdx.y;
    const int      t0 = blockIdx.x * 64;
    const int      n  = k_len[b];
    if (t0 >= n) {
        return;
    }
    if constexpr (WIN) {
        const auto wt       = std::tuple<W...>(win...);
        const int* cu_q_len = std::get<sizeof...(W) - 2>(wt);
        const int  window   = std::get<sizeof...(W) - 1>(wt);
        const int  hist               = n - (cu_q_len[b + 1] - cu_q_len[b]);
        if (t0 + 64 <= max(hist - window + 1, 0)) {
            return;  // workgroup-uniform: in front of every query row's window
        }
    }
    __shared__ half_t vt_smem[VT ? 64 * (D + 8) : 1];

    const int    lane16 = threadIdx.x & (LPR - 1);
    const int    row    = threadIdx.x / LPR;  // ROWS token rows per pass
    const char*  block  = (const char*)cache.block_ptrs[cache.cu_block_nums[b] + blockIdx.x] + cache.layer_offset;
    const size_t obase  = (size_t)hd * k_stride + cu_k_off[b];

#pragma unroll
    for (int pass = 0; pass < 64 / ROWS; ++pass) {
        const int  ti    = pass * ROWS + row;
        const bool valid = t0 + ti < n;
        half8_t    kk = {}, vv = {};
        if (valid) {
            if constexpr (BITS == kTqBits) {  // the 16 lanes of a row share `valid`: the row butterflies run with all of them
                static_assert(D == 128, "TurboQuant KV: head_dim 128");
                kk = tq_flatten_row<true>(block + L.tq_k_data(hd, ti), block + L.tq_k_param(hd, ti), lane16);
                vv = tq_flatten_row<false>(block + L.tq_v_data(hd, ti), block + L.tq_v_param(hd, ti), lane16);
            }
            else if constexpr (BITS == kKvBitsFp8) {
                const auto wt = std::tuple<W...>(win...);
                kk            = load_dequant_flatten_f8(block + L.f8_k_data(hd, ti), lane16, std::get<0>(wt));
                vv            = load_dequant_flatten_f8(block + L.f8_v_data(hd, ti), lane16, std::get<1>(wt));
            }
            else {
                kk = load_dequant_flatten<BITS>(block + L.k_data(hd, ti), block + L.k_param(hd, ti), lane16);
                vv = load_dequant_flatten<BITS>(block + L.v_data(hd, ti), block + L.v_param(hd, ti), lane16);
            }
            *(half8_t*)(k_out + (obase + t0 + ti) * D + lane16 * 8) = kk;
            if constexpr (!VT) {
                *(half8_t*)(v_out + (obase + t0 + ti) * D + lane16 * 8) = vv;
            }
        }
        if constexpr (VT) {
            *(half8_t*)(vt_smem + ti * (D + 8) + lane16 * 8) = vv;  // zeros for invalid tokens
        }
    }
    if constexpr (VT) {
        __syncthreads();
        // thread -> (d = vec & (D - 1), token octets); 64 tokens x D d = 8 D 16-B vectors / 256 thr = D / 32 each
#pragma unroll
        for (int it = 0; it < D / 32; ++it) {
            const int vec = threadIdx.x + it * 256;
            const int d   = vec & (D - 1);
            const int to  = vec / D;  // 0..7 token octet
            half8_t   o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = vt_smem[(to * 8 + e) * (D + 8) + d];
            }
            // transposed layout: [head][d][k_stride]; padded tail tokens (>= n) are written as zeros,
            // the per-sequence region is 64-aligned by contract so this never spills into a neighbour
            *(half8_t*)(v_out + ((size_t)hd * D + d) * k_stride + cu_k_off[b] + t0 + to * 8) = o;
        }
    }
}

}  // namespace tmk
