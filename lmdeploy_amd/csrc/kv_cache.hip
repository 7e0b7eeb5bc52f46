// Paged KV cache: fused RoPE + online int8/int4 quantise-and-store, and dequantising flatten.
//
// Replaces: invokeProcessKV_v2_ / invokeFlattenKV_v2_ (src/turbomind/kernels/attention/kv_cache_utils_v2.cu
//           :18-210,340-468), the decode kernel's store prologue (attention_universal.h:273-330),
//           the quantiser (quantization.h:316-366,428-489) and FastRoPE (rotary_embedding.h:54-194).
//
// Integer contract (bit exact): per (token, kv head), K (after RoPE) and V separately
//   mn = min x, mx = max x; scale = h((f32(mx)-f32(mn)) * (1/(2^b-1))); zero = mn;
//   inv = h(1/f32(scale)); q = sat_u8(rne(h(h(x-zero)*inv))); b==4: min(q,15), nibbles [0,2,4,6,1,3,5,7].
// Byte layout of a block: kernels/attention/block.h:126-219 (KvLayout in tm_kernels.h).
// KV bits 42 (TurboQuant: Hadamard rotation, K 4-bit / V 2-bit Lloyd-Max codes, fp16 norms) has a contract of its own, stated in
// turboquant.h; both kernels below carry an `if constexpr` arm for it on the same lane mapping (head_dim 128 only).
//
// Work mapping: D/8 lanes own one D-wide head row (8 halves = 16 B each, one coalesced row): 16 lanes (256 B) at head_dim 128,
// 8 lanes (128 B) at head_dim 64; min/max are wave-level DPP reductions inside that lane row -- no LDS.  HBM-bound byte work.
// Both kernels are templated on D (64 | 128): the 8-lane row reduces with xor1, xor2, half-mirror only (the row_ror:8 step of the
// 16-lane row would mix two tokens), a 256-thread workgroup holds 2048 / D token rows.
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
    static_assert(sizeof...(M) == (MROPE ? 4 : 0), "MROPE: (const int* mrope_pos, const int* pos_delta, int sec_t, int sec_th)");
    static_assert(!MROPE || (!SEQ && D == 128 && BITS != kTqBits), "MROPE: one table, head_dim 128, KV bits 16 / 8 / 4");
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
    else {
        doff = is_k ? L.k_data(kv_head, ti) : L.v_data(kv_head, ti);
    }

    if constexpr (BITS == 16) {
        *(half8_t*)(block + doff + lane16 * 16) = x;
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

int launch_kv_rope_store(half_t*        qkv,
                         int            q_heads,
                         const int*     cu_q_len,
                         const int*     k_len,
                         int            batch,
                         int            total_tokens,
                         const half2_t* cos_sin,
                         int            max_pos,
                         KvCacheView    cache,
                         hipStream_t    st,
                         const half_t*  qkv_bias,
                         const half_t*  q_norm,
                         const half_t*  k_norm,
                         float          qk_eps,
                         const int*     rope_row0)
{
    const int hd = cache.layout.head_dim;
    TM_REQUIRE(hd == 64 || hd == 128, "kv_rope_store: head_dim must be 64 or 128");
    TM_REQUIRE(hd == 128 || (q_norm == nullptr && k_norm == nullptr), "kv_rope_store: q/k RMSNorm (qk_norm) needs head_dim 128");
    TM_REQUIRE(rope_row0 == nullptr || cos_sin != nullptr, "rope_row0 needs a table");
    const int kvb = cache.layout.bits;
    TM_REQUIRE(kvb == 16 || kvb == 8 || kvb == 4 || kvb == kTqBits, "kv bits in {16,8,4,42}");
    TM_REQUIRE(kvb != kTqBits || hd == 128, "kv_rope_store: kv bits 42 (TurboQuant) needs head_dim 128, head_dim 64 is not built");
    TM_REQUIRE((q_norm == nullptr) == (k_norm == nullptr), "q_norm and k_norm come together");
    if (total_tokens == 0) {
        return 0;
    }
    const int  tpw = 2048 / hd;  // token rows per 256-thread workgroup: 16 | 32
    dim3       grid((total_tokens + tpw - 1) / tpw, q_heads + 2 * cache.layout.kv_heads);
    const bool qkx = qkv_bias != nullptr || q_norm != nullptr;
#define TM_KV_STORE_D(B_, X_, S_, D_)                                                                                             \
    kv_rope_store_kernel<B_, X_, S_, D_><<<grid, 256, 0, st>>>(qkv, q_heads, cu_q_len, k_len, batch, total_tokens, cos_sin, max_pos, \
                                                               cache, qkv_bias, q_norm, k_norm, qk_eps, rope_row0)
#define TM_KV_STORE(B_, X_)                                                                                                       \
    do {                                                                                                                          \
        if (hd == 64) {                                                                                                           \
            if (rope_row0 != nullptr) TM_KV_STORE_D(B_, X_, true, 64);                                                            \
            else TM_KV_STORE_D(B_, X_, false, 64);                                                                                \
        }                                                                                                                         \
        else if (rope_row0 != nullptr) {                                                                                          \
            TM_KV_STORE_D(B_, X_, true, 128);                                                                                     \
        }                                                                                                                         \
        else {                                                                                                                    \
            TM_KV_STORE_D(B_, X_, false, 128);                                                                                    \
        }                                                                                                                         \
    } while (0)
    switch (cache.layout.bits) {
        case 16:
            if (qkx) TM_KV_STORE(16, true);
            else TM_KV_STORE(16, false);
            break;
        case 8:
            if (qkx) TM_KV_STORE(8, true);
            else TM_KV_STORE(8, false);
            break;
        case kTqBits:  // head_dim 128 only (checked above)
            if (qkx) {
                if (rope_row0 != nullptr) TM_KV_STORE_D(kTqBits, true, true, 128);
                else TM_KV_STORE_D(kTqBits, true, false, 128);
            }
            else if (rope_row0 != nullptr) {
                TM_KV_STORE_D(kTqBits, false, true, 128);
            }
            else {
                TM_KV_STORE_D(kTqBits, false, false, 128);
            }
            break;
        default:
            if (qkx) TM_KV_STORE(4, true);
            else TM_KV_STORE(4, false);
    }
#undef TM_KV_STORE
#undef TM_KV_STORE_D
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// launch_kv_rope_store with M-RoPE sections (kv_rope_store_kernel<.., MROPE = true>): one shared table, head_dim 128, KV bits 16 / 8 / 4.
// No rope_row0: per-sequence tables (dynamic NTK) and sections do not meet -- tm_engine_set_mrope_section refuses rope_type 4.
int launch_kv_rope_store_mrope(half_t*        qkv,
                               int            q_heads,
                               const int*     cu_q_len,
                               const int*     k_len,
                               int            batch,
                               int            total_tokens,
                               const half2_t* cos_sin,
                               int            max_pos,
                               const int*     mrope_pos,
                               const int*     pos_delta,
                               int            sec_t,
                               int            sec_h,
                               int            sec_w,
                               KvCacheView    cache,
                               hipStream_t    st,
                               const half_t*  qkv_bias,
                               const half_t*  q_norm,
                               const half_t*  k_norm,
                               float          qk_eps)
{
    const int hd  = cache.layout.head_dim;
    const int kvb = cache.layout.bits;
    TM_REQUIRE(kvb != kTqBits, "kv_rope_store: M-RoPE with kv bits 42 (TurboQuant) is not built");
    TM_REQUIRE(hd != 64, "kv_rope_store: M-RoPE with head_dim 64 is not built (head_dim must be 128)");
    TM_REQUIRE(hd == 128, "kv_rope_store: M-RoPE needs head_dim 128");
    TM_REQUIRE(kvb == 16 || kvb == 8 || kvb == 4, "kv_rope_store: M-RoPE serves kv bits 16 / 8 / 4");
    TM_REQUIRE(cos_sin != nullptr && max_pos >= 1, "kv_rope_store: M-RoPE needs a table");
    TM_REQUIRE(sec_t >= 0 && sec_h >= 0 && sec_w >= 0 && sec_t + sec_h + sec_w == hd / 2,
               "kv_rope_store: mrope sections must be three non-negative sizes that sum to head_dim / 2");
    TM_REQUIRE((q_norm == nullptr) == (k_norm == nullptr), "q_norm and k_norm come together");
    if (total_tokens == 0) {
        return 0;
    }
    dim3       grid((total_tokens + 15) / 16, q_heads + 2 * cache.layout.kv_heads);
    const bool qkx    = qkv_bias != nullptr || q_norm != nullptr;
    const int  sec_th = sec_t + sec_h;
#define TM_KV_STORE_M(B_, X_)                                                                                                     \
    kv_rope_store_kernel<B_, X_, false, 128, true><<<grid, 256, 0, st>>>(qkv, q_heads, cu_q_len, k_len, batch, total_tokens, cos_sin, \
                                                                         max_pos, cache, qkv_bias, q_norm, k_norm, qk_eps, nullptr,    \
                                                                         mrope_pos, pos_delta, sec_t, sec_th)
    switch (kvb) {
        case 16:
            if (qkx) TM_KV_STORE_M(16, true);
            else TM_KV_STORE_M(16, false);
            break;
        case 8:
            if (qkx) TM_KV_STORE_M(8, true);
            else TM_KV_STORE_M(8, false);
            break;
        default:
            if (qkx) TM_KV_STORE_M(4, true);
            else TM_KV_STORE_M(4, false);
    }
#undef TM_KV_STORE_M
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------
// (cos, sin) table on the device: the table of tm_rope_table_ex for inverse frequencies the host computed by the shared recipe.
// One thread = one (position, pair): angle = one fp32 product, cos / sin in double of that fp32 value, rounded fp32 (x the YaRN
// attention factor, in fp32) -> fp16; one half2 store per thread, consecutive threads consecutive pairs.  Runs once per admission of a
// sequence that takes a base of its own (dynamic NTK), on the engine stream.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rope_table_kernel(half2_t* __restrict__ out, int64_t entries, int pairs, RopeInvFreq f)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= entries) {
        return;
    }
    const int   t   = (int)(idx / pairs);
    const int   i   = (int)(idx - (int64_t)t * pairs);
    const float ang = (float)t * f.inv[i];
    const float c   = (float)cos((double)ang) * f.attention_factor;  // a factor of 1 is exact
    const float s   = (float)sin((double)ang) * f.attention_factor;
    half2_t     o   = {(half_t)c, (half_t)s};
    out[idx]  = o;
}

int launch_rope_table(half2_t* out, int max_pos, int dim, const RopeInvFreq& f, hipStream_t st)
{
    TM_REQUIRE(out != nullptr && max_pos >= 1, "rope table: null pointer / max_pos");
    TM_REQUIRE(dim > 0 && dim % 2 == 0 && dim / 2 <= kRopeMaxPairs, "rope dim: even, at most 128");
    const int64_t entries = (int64_t)max_pos * (dim / 2);
    rope_table_kernel<<<(unsigned)((entries + 255) / 256), 256, 0, st>>>(out, entries, dim / 2, f);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
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
template<int BITS, bool VT, int D = 128, bool WIN = false, typename... W>
__global__ __launch_bounds__(256) void flatten_kv_kernel(half_t* __restrict__ k_out,
                                                         half_t* __restrict__ v_out,
                                                         const int* __restrict__ cu_k_off,
                                                         const int* __restrict__ k_len,
                                                         int         k_stride,
                                                         KvCacheView cache,
                                                         W... win)
{
    static_assert(sizeof...(W) == (WIN ? 2 : 0), "WIN: (const int* cu_q_len, int window)");
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
        const auto [cu_q_len, window] = std::tuple<const int*, int>(win...);
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

template<bool WIN>
static int launch_flatten_kv_impl(half_t*     k_out,
                                  half_t*     v_out,
                                  int         transpose_v,
                                  const int*  cu_k_off,
                                  const int*  k_len,
                                  int         batch,
                                  int         max_k_len,
                                  int         k_stride,
                                  KvCacheView cache,
                                  const int*  cu_q_len,
                                  int         window,
                                  hipStream_t st)
{
    const int hd = cache.layout.head_dim;
    TM_REQUIRE(hd == 64 || hd == 128, "flatten_kv: head_dim must be 64 or 128");
    TM_REQUIRE(cache.layout.block_len == 64, "block_len must be 64");
    TM_REQUIRE(!transpose_v || k_stride % 64 == 0, "transposed V needs a 64-aligned k_stride");
    if (batch == 0 || max_k_len == 0) {
        return 0;
    }
    dim3 grid((max_k_len + 63) / 64, cache.layout.kv_heads, batch);
#define TM_FLATTEN_D(B_, T_, D_)                                                                                                    \
    do {                                                                                                                            \
        if constexpr (WIN)                                                                                                          \
            flatten_kv_kernel<B_, T_, D_, true><<<grid, 256, 0, st>>>(k_out, v_out, cu_k_off, k_len, k_stride, cache, cu_q_len, window); \
        else                                                                                                                        \
            flatten_kv_kernel<B_, T_, D_><<<grid, 256, 0, st>>>(k_out, v_out, cu_k_off, k_len, k_stride, cache);                     \
    } while (0)
#define TM_FLATTEN(B_, T_)                      \
    do {                                        \
        if (hd == 64) TM_FLATTEN_D(B_, T_, 64); \
        else TM_FLATTEN_D(B_, T_, 128);         \
    } while (0)
    const int bits = cache.layout.bits;
    TM_REQUIRE(bits == 16 || bits == 8 || bits == 4 || bits == kTqBits, "kv bits in {16,8,4,42}");
    if (bits == kTqBits) {
        TM_REQUIRE(hd == 128, "flatten_kv: kv bits 42 (TurboQuant) needs head_dim 128, head_dim 64 is not built");
        TM_REQUIRE(!WIN, "flatten_kv: kv bits 42 (TurboQuant) with a sliding window is not built (window must be 0)");
        if constexpr (!WIN) {
            if (transpose_v) TM_FLATTEN_D(kTqBits, true, 128);
            else TM_FLATTEN_D(kTqBits, false, 128);
        }
        TM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    if (transpose_v) {
        if (bits == 16) TM_FLATTEN(16, true);
        else if (bits == 8) TM_FLATTEN(8, true);
        else TM_FLATTEN(4, true);
    }
    else {
        if (bits == 16) TM_FLATTEN(16, false);
        else if (bits == 8) TM_FLATTEN(8, false);
        else TM_FLATTEN(4, false);
    }
#undef TM_FLATTEN
#undef TM_FLATTEN_D
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_flatten_kv(half_t*     k_out,
                      half_t*     v_out,
                      int         transpose_v,
                      const int*  cu_k_off,
                      const int*  k_len,
                      int         batch,
                      int         max_k_len,
                      int         k_stride,
                      KvCacheView cache,
                      hipStream_t st)
{
    return launch_flatten_kv_impl<false>(k_out, v_out, transpose_v, cu_k_off, k_len, batch, max_k_len, k_stride, cache, nullptr, 0, st);
}

// flatten for a layer with a sliding window: tiles wholly in front of max(k_len - q_len - window + 1, 0) are neither read nor
// written (flatten_kv_kernel<.., WIN = true>); window == 0 is launch_flatten_kv, launch for launch
int launch_flatten_kv_window(half_t*     k_out,
                             half_t*     v_out,
                             int         transpose_v,
                             const int*  cu_k_off,
                             const int*  k_len,
                             const int*  cu_q_len,
                             int         window,
                             int         batch,
                             int         max_k_len,
                             int         k_stride,
                             KvCacheView cache,
                             hipStream_t st)
{
    TM_REQUIRE(window >= 0, "flatten_kv: window must be >= 0 (0 = the whole context)");
    if (window == 0) {
        return launch_flatten_kv(k_out, v_out, transpose_v, cu_k_off, k_len, batch, max_k_len, k_stride, cache, st);
    }
    TM_REQUIRE(cu_q_len, "flatten_kv: a window needs cu_q_len");
    return launch_flatten_kv_impl<true>(k_out, v_out, transpose_v, cu_k_off, k_len, batch, max_k_len, k_stride, cache, cu_q_len, window, st);
}

}  // namespace tmk
