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
// The FP8 cache (kKvBitsFp8; include/tm_mi355x.h states the contract) is one more arm on that mapping at both head_dims: a lane turns its
// 8 halves into 8 e4m3 bytes -- code = cvt_pk_fp8_f32(clamp(f32(x) / scale, -448, 448)), the IEEE fp32 division, RNE, and no NaN code
// because fmaxf / fminf drop a NaN operand -- and stores them as one 8-byte word: a head row leaves as D consecutive bytes.  Flatten
// widens a byte to fp16 exactly (f8_widen2) and rounds f32(code) * scale to fp16 once.  The two scales ride in the kernels' trailing
// argument packs, which are empty for every other width.  The FP8 arms are instantiated and launched in kv_cache_fp8.hip, a translation
// unit built without packed fp32 instructions; this one is built as it always was.  The kernels themselves: kv_cache_kernels.h.
//
// Work mapping: D/8 lanes own one D-wide head row (8 halves = 16 B each, one coalesced row): 16 lanes (256 B) at head_dim 128,
// 8 lanes (128 B) at head_dim 64; min/max are wave-level DPP reductions inside that lane row -- no LDS.  HBM-bound byte work.
// Both kernels are templated on D (64 | 128): the 8-lane row reduces with xor1, xor2, half-mirror only (the row_ror:8 step of the
// 16-lane row would mix two tokens), a 256-thread workgroup holds 2048 / D token rows.
#include "kv_cache_kernels.h"

namespace tmk {

int launch_kv_rope_store(half_t*        qkv,
                         int            q_heads,
                         const int*     cu_q_len,
                         const int*     k_len,
                         int            batch,
                         int            total_tokens,
                         const half2_t* cos_sin,
                         int            max_pos,
                         KvCacheView    cache,
                         KvScales       scales,
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
    TM_REQUIRE(kvb == 16 || kvb == 8 || kvb == 4 || kvb == kTqBits || kvb == kKvBitsFp8, "kv bits in {16,8,4,42} or TM_KV_BITS_FP8");
    TM_REQUIRE(kvb != kKvBitsFp8 || (scales.k > 0.f && scales.v > 0.f), "kv_rope_store: FP8 KV scales must be > 0");
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
        case kKvBitsFp8:  // instantiated in kv_cache_fp8.hip
            return launch_kv_rope_store_fp8(qkv, q_heads, cu_q_len, k_len, batch, total_tokens, cos_sin, max_pos, cache, scales, st, qkv_bias,
                                            q_norm, k_norm, qk_eps, rope_row0);
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
    TM_REQUIRE(kvb != kKvBitsFp8, "kv_rope_store: M-RoPE with FP8 KV (TM_KV_BITS_FP8) is not built");
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
                                  hipStream_t st,
                                  KvScales    scales)
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
    TM_REQUIRE(bits == 16 || bits == 8 || bits == 4 || bits == kTqBits || bits == kKvBitsFp8, "kv bits in {16,8,4,42} or TM_KV_BITS_FP8");
    if (bits == kKvBitsFp8) {  // instantiated in kv_cache_fp8.hip
        TM_REQUIRE(scales.k > 0.f && scales.v > 0.f, "flatten_kv: FP8 KV scales must be > 0");
        return launch_flatten_kv_fp8(k_out, v_out, transpose_v, cu_k_off, k_len, k_stride, cache, scales, WIN ? cu_q_len : nullptr, window, grid, st);
    }
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
                      KvScales    scales,
                      hipStream_t st)
{
    return launch_flatten_kv_impl<false>(k_out, v_out, transpose_v, cu_k_off, k_len, batch, max_k_len, k_stride, cache, nullptr, 0, st, scales);
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
                             KvScales    scales,
                             hipStream_t st)
{
    TM_REQUIRE(window >= 0, "flatten_kv: window must be >= 0 (0 = the whole context)");
    if (window == 0) {
        return launch_flatten_kv(k_out, v_out, transpose_v, cu_k_off, k_len, batch, max_k_len, k_stride, cache, scales, st);
    }
    TM_REQUIRE(cu_q_len, "flatten_kv: a window needs cu_q_len");
    return launch_flatten_kv_impl<true>(k_out, v_out, transpose_v, cu_k_off, k_len, batch, max_k_len, k_stride, cache, cu_q_len, window, st, scales);
}

}  // namespace tmk
