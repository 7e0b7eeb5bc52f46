// The FP8 KV cache's instantiations of the store and flatten kernels (kv_cache_kernels.h; contract: include/tm_mi355x.h, TM_KV_BITS_FP8)
// and their launches.  A translation unit of its own because it is built without packed fp32 instructions (Makefile): the FP8 arms clamp
// and scale eight fp32 values per lane, which the compiler otherwise pairs into v_pk_mul_f32 and its kin.  kv_cache.hip checks the
// arguments and computes the grid; these two functions only pick the instantiation.
#include "kv_cache_kernels.h"

namespace tmk {

int launch_kv_rope_store_fp8(half_t* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                             const half2_t* cos_sin, int max_pos, KvCacheView cache, KvScales scales, hipStream_t st, const half_t* qkv_bias,
                             const half_t* q_norm, const half_t* k_norm, float qk_eps, const int* rope_row0)
{
    const int  hd  = cache.layout.head_dim;
    const int  tpw = 2048 / hd;  // token rows per 256-thread workgroup, as in launch_kv_rope_store
    const dim3 grid((total_tokens + tpw - 1) / tpw, q_heads + 2 * cache.layout.kv_heads);
    const bool qkx = qkv_bias != nullptr || q_norm != nullptr;
    const bool seq = rope_row0 != nullptr;
#define TM_KV_STORE_F8(X_, S_, D_)                                                                                                       \
    kv_rope_store_kernel<kKvBitsFp8, X_, S_, D_, false><<<grid, 256, 0, st>>>(qkv, q_heads, cu_q_len, k_len, batch, total_tokens, cos_sin, \
                                                                              max_pos, cache, qkv_bias, q_norm, k_norm, qk_eps, rope_row0, \
                                                                              scales.k, scales.v)
#define TM_KV_STORE_F8_D(D_)                          \
    do {                                              \
        if (qkx && seq) TM_KV_STORE_F8(true, true, D_);   \
        else if (qkx) TM_KV_STORE_F8(true, false, D_);    \
        else if (seq) TM_KV_STORE_F8(false, true, D_);    \
        else TM_KV_STORE_F8(false, false, D_);            \
    } while (0)
    if (hd == 64) {
        TM_KV_STORE_F8_D(64);
    }
    else {
        TM_KV_STORE_F8_D(128);
    }
#undef TM_KV_STORE_F8_D
#undef TM_KV_STORE_F8
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// cu_q_len != nullptr: the sliding-window variant (launch_flatten_kv_window with window > 0)
int launch_flatten_kv_fp8(half_t* k_out, half_t* v_out, int transpose_v, const int* cu_k_off, const int* k_len, int k_stride,
                          KvCacheView cache, KvScales scales, const int* cu_q_len, int window, dim3 grid, hipStream_t st)
{
#define TM_FLATTEN_F8(T_, D_)                                                                                                          \
    do {                                                                                                                               \
        if (cu_q_len != nullptr)                                                                                                       \
            flatten_kv_kernel<kKvBitsFp8, T_, D_, true><<<grid, 256, 0, st>>>(k_out, v_out, cu_k_off, k_len, k_stride, cache, scales.k, \
                                                                              scales.v, cu_q_len, window);                             \
        else                                                                                                                           \
            flatten_kv_kernel<kKvBitsFp8, T_, D_><<<grid, 256, 0, st>>>(k_out, v_out, cu_k_off, k_len, k_stride, cache, scales.k,      \
                                                                        scales.v);                                                     \
    } while (0)
    if (cache.layout.head_dim == 64) {
        if (transpose_v) TM_FLATTEN_F8(true, 64);
        else TM_FLATTEN_F8(false, 64);
    }
    else if (transpose_v) {
        TM_FLATTEN_F8(true, 128);
    }
    else {
        TM_FLATTEN_F8(false, 128);
    }
#undef TM_FLATTEN_F8
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
