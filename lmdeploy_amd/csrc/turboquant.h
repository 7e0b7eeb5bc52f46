// TurboQuant KV cache (quant_policy 42): K = 3-bit Lloyd-Max code of the Hadamard-rotated row + the sign of the residual ("QJL4",
// 4 bits), V = 2-bit Lloyd-Max code of the rotated row; one fp16 pair of norms per row.  head_dim 128.
//
// Replaces: the TurboQuant branch of lmdeploy/pytorch/kernels/cuda/fill_kv_cache.py:326-514 (Triton, PyTorch engine only) and
//           the codebooks of lmdeploy/pytorch/kernels/cuda/turbo_quant.py:163-186.
//
// Contract (fp32 unless stated; D = 128, H[i][j] = (-1)^popcount(i & j), unnormalised):
//   f = f32(x); y = H f; n = sqrtf(sum f_i^2)
//   idx_i = #{ j : y_i > beta_j * n }                                   (no division: one definition of the integer outputs)
//   K only: r_i = y_i - c3[idx_i] * n; s_i = (r_i >= 0); g = n > 0 ? sqrtf(sum r_i^2) / (n * D) : 0
//   K code_i = idx_i | s_i << 3, params half2{h(n), h(g)};   V code_i = idx_i (2 bits), params half2{h(n), 0}
//   rotated-domain row:  K^_i = n (c3[idx_i] / sqrt(D) + g (2 s_i - 1)),  V^_i = n c2[idx_i] / sqrt(D);  original: (H K^) / sqrt(D)
// Bytes: a K row is D/2 bytes, dword w = dims 8w .. 8w+7, nibble i = element [0,2,4,6,1,3,5,7][i] (the int4 order);
//        a V row is D/4 bytes, dword w = dims 16w .. 16w+15, 2-bit field i = element [0,2,..,14,1,3,..,15][i].
#pragma once
#include "tm_common.h"

namespace tmk {

constexpr int   kTqBits   = 42;
constexpr float kTqRsqrtD = 0.08838834764831845f;  // 1 / sqrt(128)

// Lloyd-Max quantisers of N(0, 1): 4 and 8 levels, ascending; boundaries = midpoints
__device__ __forceinline__ float tq_c2(uint32_t i)
{
    const float mag = (i == 0 || i == 3) ? 1.5104176f : 0.4527808f;
    return i < 2 ? -mag : mag;
}
__device__ __forceinline__ float tq_c3(uint32_t i)
{
    const uint32_t m   = i < 4 ? 3 - i : i - 4;  // magnitude rank 0..3
    const float    mag = m == 0 ? 0.2450942f : m == 1 ? 0.7560052f : m == 2 ? 1.3439093f : 2.1519456f;
    return i < 4 ? -mag : mag;
}
constexpr float kTqBeta2 = 0.9815992f;
constexpr float kTqBeta3a = 0.5005497f, kTqBeta3b = 1.0499573f, kTqBeta3c = 1.7479274f;

constexpr int DPP_XOR3 = 0x1B;  // quad_perm [3,2,1,0]; behind row_half_mirror (i ^ 7) it is the exchange i ^ 4

// partner of the lane at distance XOR inside a 16-lane row
template<int XOR>
__device__ __forceinline__ float dpp_xor(float v)
{
    static_assert(XOR == 1 || XOR == 2 || XOR == 4 || XOR == 8, "row exchange");
    if constexpr (XOR == 1) {
        return dpp_f32<DPP_XOR1>(v);
    }
    else if constexpr (XOR == 2) {
        return dpp_f32<DPP_XOR2>(v);
    }
    else if constexpr (XOR == 4) {
        return dpp_f32<DPP_XOR3>(dpp_f32<DPP_HMIRR>(v));
    }
    else {
        return dpp_f32<DPP_ROR8>(v);
    }
}

// one butterfly stage across lanes: the lane whose bit is clear keeps a + b, the other one a - b (a = the lower index)
__device__ __forceinline__ float tq_bfly(float v, float partner, bool upper)
{
    return upper ? partner - v : v + partner;
}

// y = H v for a 128-wide row held by 16 lanes x 8 consecutive elements (element 8 * lane16 + e): 3 stages in registers, 4 by DPP
__device__ __forceinline__ void fwht128_row16(float (&v)[8], int lane16)
{
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if ((e & s) == 0) {
                const float a = v[e], b = v[e | s];
                v[e]          = a + b;
                v[e | s]      = a - b;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        v[e] = tq_bfly(v[e], dpp_xor<1>(v[e]), lane16 & 1);
        v[e] = tq_bfly(v[e], dpp_xor<2>(v[e]), lane16 & 2);
        v[e] = tq_bfly(v[e], dpp_xor<4>(v[e]), lane16 & 4);
        v[e] = tq_bfly(v[e], dpp_xor<8>(v[e]), lane16 & 8);
    }
}

// y = H v for a 128-wide row held by one wave, lane l = elements (2l, 2l + 1): 1 stage in registers, 4 by DPP, 2 by lane exchange
__device__ __forceinline__ void fwht128_wave(float& a, float& b, int lane)
{
    const float s = a + b, d = a - b;
    a = s, b = d;
    a = tq_bfly(a, dpp_xor<1>(a), lane & 1), b = tq_bfly(b, dpp_xor<1>(b), lane & 1);
    a = tq_bfly(a, dpp_xor<2>(a), lane & 2), b = tq_bfly(b, dpp_xor<2>(b), lane & 2);
    a = tq_bfly(a, dpp_xor<4>(a), lane & 4), b = tq_bfly(b, dpp_xor<4>(b), lane & 4);
    a = tq_bfly(a, dpp_xor<8>(a), lane & 8), b = tq_bfly(b, dpp_xor<8>(b), lane & 8);
    a = tq_bfly(a, __shfl_xor(a, 16), lane & 16), b = tq_bfly(b, __shfl_xor(b, 16), lane & 16);
    a = tq_bfly(a, __shfl_xor(a, 32), lane & 32), b = tq_bfly(b, __shfl_xor(b, 32), lane & 32);
}

// Quantise one head row (16 lanes x 8 halves, all 16 lanes active) and store its codes and norms.  No LDS, no atomics.
template<bool IS_K>
__device__ __forceinline__ void tq_store_row(half8_t x, int lane16, char* data, char* param)
{
    float y[8];
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        y[e] = (float)x[e];
        ss   = __builtin_fmaf(y[e], y[e], ss);  // the square of an fp16 is exact in fp32
    }
    const float n = __builtin_sqrtf(group_sum<16>(ss));
    fwht128_row16(y, lane16);
    uint32_t q[8];
    if constexpr (IS_K) {
        const float ba = kTqBeta3a * n, bb = kTqBeta3b * n, bc = kTqBeta3c * n;
        float       rr = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t idx = (uint32_t)(y[e] > -bc) + (uint32_t)(y[e] > -bb) + (uint32_t)(y[e] > -ba) + (uint32_t)(y[e] > 0.f)
                                 + (uint32_t)(y[e] > ba) + (uint32_t)(y[e] > bb) + (uint32_t)(y[e] > bc);
            const float t = tq_c3(idx) * n;
            const float r = y[e] - t;
            q[e]          = idx | (r >= 0.f ? 8u : 0u);
            rr += r * r;
        }
        rr = group_sum<16>(rr);
        // nibble i of the word = element [0,2,4,6,1,3,5,7][i]
        const uint32_t w = q[0] | (q[2] << 4) | (q[4] << 8) | (q[6] << 12) | (q[1] << 16) | (q[3] << 20) | (q[5] << 24) | (q[7] << 28);
        *(uint32_t*)(data + lane16 * 4) = w;
        if (lane16 == 0) {
            const float g = n > 0.f ? __builtin_sqrtf(rr) / (n * 128.0f) : 0.f;
            half2_t     pr = {(half_t)n, (half_t)g};
            *(half2_t*)param = pr;
        }
    }
    else {
        const float b = kTqBeta2 * n;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q[e] = (uint32_t)(y[e] > -b) + (uint32_t)(y[e] > 0.f) + (uint32_t)(y[e] > b);
        }
        // the dword of a lane pair holds 16 dims; field i = element [0,2,..,14,1,3,..,15][i]: this lane's even elements land in byte
        // (lane16 & 1), its odd ones in byte 2 + (lane16 & 1)
        const uint32_t ev   = q[0] | (q[2] << 2) | (q[4] << 4) | (q[6] << 6);
        const uint32_t od   = q[1] | (q[3] << 2) | (q[5] << 4) | (q[7] << 6);
        const int      sh   = (lane16 & 1) * 8;
        const uint32_t half = (ev << sh) | (od << (16 + sh));
        const uint32_t w    = half | dpp_u32<DPP_XOR1>(half);
        if ((lane16 & 1) == 0) {
            *(uint32_t*)(data + (lane16 >> 1) * 4) = w;
        }
        if (lane16 == 0) {
            half2_t pr = {(half_t)n, (half_t)0.f};
            *(half2_t*)param = pr;
        }
    }
}

// Dims [8 * lane16, 8 * lane16 + 8) of one cached row in the ORIGINAL domain: unpack, rebuild the rotated row, inverse FWHT, one
// rounding to fp16.  All 16 lanes of the row active.
template<bool IS_K>
__device__ __forceinline__ half8_t tq_flatten_row(const char* data, const char* param, int lane16)
{
    const half2_t pr = *(const half2_t*)param;
    const float   n  = (float)pr[0];
    float         v[8];
    if constexpr (IS_K) {
        const float    g = (float)pr[1];
        const uint32_t w = *(const uint32_t*)(data + lane16 * 4);
        constexpr int  nib_of[8] = {0, 4, 1, 5, 2, 6, 3, 7};  // element e sits in nibble nib_of[e]
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t c = (w >> (4 * nib_of[e])) & 0xfu;
            v[e]             = n * (tq_c3(c & 7u) * kTqRsqrtD + ((c & 8u) ? g : -g));
        }
    }
    else {
        const uint32_t w  = *(const uint32_t*)(data + (lane16 >> 1) * 4);
        const int      sh = (lane16 & 1) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int      bit = (e & 1) ? 16 + sh + (e - 1) : sh + e;
            const uint32_t c   = (w >> bit) & 3u;
            v[e]               = n * (tq_c2(c) * kTqRsqrtD);
        }
    }
    fwht128_row16(v, lane16);
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] = (half_t)(v[e] * kTqRsqrtD + 0.0f);  // (+ 0: a zero row comes back as +0, whatever signs the butterflies left)
    }
    return o;
}

}  // namespace tmk
