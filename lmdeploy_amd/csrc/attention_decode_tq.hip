// Split-K paged flash-decode over a TurboQuant KV cache (KV bits 42, head_dim 128), entirely in the rotated domain (gfx950).
//
// Replaces: the TurboQuant branch of the reference's PyTorch-engine paged attention (lmdeploy/pytorch/kernels/cuda/pagedattention.py,
//           which de-rotates every K / V row it reads); the TurboMind engine of the reference has no such path.
//
// H is symmetric and H H = D I, so with q' = H q / sqrt(D) and the cached rotated rows K^, V^ (turboquant.h):
//   q . (H K^ / sqrt(D)) = q' . K^          S_t = n_t * sum_i (c3[idx_i] / sqrt(D) + g_t * (+-1)) q'_i
//   sum_t p_t (H V^_t / sqrt(D)) = H (sum_t p_t V^_t) / sqrt(D):   O' += p_t * n_t / sqrt(D) * c2[idx];   out = H (O' / L) / sqrt(D)
// One rotation of q per head in the prologue and one of the output behind the merge: no cached row is ever de-rotated.
//
// Mapping: the structure of decode_attention_kernel (attention_decode.hip): one workgroup = (kv head, <= 4 query heads, sequence,
// split), its 4 waves take alternate 32-token tiles with online-softmax state of their own, merged once through LDS.  8 lanes share a
// token, 16 dims each: one 8-byte load per lane covers 8 K rows (64 B each), one 4-byte load 8 V rows (32 B each).  Centroids come
// from two v_perm byte tables (low and high bytes of the fp16 centroids, 4 codes per instruction); the sign of the residual becomes
// the sign of an fp16 +-1 that one packed fma multiplies by g: k^ = h(fma(+-1, g, c3 / sqrt(D))), the score is n * fdot2(k^, q').
// Masking, the order of the online softmax, the k_len >= 1 contract and the workspace are those of decode_attention_kernel.
#include "tm_common.h"
#include "tm_kernels.h"
#include "turboquant.h"

namespace tmk {

namespace {

constexpr int D    = 128;
constexpr int E    = 16;        // head dims per lane
constexpr int CPT  = D / E;     // 8 lanes share a token
constexpr int TILE = 32;        // tokens per online-softmax step
constexpr int TPI  = 64 / CPT;  // 8 tokens per load instruction
constexpr int IPT  = TILE / TPI;

// fp16 bit patterns of the centroids as byte tables for v_perm: entry i of (lo, hi) = low / high byte of h(c[i] / sqrt(128)) for K,
// h(c[i]) for V (the 1 / sqrt(128) of V goes into the fp32 weight)
//   K: c3 / sqrt(128) = -+0.190205, -+0.118786, -+0.066822, -+0.021663  -> 0xb216 0xaf9a 0xac47 0xa58c | 0x258c 0x2c47 0x2f9a 0x3216
//   V: c2 = -1.5104176 -0.4527808 0.4527808 1.5104176                   -> 0xbe0b 0xb73f 0x373f 0x3e0b
constexpr uint32_t kK_lo03 = 0x8c479a16u, kK_lo47 = 0x169a478cu;
constexpr uint32_t kK_hi03 = 0xa5acafb2u, kK_hi47 = 0x322f2c25u;
constexpr uint32_t kV_lo   = 0x0b3f3f0bu, kV_hi = 0x3e37b7beu;

// 8 K codes of one dword -> 4 half2 pairs (2p, 2p + 1) of k^ / n = c3[idx] / sqrt(D) + g * (+-1)
__device__ __forceinline__ void tq_k_dword(uint32_t raw, half2_t g2, half2_t (&out)[4])
{
    // bytes of selA = nibbles 0, 2, 4, 6 = elements 0, 4, 1, 5; of selB = nibbles 1, 3, 5, 7 = elements 2, 6, 3, 7
    const uint32_t selA = raw & 0x07070707u;
    const uint32_t selB = (raw >> 4) & 0x07070707u;
    const uint32_t la = __builtin_amdgcn_perm(kK_lo47, kK_lo03, selA), ha = __builtin_amdgcn_perm(kK_hi47, kK_hi03, selA);
    const uint32_t lb = __builtin_amdgcn_perm(kK_lo47, kK_lo03, selB), hb = __builtin_amdgcn_perm(kK_hi47, kK_hi03, selB);
    uint32_t       c[4];
    c[0] = __builtin_amdgcn_perm(ha, la, 0x06020400u);  // elements (0, 1)
    c[2] = __builtin_amdgcn_perm(ha, la, 0x07030501u);  // elements (4, 5)
    c[1] = __builtin_amdgcn_perm(hb, lb, 0x06020400u);  // elements (2, 3)
    c[3] = __builtin_amdgcn_perm(hb, lb, 0x07030501u);  // elements (6, 7)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        // bit 3 of nibbles p and p + 4 -> the sign bits of an fp16 pair of ones: +1 where the residual was >= 0
        const uint32_t sg = ((raw << (12 - 4 * p)) & 0x80008000u) ^ 0xbc00bc00u;
        out[p]            = h2_fma(bit_cast<half2_t>(sg), g2, bit_cast<half2_t>(c[p]));
    }
}

// 16 V codes of one dword -> 8 half2 pairs of c2[idx]: out[p] = elements (2p, 2p + 1)
__device__ __forceinline__ void tq_v_dword(uint32_t raw, half2_t (&out)[8])
{
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        // bytes of sel = fields p, p + 4, p + 8, p + 12 = elements 2p, 2p + 8, 2p + 1, 2p + 9
        const uint32_t sel = (raw >> (2 * p)) & 0x03030303u;
        const uint32_t lo = __builtin_amdgcn_perm(0u, kV_lo, sel), hi = __builtin_amdgcn_perm(0u, kV_hi, sel);
        out[p]     = bit_cast<half2_t>(__builtin_amdgcn_perm(hi, lo, 0x06020400u));
        out[p + 4] = bit_cast<half2_t>(__builtin_amdgcn_perm(hi, lo, 0x07030501u));
    }
}

template<int HPW>
__global__ __launch_bounds__(256, 2) void decode_attention_tq_kernel(DecodeAttnParams p, int head_chunks)
{
    const KvLayout L = p.cache.layout;

    const int kv_head = blockIdx.x / head_chunks;
    const int chunk   = blockIdx.x - kv_head * head_chunks;
    const int b       = blockIdx.y;
    const int split   = blockIdx.z;
    const int group   = p.q_heads / L.kv_heads;
    const int head0   = kv_head * group + chunk * HPW;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c    = lane % CPT;
    const int tg   = lane / CPT;

    const int ctx        = p.k_len[b];
    const int tiles      = (ctx + TILE - 1) / TILE;
    const int per_split  = (tiles + p.splits - 1) / p.splits;
    const int tile_begin = split * per_split;
    const int tile_end   = min(tile_begin + per_split, tiles);

    __shared__ float sm_o[4][HPW][D];
    __shared__ float sm_ml[4][HPW][2];
    __shared__ half_t sm_q[HPW][D];

    // ---- q' = H q / sqrt(D): wave h rotates head h (lane l = dims 2l, 2l + 1), every lane then takes its 16 dims --------------
    if (wave < HPW) {
        const half2_t t = *(const half2_t*)(p.q + (size_t)b * p.q_stride + (size_t)(head0 + wave) * D + lane * 2);
        float         a = (float)t[0], bq = (float)t[1];
        fwht128_wave(a, bq, lane);
        *(half2_t*)(&sm_q[wave][lane * 2]) = half2_t{(half_t)(a * kTqRsqrtD), (half_t)(bq * kTqRsqrtD)};
    }
    __syncthreads();
    half2_t qv[HPW][E / 2];
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
#pragma unroll
        for (int i = 0; i < E / 2; ++i) {
            qv[h][i] = *(const half2_t*)(&sm_q[h][c * E + 2 * i]);
        }
    }

    float m[HPW], lsum[HPW], O[HPW][E];
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
        m[h]    = -INFINITY;
        lsum[h] = 0.f;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            O[h][e] = 0.f;
        }
    }
    const float sc = p.scale_log2;

    const uint64_t* blocks = p.cache.block_ptrs + p.cache.cu_block_nums[b];

    // newest -> oldest, waves interleaved
    for (int tile = tile_end - 1 - wave; tile >= tile_begin; tile -= 4) {
        const int   tok0  = tile * TILE;
        const int   toff  = tok0 & 63;
        const char* base  = (const char*)blocks[tok0 >> 6] + p.cache.layer_offset;
        const char* kdata = base + L.tq_k_data(kv_head, toff);
        const char* vdata = base + L.tq_v_data(kv_head, toff);
        const int   ntok  = min(TILE, ctx - tok0);  // >= 1

        // per-token (n, g): lane = token; rows past the context get n = g = 0 (their bytes may be anything)
        uint32_t kpar = *(const uint32_t*)(base + L.tq_k_param(kv_head, toff + (lane & (TILE - 1))));
        uint32_t vpar = *(const uint32_t*)(base + L.tq_v_param(kv_head, toff + (lane & (TILE - 1))));
        if (lane >= ntok) {
            kpar = 0;
            vpar = 0;
        }

        // ---- K: S[r][h] ------------------------------------------------------------------------
        u32x2 kraw[IPT];
#pragma unroll
        for (int r = 0; r < IPT; ++r) {
            kraw[r] = __builtin_nontemporal_load((const u32x2*)(kdata + (size_t)(r * TPI + tg) * (D / 2) + c * 8));
        }
        float S[IPT][HPW];
#pragma unroll
        for (int r = 0; r < IPT; ++r) {
            const half2_t pp = bit_cast<half2_t>((uint32_t)__shfl((int)kpar, r * TPI + tg));
            const float   n  = (float)pp[0];
            const half2_t g2 = {pp[1], pp[1]};
            half2_t       kd[E / 2];
            {
                half2_t lo[4], hi[4];
                tq_k_dword(kraw[r][0], g2, lo);
                tq_k_dword(kraw[r][1], g2, hi);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    kd[i]     = lo[i];
                    kd[4 + i] = hi[i];
                }
            }
            const bool valid = r * TPI + tg < ntok;
#pragma unroll
            for (int h = 0; h < HPW; ++h) {
                float acc = 0.f;
#pragma unroll
                for (int i = 0; i < E / 2; ++i) {
                    acc = __builtin_amdgcn_fdot2(kd[i], qv[h][i], acc, false);
                }
                acc     = group_sum<CPT>(acc);
                S[r][h] = valid ? acc * n : -INFINITY;
            }
        }

        // ---- V loads (issued before the softmax math so they overlap it) -------------------
        uint32_t vraw[IPT];
#pragma unroll
        for (int r = 0; r < IPT; ++r) {
            vraw[r] = __builtin_nontemporal_load((const uint32_t*)(vdata + (size_t)(r * TPI + tg) * (D / 4) + c * 4));
        }

        // ---- online softmax ---------------------------------------------------------------
        float alpha[HPW];
        bool  rescale = false;
#pragma unroll
        for (int h = 0; h < HPW; ++h) {
            float tm_ = S[0][h];
#pragma unroll
            for (int r = 1; r < IPT; ++r) {
                tm_ = fmaxf(tm_, S[r][h]);
            }
            tm_              = upper_max<CPT>(tm_);
            const float mnew = fmaxf(m[h], tm_);
            alpha[h]         = (m[h] == -INFINITY) ? 0.f : fast_exp2((m[h] - mnew) * sc);
            rescale |= (mnew != m[h]);
            m[h] = mnew;
        }
        if (__builtin_amdgcn_readfirstlane((int)rescale)) {
#pragma unroll
            for (int h = 0; h < HPW; ++h) {
                lsum[h] *= alpha[h];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    O[h][e] *= alpha[h];
                }
            }
        }

        // ---- P.V in the rotated domain: O' += (p * n / sqrt(D)) * c2[idx] -------------------------
#pragma unroll
        for (int r = 0; r < IPT; ++r) {
            const half2_t pp = bit_cast<half2_t>((uint32_t)__shfl((int)vpar, r * TPI + tg));
            const float   vn = (float)pp[0] * kTqRsqrtD;
            half2_t       vd[E / 2];
            tq_v_dword(vraw[r], vd);
#pragma unroll
            for (int h = 0; h < HPW; ++h) {
                const float  pf = fast_exp2(S[r][h] * sc - m[h] * sc);  // exp2(-inf) = 0 for masked tokens
                const half_t ph = (half_t)pf;
                lsum[h] += (c == 0) ? pf : 0.f;
                const float w = (float)ph * vn;
#pragma unroll
                for (int i = 0; i < E / 2; ++i) {
                    O[h][2 * i]     = __builtin_fmaf(w, (float)vd[i][0], O[h][2 * i]);
                    O[h][2 * i + 1] = __builtin_fmaf(w, (float)vd[i][1], O[h][2 * i + 1]);
                }
            }
        }
    }

    // ---- reduce over the token lanes of the wave, then over the 4 waves through LDS -------------
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
        lsum[h] = group_sum<64>(lsum[h]);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            O[h][e] = upper_sum<CPT>(O[h][e]);
        }
        if (tg == 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                sm_o[wave][h][c * E + e] = O[h][e];
            }
        }
        if (lane == 0) {
            sm_ml[wave][h][0] = m[h];
            sm_ml[wave][h][1] = lsum[h];
        }
    }
    __syncthreads();

    // wave h merges head h: lane l = rotated dims (2l, 2l + 1); with one split it also rotates back and writes the output row
    if (wave < HPW) {
        const int h  = wave;
        float     ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            ms = fmaxf(ms, sm_ml[w][h][0]);
        }
        float o0 = 0.f, o1 = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = sm_ml[w][h][0];
            const float wt = (mw == -INFINITY) ? 0.f : fast_exp2((mw - ms) * sc);
            o0 += wt * sm_o[w][h][2 * lane];
            o1 += wt * sm_o[w][h][2 * lane + 1];
            l += wt * sm_ml[w][h][1];
        }
        const int hq = head0 + h;
        if (p.splits == 1) {
            o0 = o0 / l, o1 = o1 / l;
            fwht128_wave(o0, o1, lane);
            *(half2_t*)(p.out + (size_t)b * p.q_heads * D + (size_t)hq * D + 2 * lane) =
                half2_t{(half_t)(o0 * kTqRsqrtD), (half_t)(o1 * kTqRsqrtD)};
        }
        else {
            const size_t slot = ((size_t)b * p.q_heads + hq) * p.splits + split;
            p.partial_o[slot * D + 2 * lane]     = o0;
            p.partial_o[slot * D + 2 * lane + 1] = o1;
            if (lane == 0) {
                p.partial_ml[slot * 2]     = ms;
                p.partial_ml[slot * 2 + 1] = l;
            }
        }
    }
}

// split-K merge in the rotated domain, then the one rotation back: one wave per (sequence, query head), lane l = dims (2l, 2l + 1)
__global__ __launch_bounds__(64) void decode_reduce_tq_kernel(DecodeAttnParams p)
{
    const int    hq   = blockIdx.x;
    const int    b    = blockIdx.y;
    const int    lane = threadIdx.x;
    const size_t slot = ((size_t)b * p.q_heads + hq) * p.splits;
    float        ms   = -INFINITY;
    for (int s = 0; s < p.splits; ++s) {
        ms = fmaxf(ms, p.partial_ml[(slot + s) * 2]);
    }
    float o0 = 0.f, o1 = 0.f, l = 0.f;
    for (int s = 0; s < p.splits; ++s) {
        const float mw = p.partial_ml[(slot + s) * 2];
        const float wt = (mw == -INFINITY) ? 0.f : fast_exp2((mw - ms) * p.scale_log2);
        o0 += wt * p.partial_o[(slot + s) * D + 2 * lane];
        o1 += wt * p.partial_o[(slot + s) * D + 2 * lane + 1];
        l += wt * p.partial_ml[(slot + s) * 2 + 1];
    }
    o0 = o0 / l, o1 = o1 / l;
    fwht128_wave(o0, o1, lane);
    *(half2_t*)(p.out + (size_t)b * p.q_heads * D + (size_t)hq * D + 2 * lane) = half2_t{(half_t)(o0 * kTqRsqrtD), (half_t)(o1 * kTqRsqrtD)};
}

}  // namespace

int launch_decode_attention_tq(const DecodeAttnParams& p, hipStream_t st)
{
    const KvLayout& L = p.cache.layout;
    TM_REQUIRE(L.bits == kTqBits && L.block_len == 64, "decode attention (TurboQuant): kv bits 42, block_len 64");
    TM_REQUIRE(L.head_dim == 128, "decode attention: kv bits 42 (TurboQuant) needs head_dim 128, head_dim 64 is not built");
    TM_REQUIRE(!p.qkv_slabs && !p.qkv_f16,
               "fused decode prologue with kv bits 42 (TurboQuant) is not built: run tm_kv_rope_store + tm_decode_attention");
    TM_REQUIRE(p.window == 0 && !p.sinks, "decode attention: kv bits 42 (TurboQuant) with a sliding window or attention sinks is not built");
    TM_REQUIRE(p.q_stride % 2 == 0, "decode attention (TurboQuant): q_stride must be even");
    const int group = p.q_heads / L.kv_heads;
    int       hpw   = 1;
    for (int cand = 4; cand >= 1; --cand) {
        if (group % cand == 0) {
            hpw = cand;
            break;
        }
    }
    const int chunks = group / hpw;
    dim3      grid(L.kv_heads * chunks, p.batch, p.splits);
    switch (hpw) {
        case 4:
            decode_attention_tq_kernel<4><<<grid, 256, 0, st>>>(p, chunks);
            break;
        case 3:
            decode_attention_tq_kernel<3><<<grid, 256, 0, st>>>(p, chunks);
            break;
        case 2:
            decode_attention_tq_kernel<2><<<grid, 256, 0, st>>>(p, chunks);
            break;
        default:
            decode_attention_tq_kernel<1><<<grid, 256, 0, st>>>(p, chunks);
    }
    TM_HIP_CHECK(hipGetLastError());
    if (p.splits > 1) {
        decode_reduce_tq_kernel<<<dim3(p.q_heads, p.batch), 64, 0, st>>>(p);
        TM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace tmk
