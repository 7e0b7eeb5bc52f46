// Bidirectional (non-causal) flash attention over packed variable-length segments on MFMA (gfx950): the attention of the
// Qwen2-VL / Qwen2.5-VL vision tower, straight on the fused qkv linear's output, 2-D rotary embedding included.
//
// Replaces: the ViT attention of the reference's qwenvit model -- Attn / CreateVitAttentionParams (src/turbomind/models/qwenvit/
//           qwenvit.cc) -> dispatchAttention with a non-causal mask over cu_seqlens.  Arithmetic contract (transformers,
//           apply_rotary_pos_emb_vision + per-segment softmax): q' = fp16(f32(q) * cos + rotate_half(f32(q)) * sin), k' alike, then
//           O = softmax(scale * q' k'^T) v over the keys of the row's own segment, fp32 accumulators, one rounding to fp16.
//
// Inputs: qkv fp16 [tokens][3][heads][D] (row stride qkv_stride), cu_seqlens int32 [nseg + 1] (device), cos / sin fp16 or fp32
// [tokens][>= D/2] (row stride cs_stride), a work list of (segment, 64-row query block) built on the host.  D = 64 | 80 | 128, ONE
// template: DP = D rounded up to 32 is the width of the QK contraction, NDD = DP / 32 its MFMA k-steps, NDT = D / 16 the O column tiles.
//
// Layout (as attention_prefill.hip, wave64, v_mfma_f32_16x16x32_f16): scores are computed transposed, S^T = K Q^T, so a lane's
// accumulator (column = query row, 4 consecutive keys) is, after exp2 and a cast, the B operand of O^T = V^T P^T: P never leaves the
// registers.  Score tile A row 4g + r <-> key 8g + r, tile B <-> key 8g + 4 + r of a 32-key step: a lane's 8 probabilities are 8
// consecutive keys.  A workgroup = 4 waves = 64 query rows of ONE head of ONE segment (no GQA in a ViT), 16 rows per wave.
//
// D = 80: the third k-step holds channels 64 .. 95; its lanes g = 2, 3 (channels 80 .. 95) carry zeros in REGISTERS on both operands
// (Q fragment and K fragment are selects on g), so the pad is neither in HBM nor in LDS: K rows in LDS are 160 B, V rows too.
//
// Stages: 64 keys of K and V go through LDS once per workgroup, double buffered, one barrier per stage.  They go through REGISTERS
// (16-byte global loads of stage s + 1 are issued before stage s is contracted, rotated and written to LDS behind it), not LDS-DMA,
// because K is rotated on the way: RoPE on K happens WHILE A STAGE IS LOADED.  The alternative, a pre-pass that writes rotated K,
// needs a workspace of tokens * heads * D fp16, a launch per block and a second trip of K through HBM.  In 28 of Qwen2.5-VL's 32
// blocks a segment is a window of <= 64 tokens, i.e. ONE query block per (segment, head): every key is rotated exactly once either
// way.  In a full-attention segment of n tokens a key is rotated n / 64 times, 24 fp32 VALU ops per 16 channels beside the 2 * 64
// MFMA rows it feeds.  The pair (c, c + D/2) of rotate-half lives in ONE thread (it loads both 16-byte chunks, cos and sin once).
// Rows past the segment's end are written as ZEROS, K and V both: a masked key has P = 0, but 0 * NaN from a neighbouring
// segment's V would still poison O.
//
// V is stored row-major [key][D] as it arrives and transposed on the way OUT of LDS by ds_read_b64_tr_b16: the 16 lanes of a g
// pass the addresses of 4 key rows x 16 head-dim columns (lane i: row i / 4, columns 4 (i % 4) .. + 3) and lane i receives column
// i of the four rows -- two reads give a lane its 8 keys of head-dim row 16 dt + i16, the A operand of O^T = V^T P^T.
//
// Banks (rule: bank = byte address / 4 mod 64; a ds_read_b128 is served in groups of 16 lanes {0-3, 12-15, 20-27}, {4-11, 16-19,
// 28-31}, ..., a 64-bit read 32 lanes at a time).  160-byte rows do not tile the 64 banks the way 128 / 256 do, and 10 slots of 16 B
// cannot be XOR-swizzled.  Instead (1) the row pitch is P slots of 16 B with P even and P / 2 odd: 10 (D = 64, 80: for 80 that is
// the natural pitch), 18 (D = 128) -- then r * P mod 16 = 2 (r * P/2 mod 8) takes 8 distinct even values over any 8 rows that are
// distinct mod 8; and (2) the loader, which owns the placement, stores key k at the LDS row its READERS want consecutive:
//   * K: row = the score-tile row, key 32s + 8q + 4t + j -> row 32s + 16t + 4q + j.  A service group is g's lanes i16 in {0-3, 12-15}
//     on chunk c and (g + 1)'s lanes i16 in {4-11} on chunk c + 1 (c even): rows {0-3, 12-15} -> the eight even slots, rows {4-11}
//     -> the eight odd ones: 16 distinct 16-byte slots, conflict-free, the same at every D.
//   * V: bits 2 and 3 of the key swapped, so that the keys {8g + 4h + j : g in a pair, j < 4} of one transposed read are 8
//     consecutive rows; each row contributes 32 contiguous bytes (8 banks) at start bank 4 P r + 8 dt mod 64 = 8 (r * P/2 mod 8) +
//     8 dt: eight rows, eight distinct octets of banks: conflict-free.
// The loader's 16-byte LDS writes were not analysed.  No counter run has confirmed either statement.
//
// Work split: the host knows every segment length (image_grid_thw), vision_plan() lists (segment, query block) for every non-empty
// segment, longest segments first (the dispatcher hands out workgroups in blockIdx order: longest-processing-time first), and
// blockIdx.x = item * heads + head.  No tile straddles a segment; the only masks are the ragged last rows and last keys.
// No split-K, no paged cache, no GQA, no window / sink / bias / dropout.
#include "tm_common.h"
#include "tm_kernels.h"
#include <algorithm>
#include <numeric>
#include <vector>

namespace tmk {

namespace {

#define GLOBAL_AS __attribute__((address_space(1)))
#define LDS_AS __attribute__((address_space(3)))

constexpr float kMinScoreV = -1.0e30f;  // finite start of the running maximum: see attention_prefill.hip

typedef unsigned vu32x2_t __attribute__((ext_vector_type(2)));
typedef short    v4s_t __attribute__((ext_vector_type(4)));
// max / sum over the lane pairs l ^ 16 and l ^ 32 by gfx950's row / half swaps (as in attention_prefill.hip)
__device__ __forceinline__ float vmax_xor16_xor32(float v)
{
    unsigned       b = __builtin_bit_cast(unsigned, v);
    const vu32x2_t r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    b = __builtin_bit_cast(unsigned, fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1])));
    const vu32x2_t q = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)q[0]), __builtin_bit_cast(float, (unsigned)q[1]));
}
__device__ __forceinline__ float vsum_xor16_xor32(float v)
{
    unsigned       b = __builtin_bit_cast(unsigned, v);
    const vu32x2_t r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    b                = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]));
    const vu32x2_t q = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return __builtin_bit_cast(float, (unsigned)q[0]) + __builtin_bit_cast(float, (unsigned)q[1]);
}

// 8 consecutive cos (or sin) values of a token as fp32
struct F8 {
    floatx4 a, b;  // vectors, not an array: the values stay in registers whatever the control flow around them
    __device__ __forceinline__ float operator[](int e) const { return e < 4 ? a[e] : b[e - 4]; }
};
template<bool F32>
__device__ __forceinline__ F8 load_cs8(const void* base, size_t elem)
{
    F8 r;
    if constexpr (F32) {
        r.a = *(const GLOBAL_AS floatx4*)((const float*)base + elem);
        r.b = *(const GLOBAL_AS floatx4*)((const float*)base + elem + 4);
    }
    else {
        const half8_t h = *(const GLOBAL_AS half8_t*)((const half_t*)base + elem);
        r.a = floatx4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        r.b = floatx4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
    }
    return r;
}

// rotate-half on the chunk pair (x1 = channels c .. c+7 of the first half, x2 = the same of the second half), op by op in fp32 as
// apply_rotary_pos_emb_vision states it (the Makefile's -ffp-contract=off keeps mul, mul, add apart), one rounding to fp16:
//   o1 = x1 * cos + (-x2) * sin      o2 = x2 * cos + x1 * sin
__device__ __forceinline__ void rope_pair(half8_t& x1, half8_t& x2, const F8& c, const F8& s)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float a = (float)x1[e], b = (float)x2[e];
        x1[e]         = (half_t)(a * c[e] + (-b) * s[e]);
        x2[e]         = (half_t)(b * c[e] + a * s[e]);
    }
}

}  // namespace

template<int D, bool CSF32>
__global__ __launch_bounds__(256, 2) void vision_attention_kernel(VisionAttnParams p)
{
    static_assert(D == 64 || D == 80 || D == 128, "head_dim 64, 80 or 128");
    constexpr int  NDD   = (D + 31) / 32;                 // MFMA k-steps of the QK contraction (the last one half zero at D = 80)
    constexpr int  NDT   = D / 16;                        // 16-column tiles of O
    constexpr int  NCH   = D / 8;                         // 16-byte chunks of a row
    constexpr int  NP    = D / 16;                        // rotate-half chunk pairs of a row
    constexpr bool PAD   = D % 32 != 0;
    constexpr int  PITCH = (NCH % 4 == 2 ? NCH : NCH + 2) * 16;  // bytes; slots even, slots / 2 odd: 160 | 160 | 288
    constexpr int  KS    = 64;                            // keys per stage
    constexpr int  TILE  = KS * PITCH;                    // bytes of a K tile (and of a V tile)
    constexpr int  STG   = 2 * TILE;
    constexpr int  KIT   = (KS * NP + 255) / 256;         // chunk pairs of K per thread and stage: 1 | 2 (the second a quarter full) | 2
    constexpr int  VIT   = (KS * NCH + 255) / 256;        // chunks of V per thread and stage: 2 | 3 | 4
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int item = blockIdx.x / p.heads;
    const int head = blockIdx.x - item * p.heads;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16  = lane & 15;
    const int g    = lane >> 4;

    const int2 w = p.work[item];
    if ((unsigned)w.x >= (unsigned)p.nseg) {
        return;  // workgroup-uniform; a work list is the caller's, the bounds are ours
    }
    const int beg  = min(max(p.cu_seqlens[w.x], 0), p.tokens);
    const int slen = min(max(p.cu_seqlens[w.x + 1], beg), p.tokens) - beg;  // keys = query rows of the segment
    if (w.y < 0 || w.y * 64 >= slen) {
        return;
    }
    const int  q0     = w.y * 64 + wave * 16;
    const bool active = q0 < slen;  // wave-uniform; an inactive wave still stages tiles and meets the barriers

    const half_t* qbase = p.qkv + (size_t)head * D;                        // + token * qkv_stride
    const half_t* kbase = qbase + (size_t)p.heads * D;
    const half_t* vbase = kbase + (size_t)p.heads * D;

    // Q^T fragments (B operand), rotated: lane (j = query row, g) holds q'[q0 + j][32 dd + 8g .. + 8)
    half8_t qf[NDD];
    {
        const size_t  tok  = (size_t)(beg + min(q0 + i16, slen - 1));
        const half_t* qptr = qbase + tok * p.qkv_stride;
#pragma unroll
        for (int dd = 0; dd < NDD; ++dd) {
            const int  c     = 4 * dd + g;
            const bool valid = !PAD || c < NCH;
            const int  cc    = valid ? c : c - 2;               // a pad lane reads a chunk of its own row and drops it
            const bool lo    = cc < NP;                         // first half of the head
            const int  c1    = lo ? cc : cc - NP;
            half8_t    x1    = *(const GLOBAL_AS half8_t*)(qptr + c1 * 8);
            half8_t    x2    = *(const GLOBAL_AS half8_t*)(qptr + (c1 + NP) * 8);
            const F8   cs    = load_cs8<CSF32>(p.cos, tok * p.cs_stride + c1 * 8);
            const F8   sn    = load_cs8<CSF32>(p.sin, tok * p.cs_stride + c1 * 8);
            rope_pair(x1, x2, cs, sn);
            const half8_t r = lo ? x1 : x2;
            qf[dd]          = valid ? r : half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }

    // ---- the loader: registers of the stage in flight -------------------------------------------------------------------------
    half8_t kx1[KIT], kx2[KIT], vx[VIT];
    F8      kc[KIT], ksn[KIT];
    auto stage_load = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            const int idx = it * 256 + (int)threadIdx.x;
            const int key = idx / NP, pc = idx - key * NP;
            // branch-free: a row past the segment's end (or past the 64 keys, in a ragged last pass) loads the segment's LAST token and
            // is then zeroed by a select -- every address stays inside the segment, and 0 * cos + 0 * sin = 0 is what LDS gets
            const size_t  tok = (size_t)(beg + min(ks + key, slen - 1));
            const half_t* kp  = kbase + tok * p.qkv_stride + pc * 8;
            kx1[it]           = *(const GLOBAL_AS half8_t*)kp;
            kx2[it]           = *(const GLOBAL_AS half8_t*)(kp + NP * 8);
            kc[it]            = load_cs8<CSF32>(p.cos, tok * p.cs_stride + pc * 8);
            ksn[it]           = load_cs8<CSF32>(p.sin, tok * p.cs_stride + pc * 8);
            if (ks + key >= slen) {
                kx1[it] = kx2[it] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
#pragma unroll
        for (int it = 0; it < VIT; ++it) {
            const int idx = it * 256 + (int)threadIdx.x;
            const int key = idx / NCH, c = idx - key * NCH;
            vx[it] = *(const GLOBAL_AS half8_t*)(vbase + (size_t)(beg + min(ks + key, slen - 1)) * p.qkv_stride + c * 8);
            if (ks + key >= slen) {
                vx[it] = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    };
    auto stage_store = [&](int buf) __attribute__((always_inline)) {
        char* kt = smem + buf * STG;
        char* vt = kt + TILE;
#pragma unroll
        for (int it = 0; it < KIT; ++it) {
            const int idx = it * 256 + (int)threadIdx.x;
            const int key = idx / NP, pc = idx - key * NP;
            if (idx < KS * NP) {
                rope_pair(kx1[it], kx2[it], kc[it], ksn[it]);
                const int row = (key & 32) | ((key & 4) << 2) | ((key & 24) >> 1) | (key & 3);  // the score-tile row of the key
                *(half8_t*)(kt + row * PITCH + pc * 16)        = kx1[it];
                *(half8_t*)(kt + row * PITCH + (pc + NP) * 16) = kx2[it];
            }
        }
#pragma unroll
        for (int it = 0; it < VIT; ++it) {
            const int idx = it * 256 + (int)threadIdx.x;
            const int key = idx / NCH, c = idx - key * NCH;
            if (idx < KS * NCH) {
                const int row = (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1);  // key bits 2 and 3 swapped
                *(half8_t*)(vt + row * PITCH + c * 16) = vx[it];
            }
        }
    };

    floatx4 O[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        O[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    float       m = kMinScoreV, l = 0.f;
    const float sc = p.scale_log2;

    stage_load(0);
    stage_store(0);
    __syncthreads();
    int buf = 0;
    for (int ks0 = 0; ks0 < slen; ks0 += KS, buf ^= 1) {
        const bool more = ks0 + KS < slen;  // workgroup-uniform
        if (more) {
            stage_load(ks0 + KS);  // in flight while this stage is contracted
        }
        const char* kt = smem + buf * STG;
        const char* vt = kt + TILE;
#pragma nounroll
        for (int sub = 0; sub < 2; ++sub) {
            const int ks = ks0 + 32 * sub;
            if (!active || ks >= slen) {  // wave-uniform
                continue;
            }
            floatx4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
            {
                const char* ra = kt + (32 * sub + i16) * PITCH;  // tile A: rows 32 sub + i16, tile B: + 16
                const char* rb = ra + 16 * PITCH;
#pragma unroll
                for (int dd = 0; dd < NDD; ++dd) {
                    const int  c     = 4 * dd + g;
                    const bool valid = !PAD || c < NCH;
                    const int  cc    = valid ? c : c - 2;
                    half8_t    ka    = *(const half8_t*)(ra + cc * 16);
                    half8_t    kb    = *(const half8_t*)(rb + cc * 16);
                    if (!valid) {
                        ka = kb = half8_t{0, 0, 0, 0, 0, 0, 0, 0};
                    }
                    sa = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, qf[dd], sa, 0, 0, 0);
                    sb = __builtin_amdgcn_mfma_f32_16x16x32_f16(kb, qf[dd], sb, 0, 0, 0);
                }
            }
            // lane holds S[key = ks + 8g + r][q] in sa[r] and S[key = ks + 8g + 4 + r][q] in sb[r]
            float s[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r]     = sa[r];
                s[4 + r] = sb[r];
            }
            if (ks + 32 > slen) {  // the segment's ragged last keys (wave-uniform)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s[e] = ks + 8 * g + e < slen ? s[e] : -INFINITY;
                }
            }
            float tmax = s[0];
#pragma unroll
            for (int e = 1; e < 8; ++e) {
                tmax = fmaxf(tmax, s[e]);
            }
            tmax              = vmax_xor16_xor32(tmax);
            const float mnew  = fmaxf(m, tmax);  // finite (kMinScoreV at least)
            const float alpha = fast_exp2((m - mnew) * sc);
            const float ms    = mnew * sc;
            float       psum  = 0.f;
            half8_t     pf;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float pv = fast_exp2(__builtin_fmaf(s[e], sc, -ms));  // masked score: exp2(-inf) = 0
                psum += pv;
                pf[e] = (half_t)pv;
            }
            l = l * alpha + psum;
            if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m))) {  // wave-uniform: did any row's max move?
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    O[dt] *= alpha;
                }
            }
            m = mnew;
            // ---- O^T += V^T P^T: the transposed read hands lane (i16, g) V[keys ks + 8g + 4h .. + 3][16 dt + i16] ----
            const char* vr = vt + (32 * sub + 16 * (g >> 1) + 4 * (g & 1) + (i16 >> 2)) * PITCH + (i16 & 3) * 8;
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const half4_t v0 = bit_cast<half4_t>(__builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS v4s_t*)(vr + dt * 32)));
                const half4_t v1 = bit_cast<half4_t>(__builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS v4s_t*)(vr + 8 * PITCH + dt * 32)));
                const half8_t vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                O[dt]            = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, O[dt], 0, 0, 0);
            }
        }
        if (more) {
            stage_store(buf ^ 1);  // every wave is past the barrier behind its reads of that buffer
        }
        __syncthreads();  // the next stage is complete, and everybody is done reading this one
    }

    if (active && q0 + i16 < slen) {
        const float lh   = vsum_xor16_xor32(l);
        const float inv  = 1.0f / lh;
        half_t*     optr = p.out + (size_t)(beg + q0 + i16) * p.heads * D + (size_t)head * D;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            half4_t o = {(half_t)(O[dt][0] * inv), (half_t)(O[dt][1] * inv), (half_t)(O[dt][2] * inv), (half_t)(O[dt][3] * inv)};
            *(half4_t*)(optr + dt * 16 + g * 4) = o;
        }
    }
}

// (segment, 64-row query block) of every non-empty segment, longest segments first (stable: equal lengths keep their order).
// Returns the number of items, or -1 when cu_seqlens does not start at 0 or decreases.
int vision_plan(const int* cu_seqlens, int nseg, int* work, int capacity)
{
    if (nseg < 0 || cu_seqlens[0] != 0) {
        return -1;
    }
    for (int s = 0; s < nseg; ++s) {
        if (cu_seqlens[s + 1] < cu_seqlens[s]) {
            return -1;
        }
    }
    std::vector<int> order(nseg);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return cu_seqlens[a + 1] - cu_seqlens[a] > cu_seqlens[b + 1] - cu_seqlens[b];
    });
    int n = 0;
    for (const int s : order) {
        const int blocks = (cu_seqlens[s + 1] - cu_seqlens[s] + 63) / 64;
        for (int b = 0; b < blocks; ++b, ++n) {
            if (work && n < capacity) {
                work[2 * n]     = s;
                work[2 * n + 1] = b;
            }
        }
    }
    return n;
}

template<int D, bool CSF32>
static int launch_vision(const VisionAttnParams& p, hipStream_t st)
{
    constexpr int     NCH = D / 8;
    constexpr int     lds = 2 * 2 * 64 * (NCH % 4 == 2 ? NCH : NCH + 2) * 16;  // two stages of (K tile + V tile)
    const void* const k   = (const void*)vision_attention_kernel<D, CSF32>;
    if (const int rc = ensure_dynamic_lds(k, lds)) {
        return rc;
    }
    vision_attention_kernel<D, CSF32><<<dim3((unsigned)(p.n_work * p.heads)), 256, lds, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_vision_attention(const VisionAttnParams& p, int head_dim, bool cs_f32, hipStream_t st)
{
    TM_REQUIRE(head_dim == 64 || head_dim == 80 || head_dim == 128, "vision attention: head_dim must be 64, 80 or 128");
    TM_REQUIRE(p.heads >= 1 && p.tokens >= 0 && p.nseg >= 0 && p.n_work >= 0, "vision attention: negative size");
    TM_REQUIRE((long long)p.n_work * p.heads <= 0x7fffffffLL, "vision attention: work items * heads exceed the grid");
    if (p.n_work == 0 || p.tokens == 0) {
        return 0;
    }
    switch (head_dim) {
        case 64:
            return cs_f32 ? launch_vision<64, true>(p, st) : launch_vision<64, false>(p, st);
        case 80:
            return cs_f32 ? launch_vision<80, true>(p, st) : launch_vision<80, false>(p, st);
        default:
            return cs_f32 ? launch_vision<128, true>(p, st) : launch_vision<128, false>(p, st);
    }
}

}  // namespace tmk
