// Split-K paged flash-decode over the FP8 KV cache (KvLayout::bits == kKvBitsFp8: e4m3fn codes, one fp32 scale per tensor and layer, no
// per-token parameters) on the matrix cores at head_dim 64 and 128, with a sliding window and attention sinks.  Unfused: q is roped and
// the new token is in the cache already (launch_kv_rope_store).  It serves tm_decode_attention and tm_decode_attention_window for the tag.
//
// Arithmetic (include/tm_mi355x.h, TM_KV_BITS_FP8).  A code byte widens in registers to the fp16 value code * 2^-8 -- exactly, subnormals
// included, and every byte, the NaN codes 0x7f / 0xff too, to a FINITE number (f8_widen2: perm into the high bytes, packed arithmetic
// shift, one AND).  Both products run on v_mfma_f32_16x16x32_f16 with fp32 accumulators:
//     S[h,t] = q[h] . kc_t          P = exp2((S - m) * sc),  sc = softmax_scale * log2(e) * k_scale * 2^8          O[h,d] = sum_t P[h,t] vc[t,d]
// k_scale enters once per launch through sc, v_scale * 2^8 once per output element behind the merge of the four waves.  There is no
// per-token multiply on P, no zero term and no sum_d q term.  P is rounded to fp16 in [0, 1]; v_scale multiplies the fp32 accumulator (the
// reference rounds P * v_scale to fp16 instead: the same number of roundings, at another point).  Partials go out in the layout
// decode_reduce_kernel merges, m in the units of its scale_log2 (m * k_scale * 2^8), so that kernel needs no scale of its own; it adds
// the sink term when splits > 1, the epilogue here adds it at splits == 1.
//
// Work split: that of attention_decode_ws_mfma.hip.  A workgroup owns ONE kv head (one chunk of <= 16 of its query heads) x the tiles of
// one split; its four waves take the 64-token tiles newest -> oldest, interleaved, and are merged through LDS at the end.  The query heads
// are the 16 MFMA columns; a group over 16 is cut by dividing out its smallest prime factors until it fits (32 -> 16, 24 -> 12, 34 -> 1).
//
// Window and masking: the query at ctx - 1 sees [wbeg, ctx), wbeg = max(ctx - W, 0).  The splits partition the tiles [wbeg / 64,
// ceil(ctx / 64)) by one rule for every W, so a covering window walks the tiles of W = 0 bit for bit.  Tiles before wbeg / 64 are never
// loaded and their block-table entries never dereferenced.  In a partly visible tile the score of a token outside [wbeg, ctx) is
// SELECTED to -inf, so P = exp2(-inf) = +0 exactly; the token's K and V bytes widen to finite numbers whatever they hold, +0 * finite
// adds +-0 to an accumulator, and no output bit moves.  A split with no tile writes m = -inf, l = 0, o = 0.
//
// Data path -- what differs from the int8 / int4 kernel:
//   K goes from global memory to the MFMA operand through REGISTERS ONLY.  A lane's A operand is 8 consecutive bytes of one token row,
//   and WHICH 8 channels a k-slot stands for is free as long as q is laid out the same way.  So lane (i16, g) loads, for each of the four
//   16-token row tiles tt, the 16-byte chunks g and g + 4 (head_dim 128; chunk g alone at 64) of token row 16 tt + i16: each chunk is two
//   k-steps (its low and high 8 bytes), and the q fragment of step (chunk c, half) holds q[head][16 c + 8 half .. + 8).  A load instruction
//   covers 16 rows x 64 consecutive bytes (the whole row at head_dim 64); the two instructions of a row tile fill its 128-byte lines.  The
//   int8 kernel stages K in LDS only because its loads are laid out for the LDS stores; without parameters to stage next to the codes
//   nothing is left that needs the image, and 64 x D bytes of LDS writes and reads per tile and wave go away.
//   V needs the transposed read (B operand: 8 token rows of one channel), so it keeps a wave-private LDS image [64 tokens][D bytes],
//   chunk-swizzled and read by ds_read_b64_tr_b8 exactly as in attention_decode_ws_mfma.hip (its header has the bank argument: the 16
//   rows a service group reads differ in token bits 0, 1, 2, 4, which the swizzle sends to distinct bank quads; the stores are whole
//   16-byte chunks of consecutive rows, 1 KB per instruction over distinct addresses).
//   Pipeline: the next tile's V loads are issued as soon as this tile's V is in LDS, its K loads as soon as the S products have consumed
//   the K registers -- both stay in flight across softmax and P V.  No parameter words, no Pm region.
//
// LDS per workgroup: four V images = 4 x 64 x D bytes, overlaid by the merge buffers (4 x 16 x D fp32 + 512 bytes): 33 280 bytes at
// head_dim 128 (the int8 kernel: 67 584), 16 896 at 64.  160 KB of LDS then hold four workgroups per CU; registers decide: the kernel is
// compiled for at least 3 waves per SIMD (launch bounds).  The compiler's resource report: head_dim 64 122 VGPRs, 4 waves per SIMD, no
// scratch; head_dim 128 168 VGPRs, 3 waves per SIMD, 24 bytes of scratch per lane (the int8 kernel runs 2 waves per SIMD).
// The bank statements follow from the bank rule; no counter run has confirmed them.
#include "tm_common.h"
#include "tm_kernels.h"
#include <type_traits>

namespace tmk {

namespace {

typedef int v2i __attribute__((ext_vector_type(2)));

#define F8_GLOBAL_AS __attribute__((address_space(1)))
#define F8_CONST_AS __attribute__((address_space(4)))

// 8 code bytes -> 8 fp16 lanes of code * 2^-8 (f8_widen2, tm_common.h)
__device__ __forceinline__ half8_t f8_codes8_to_f16(uint32_t w0, uint32_t w1)
{
    return bit_cast<half8_t>(u32x4{f8_widen2(w0, false), f8_widen2(w0, true), f8_widen2(w1, false), f8_widen2(w1, true)});
}

// chunk swizzle term of token row t of the V image (attention_decode_ws_mfma.hip, ws_vswz)
template<int D>
__device__ __forceinline__ int f8_vswz(int t)
{
    return D == 128 ? ((t >> 1) & 3) | ((t >> 2) & 4) : ((t >> 2) & 1) | ((t >> 3) & 2);
}

template<int D>
constexpr int f8_lds_bytes()
{
    constexpr int images = 4 * 64 * D, merge = 4 * 16 * D * 4 + 4 * 16 * 2 * 4;
    return images > merge ? images : merge;
}

template<int D>
__global__ __launch_bounds__(256, 3) void decode_attention_fp8_mfma_kernel(DecodeAttnParams p, int head_chunks, int hpw, float kmul, float vmul)
{
    static_assert(D == 64 || D == 128, "head_dim 64 / 128");
    constexpr int IMG = 64 * D;   // V image: one byte per code, 64 token rows
    constexpr int CH  = D / 64;   // K chunks (16 bytes) per lane and row tile
    constexpr int NDD = 2 * CH;   // MFMA k-steps of K q^T
    constexpr int NDT = D / 16;   // column tiles of O
    constexpr int CPR = D / 16;   // 16-byte chunks per cache row = V load instructions per tile
    constexpr int RPI = 64 / CPR; // V token rows per load instruction
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const KvLayout L = p.cache.layout;

    const int kv_head = blockIdx.x / head_chunks;
    const int chunk   = blockIdx.x - kv_head * head_chunks;
    const int b       = blockIdx.y;
    const int split   = blockIdx.z;
    const int group   = p.q_heads / L.kv_heads;
    const int head0   = kv_head * group + chunk * hpw;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16  = lane & 15;
    const int g    = lane >> 4;

    char* Vt = smem + wave * IMG;

    // context length and block pointers by scalar loads (read-only during the launch)
    const int       bstride = p.cache.block_stride;
    const uint64_t* blocks  = p.cache.block_ptrs
                             + (bstride > 0 ? (size_t)b * bstride : (size_t) * (const F8_CONST_AS int*)(p.cache.cu_block_nums + b));
    auto block_ptr = [&](int tile) -> const char* {  // tile: wave-uniform
        return (const char*)*(const F8_CONST_AS uint64_t*)(blocks + __builtin_amdgcn_readfirstlane(tile));
    };

    const int ctx        = *(const F8_CONST_AS int*)(p.k_len + b);
    const int wbeg       = p.window > 0 ? max(ctx - p.window, 0) : 0;  // first token the query at ctx - 1 sees
    const int tile_lo    = wbeg >> 6;                                  // tiles before it are skipped, not masked
    const int tiles      = (ctx + 63) >> 6;                            // end of the tile range (absolute)
    const int per_split  = (tiles - tile_lo + p.splits - 1) / p.splits;
    const int tile_begin = tile_lo + split * per_split;
    const int tile_end   = min(tile_begin + per_split, tiles);

    const bool  hv = i16 < hpw;  // a real head column (the others are padding)
    const float sc = p.scale_log2 * kmul;

    floatx4 O[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        O[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, lsum = 0.f;  // per head column i16, partial over this lane's tokens

    const int koff = L.f8_k_data(kv_head, 0);
    const int voff = L.f8_v_data(kv_head, 0);

    u32x4 kreg[4][CH] = {}, vreg[CPR] = {};
    // FIRST: the first tile a wave touches, the only one that can end inside its block: rows past the context are masked below whatever
    // the registers hold, so those lanes re-read the last valid row (same cache lines).  Issued by every wave, branch-free: a wave
    // without a tile reads row 0 of a clamped (mapped) block and never uses it.
    auto last_row = [&](int tile, auto FIRST) {
        return decltype(FIRST)::value ? (tile < tile_begin ? 0 : min(63, ctx - tile * 64 - 1)) : 63;
    };
    // non-temporal: every cache byte is read once per launch by one workgroup; address space 1 spelled out, or the loads are FLAT
    auto load_k = [&](const char* blk, int tile, auto FIRST) {
        const char* base = blk + p.cache.layer_offset + koff + g * 16;
        const int   last = last_row(tile, FIRST);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int off = min(16 * tt + i16, last) * D;
#pragma unroll
            for (int h = 0; h < CH; ++h) {
                kreg[tt][h] = __builtin_nontemporal_load((const F8_GLOBAL_AS u32x4*)(base + off + h * 64));
            }
        }
    };
    auto load_v = [&](const char* blk, int tile, auto FIRST) {
        const char* base = blk + p.cache.layer_offset + voff + (lane % CPR) * 16;
        const int   last = last_row(tile, FIRST);
#pragma unroll
        for (int r = 0; r < CPR; ++r) {
            vreg[r] = __builtin_nontemporal_load((const F8_GLOBAL_AS u32x4*)(base + min(lane / CPR + RPI * r, last) * D));
        }
    };
    auto store_v = [&]() {
#pragma unroll
        for (int r = 0; r < CPR; ++r) {
            const int t = lane / CPR + RPI * r;
            const int c = lane % CPR;
            *(u32x4*)(Vt + t * D + ((c ^ f8_vswz<D>(t)) << 4)) = vreg[r];
        }
    };

    int tile = tile_end - 1 - wave;  // newest -> oldest, waves interleaved
    // the clamp keeps a wave with fewer tiles (or none: an empty split) on a block of the live range [tile_lo, tiles)
    auto        in_range = [&](int t) { return max(min(max(t, tile_begin), tiles - 1), tile_lo); };
    const char* ptr_cur  = block_ptr(in_range(tile));
    const char* ptr_next = block_ptr(in_range(tile - 4));
    load_k(ptr_cur, tile, std::true_type{});
    load_v(ptr_cur, tile, std::true_type{});

    // ---- q^T fragments (B operand of S^T = K q^T): lane (head = i16, g), k-step (h, half) holds q[head][16 (g + 4h) + 8 half .. + 8) ----
    half8_t       qf[NDD];
    const half_t* qp = p.q + (size_t)b * p.q_stride + (size_t)(head0 + (hv ? i16 : 0)) * D;
#pragma unroll
    for (int s = 0; s < NDD; ++s) {
        half8_t t = *(const half8_t*)(qp + 16 * (g + 4 * (s >> 1)) + 8 * (s & 1));
        if (!hv) {
            t = half8_t{};
        }
        qf[s] = t;
    }

    for (; tile >= tile_begin; tile -= 4) {
        store_v();  // wave-private LDS: in-order DS pipeline, no barrier needed
        const int  tok0 = tile * 64;
        const bool more = tile - 4 >= tile_begin;
        if (more) {
            load_v(ptr_next, tile - 4, std::false_type{});  // the next tile's V streams in while this tile is contracted
        }

        // ---- S^T = K q^T on the widened codes, K straight from the load registers -----------------------------------------------------
        floatx4 S[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            S[tt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NDD; ++s) {
                const u32x4   kc = kreg[tt][s >> 1];
                const half8_t a  = (s & 1) ? f8_codes8_to_f16(kc[2], kc[3]) : f8_codes8_to_f16(kc[0], kc[1]);
                S[tt]            = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[s], S[tt], 0, 0, 0);
            }
        }
        if (more) {
            load_k(ptr_next, tile - 4, std::false_type{});  // the K registers are free again
            ptr_next = block_ptr(in_range(tile - 8));       // and the pointer of the tile after it
        }

        // ---- mask, online softmax (lane: head column i16, tokens 16tt + 4g + r) ------------------------------------------------------
        // wave-uniform: only the tile the context ends in and the tile the window starts in hold tokens the query does not see
        if (tok0 + 64 > ctx || tok0 < wbeg) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tok = tok0 + 16 * tt + 4 * g + r;
                    S[tt][r]      = (tok >= wbeg && tok < ctx) ? S[tt][r] : -INFINITY;  // a select: the masked score may be anything
                }
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tmax = fmaxf(tmax, S[tt][r]);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew  = fmaxf(m, tmax);
        const float alpha = (m == -INFINITY) ? 0.f : fast_exp2((m - mnew) * sc);
        if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m))) {  // did any head's max move?  (alpha == 1 exactly otherwise)
            lsum *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = __shfl(alpha, 4 * g + r);  // O rows are heads 4g + r
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    O[dt][r] *= ar;
                }
            }
        }
        m = mnew;
        const float msc = mnew * sc;  // finite: every tile of the range holds >= 1 token the query sees

        half8_t pa[2];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pf = fast_exp2(__builtin_fmaf(S[tt][r], sc, -msc));  // exp2(-inf) = +0 for a masked token
                lsum += pf;
                pa[tt >> 1][(tt & 1) * 4 + r] = (half_t)pf;
            }
        }

        // ---- O = P V on the widened codes: k-slot (g, e) -> token 32a + 4g + e (e < 4) / 32a + 16 + 4g + e - 4 ------------------------
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int   j    = i16 >> 1;
            const int   T    = 32 * a + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
            const char* vrow = Vt + T * D + (i16 & 1) * 8;
            const int   vs   = f8_vswz<D>(T);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const v2i vb = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)(vrow + ((dt ^ vs) << 4)));
                O[dt]        = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa[a], f8_codes8_to_f16((uint32_t)vb[0], (uint32_t)vb[1]), O[dt], 0, 0, 0);
            }
        }
    }

    // ---- per-wave totals, then merge the 4 waves through LDS ------------------------------------------------------------------------
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);

    __syncthreads();  // every wave is done with its image: the region is reused for the merge
    float* sm_o  = (float*)smem;                     // [4][16][D]
    float* sm_ml = (float*)(smem + 4 * 16 * D * 4);  // [4][16][2]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int h = 4 * g + r;
        if (h < hpw) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                sm_o[(wave * 16 + h) * D + dt * 16 + i16] = O[dt][r];
            }
        }
    }
    if (g == 0 && hv) {
        sm_ml[(wave * 16 + i16) * 2]     = m;
        sm_ml[(wave * 16 + i16) * 2 + 1] = lsum;
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < hpw * D; idx += 256) {
        const int h  = idx / D;
        const int d  = idx - h * D;
        float     ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            ms = fmaxf(ms, sm_ml[(w * 16 + h) * 2]);
        }
        float o = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = sm_ml[(w * 16 + h) * 2];
            const float wt = (mw == -INFINITY) ? 0.f : fast_exp2((mw - ms) * sc);
            o += wt * sm_o[(w * 16 + h) * D + d];
            l += wt * sm_ml[(w * 16 + h) * 2 + 1];
        }
        o *= vmul;  // v_scale * 2^8, once per output element
        const int hq = head0 + h;
        if (p.splits == 1) {
            if (p.sinks) {  // the sink logit joins the denominator once and carries no value; exp2(-inf) = +0 changes no bit
                l += fast_exp2((float)p.sinks[hq] * 1.4426950408889634f - ms * sc);
            }
            p.out[(size_t)b * p.q_heads * D + (size_t)hq * D + d] = (half_t)(o / l);
        }
        else {  // decode_reduce_kernel merges the splits (m in the units of p.scale_log2) and adds the sink; an empty split: -inf, 0, 0
            const size_t slot         = ((size_t)b * p.q_heads + hq) * p.splits + split;
            p.partial_o[slot * D + d] = o;
            if (d == 0) {
                p.partial_ml[slot * 2]     = ms * kmul;
                p.partial_ml[slot * 2 + 1] = l;
            }
        }
    }
}

template<int D>
int launch_f8(const DecodeAttnParams& p, KvScales s, hipStream_t st)
{
    const int group = p.q_heads / p.cache.layout.kv_heads;
    int       hpw   = group;
    while (hpw > 16) {  // divide out the smallest factors until the chunk fits the 16 MFMA columns (not always the largest such divisor)
        int d = 2;
        while (hpw % d) {
            ++d;
        }
        hpw /= d;
    }
    const int     chunks = group / hpw;
    const dim3    grid(p.cache.layout.kv_heads * chunks, p.batch, p.splits);
    constexpr int lds = f8_lds_bytes<D>();
    const auto    K   = decode_attention_fp8_mfma_kernel<D>;
    if (const int rc = ensure_dynamic_lds((const void*)K, lds)) {
        return rc;
    }
    K<<<grid, 256, lds, st>>>(p, chunks, hpw, s.k * 256.0f, s.v * 256.0f);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int launch_decode_attention_fp8_mfma(const DecodeAttnParams& p, KvScales s, hipStream_t st)
{
    const KvLayout& L = p.cache.layout;
    TM_REQUIRE(L.bits == kKvBitsFp8, "FP8 MFMA decode attention: FP8 KV (TM_KV_BITS_FP8) only");
    TM_REQUIRE(L.head_dim == 64 || L.head_dim == 128, "FP8 MFMA decode attention: head_dim 64 or 128");
    TM_REQUIRE(L.block_len == 64 && L.kv_heads > 0 && p.q_heads % L.kv_heads == 0, "FP8 MFMA decode attention: block_len 64, q_heads % kv_heads");
    TM_REQUIRE(p.window >= 0, "FP8 MFMA decode attention: window must be >= 0 (0 = full attention)");
    TM_REQUIRE(!p.qkv_slabs && !p.qkv_f16, "fused decode prologue with FP8 KV is not built: run tm_kv_rope_store + tm_decode_attention");
    TM_REQUIRE(s.k > 0.f && s.v > 0.f, "FP8 MFMA decode attention: k_scale and v_scale must be > 0");
    return L.head_dim == 64 ? launch_f8<64>(p, s, st) : launch_f8<128>(p, s, st);
}

}  // namespace tmk
