// Split-K paged flash-decode for int8 / int4 KV on the matrix cores at head_dim 64 and 128, with a sliding window and attention
// sinks (DecodeAttnParams::window, ::sinks): the shapes attention_decode_mfma.hip refuses.  Unfused: q is roped and the new token is
// in the cache already (launch_kv_rope_store), as for the VALU kernel's window variant, which this kernel replaces for these calls.
//
// Arithmetic: that of attention_decode_mfma.hip.  The codes enter v_mfma_f32_16x16x32_f16 as the exact fp16 subnormals b * 2^-24,
//     S[h,t] = s_t * (q . kq_t) + z_t * sum_d q[h,d]          O[h,d] = sum_t (P s_t)[h,t] vq[t,d] + sum_t P[h,t] z_t
// with fp32 accumulators and exp2 on scale_log2; partials go to partial_o / partial_ml in the layout decode_reduce_kernel merges
// (it adds the sink term when splits > 1; at splits == 1 the epilogue below adds it once).
//
// Work split: a workgroup owns ONE kv head (one chunk of <= 16 of its query heads) x the token range of one split; its four waves take
// the range's 64-token tiles newest -> oldest, interleaved, and are merged through LDS at the end.  The query heads of the GQA group
// are the 16 score columns of the MFMA; a group smaller than 16 leaves padding columns (q = 0, never written): at group 4 the kernel
// issues 4 x the useful MFMAs, and still needs 32 (head_dim 64) or 64 MFMAs per 64-token tile against the ~1400 VALU instructions of
// the kernel it replaces.  Groups over 16 are cut into the largest divisor <= 16 (workgroups along blockIdx.x).
//
// Window: the query at ctx - 1 sees the tokens [wbeg, ctx), wbeg = max(ctx - W, 0) (W = 0: wbeg = 0).  The splits partition the tiles
// [wbeg / 64, ceil(ctx / 64)) -- for every W by the same rule, so a window that covers the context walks the tiles of the call without
// one, bit for bit.  Tiles before wbeg / 64 are never loaded, nor are their block-table entries dereferenced.  Inside the one tile the
// window starts in (and the one the context ends in) masking is a SELECT on the token index: the score becomes -inf and the token's V
// (scale, zero) word 0, so P s_t and P z_t are +0 whatever the masked token's cache bytes hold (NaN parameters included).  A split
// with no tile writes m = -inf, l = 0, o = 0.
//
// Data path per wave and tile: block pointer by scalar load (one block ahead) -> 16-byte non-temporal global loads into registers (the
// next tile's stay in flight while this one is contracted) -> wave-private LDS image [64 tokens][D bytes] of K and of V (int4: nibbles
// expanded to one byte per code on the way) + [64][(k_param, v_param)] -> K operand by ds_read_b64, V operand by ds_read_b64_tr_b8.
//
// LDS image and banks (bank = byte address / 4 mod 64; a ds_read_b64 is served 32 lanes at a time, 256 bytes = every bank once if no
// two lanes meet).  A row is D bytes = D / 16 chunks of 16 bytes, the chunk index XORed with a term of the token:
//   K, read by (token 16tt + i16, 8 bytes (4dd + g) of the row): a service group is g in {0, 1} or {2, 3}, i.e. BOTH halves of ONE chunk
//      of 16 consecutive token rows.  D = 128: two rows span the banks; chunk ^ ((t >> 1) & 7) sends the eight row pairs to eight
//      chunks.  D = 64: four rows span the banks; chunk ^ ((t >> 2) & 3) sends the four row quads to four chunks.  16 distinct bank
//      quads either way: conflict-free.
//   V, transposed read: lane (g, i16) addresses half i16 & 1 of chunk dt of token row T = 32a + {4g + j | 16 + 4g + j - 4}, j = i16 >> 1;
//      a service group reads one chunk of the 16 rows {0..7, 16..23} (+ 8 for g in {2, 3}).  Those rows differ in bits 0, 1, 2 and 4.
//      D = 128: bit 0 picks the half of the bank span, bits (1, 2, 4) -> swizzle bits (0, 1, 2).  D = 64: bits (0, 1) pick the
//      quarter of the bank span, bits (2, 4) -> swizzle bits (0, 1).  16 distinct bank quads: conflict-free.  (K's term would fold
//      rows T and T + 16 onto each other here.)
//   The stores are whole 16-byte chunks of consecutive rows: 1 KB per instruction over distinct addresses, four passes, the minimum.
// Both statements follow from the bank rule; no counter run has confirmed them.
#include "tm_common.h"
#include "tm_kernels.h"
#include <type_traits>

namespace tmk {

namespace {

typedef int v2i __attribute__((ext_vector_type(2)));

// byte b -> fp16 bit pattern 0x00bb = b * 2^-24 (attention_decode_mfma.hip)
__device__ __forceinline__ half8_t ws_codes8_to_f16(u32x2 w)
{
    const uint32_t a0 = __builtin_amdgcn_perm(0u, w[0], 0x0c010c00u);
    const uint32_t a1 = __builtin_amdgcn_perm(0u, w[0], 0x0c030c02u);
    const uint32_t a2 = __builtin_amdgcn_perm(0u, w[1], 0x0c010c00u);
    const uint32_t a3 = __builtin_amdgcn_perm(0u, w[1], 0x0c030c02u);
    return bit_cast<half8_t>(u32x4{a0, a1, a2, a3});
}
constexpr float kWsTwo24 = 16777216.0f;

#define WS_GLOBAL_AS __attribute__((address_space(1)))
#define WS_CONST_AS __attribute__((address_space(4)))

// 32 int4 codes (cache order [0,2,4,6,1,3,5,7] per word) -> 32 bytes in element order (attention_decode_mfma.hip)
__device__ __forceinline__ void ws_expand_nibbles32(u32x4 w, u32x4& a, u32x4& b)
{
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t lo = w[j] & 0x0f0f0f0fu;
        const uint32_t hi = (w[j] >> 4) & 0x0f0f0f0fu;
        o[2 * j]     = __builtin_amdgcn_perm(hi, lo, 0x06040200u);
        o[2 * j + 1] = __builtin_amdgcn_perm(hi, lo, 0x07050301u);
    }
    a = u32x4{o[0], o[1], o[2], o[3]};
    b = u32x4{o[4], o[5], o[6], o[7]};
}

// chunk swizzle terms of token row t (file header)
template<int D>
__device__ __forceinline__ int ws_kswz(int t)
{
    return D == 128 ? (t >> 1) & 7 : (t >> 2) & 3;
}
template<int D>
__device__ __forceinline__ int ws_vswz(int t)
{
    return D == 128 ? ((t >> 1) & 3) | ((t >> 2) & 4) : ((t >> 2) & 1) | ((t >> 3) & 2);
}

template<int D>
constexpr int ws_wave_lds()
{
    return 2 * 64 * D + 512;  // K image | V image | (k_param, v_param) per token
}

template<int D, int BITS>
__global__ __launch_bounds__(256, 2) void decode_attention_ws_mfma_kernel(DecodeAttnParams p, int head_chunks, int hpw)
{
    static_assert((D == 64 || D == 128) && (BITS == 8 || BITS == 4), "head_dim 64 / 128, int8 / int4 KV");
    constexpr int IMG  = 64 * D;           // one byte per code, 64 token rows
    constexpr int NDD  = D / 32;           // MFMA k-steps of K q^T
    constexpr int NDT  = D / 16;           // column tiles of O
    constexpr int GROW = D * BITS / 8;     // bytes of a token row in the cache
    constexpr int CPR  = GROW / 16;        // 16-byte chunks per cache row = load instructions per tile (8, 4 | 4, 2)
    constexpr int RPI  = 64 / CPR;         // token rows per load instruction
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

    char* Kt = smem + wave * ws_wave_lds<D>();
    char* Vt = Kt + IMG;
    char* Pm = Kt + 2 * IMG;

    // context length and block pointers by scalar loads (read-only during the launch)
    const int       bstride = p.cache.block_stride;
    const uint64_t* blocks  = p.cache.block_ptrs
                             + (bstride > 0 ? (size_t)b * bstride : (size_t) * (const WS_CONST_AS int*)(p.cache.cu_block_nums + b));
    auto block_ptr = [&](int tile) -> const char* {  // tile: wave-uniform
        return (const char*)*(const WS_CONST_AS uint64_t*)(blocks + __builtin_amdgcn_readfirstlane(tile));
    };

    const int ctx        = *(const WS_CONST_AS int*)(p.k_len + b);
    const int wbeg       = p.window > 0 ? max(ctx - p.window, 0) : 0;  // first token the query at ctx - 1 sees
    const int tile_lo    = wbeg >> 6;                                  // tiles before it are skipped, not masked
    const int tiles      = (ctx + 63) >> 6;                            // end of the tile range (absolute)
    const int per_split  = (tiles - tile_lo + p.splits - 1) / p.splits;
    const int tile_begin = tile_lo + split * per_split;
    const int tile_end   = min(tile_begin + per_split, tiles);

    const bool  hv = i16 < hpw;  // a real head column (the others are padding)
    const float sc = p.scale_log2;

    floatx4 O[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
        O[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, lsum = 0.f, zacc = 0.f;  // per head column i16, partial over this lane's tokens

    const int koff  = L.k_data(kv_head, 0);
    const int voff  = L.v_data(kv_head, 0);
    const int kpoff = L.k_param(kv_head, 0);
    const int vpoff = L.v_param(kv_head, 0);

    u32x4    kreg[CPR] = {}, vreg[CPR] = {};
    uint32_t kpr = 0, vpr = 0;
    // FIRST: the first tile a wave touches, the only one that can end inside its block: rows past the context are masked below
    // whatever the registers hold, so those lanes re-read the last valid row (same cache lines).  Issued by every wave, branch-free: a
    // wave without a tile reads row 0 of a clamped (mapped) block and never uses it.
    auto load_tile = [&](const char* blk, int tile, auto FIRST) {
        const char* base = blk + p.cache.layer_offset;
        const int   last = decltype(FIRST)::value ? (tile < tile_begin ? 0 : min(63, ctx - tile * 64 - 1)) : 63;
#pragma unroll
        for (int r = 0; r < CPR; ++r) {
            const int row = lane / CPR + RPI * r;
            const int off = min(row, last) * GROW + (lane % CPR) * 16;
            // non-temporal: every cache byte is read once per launch by one workgroup; address space 1 spelled out, or the loads are FLAT
            kreg[r] = __builtin_nontemporal_load((const WS_GLOBAL_AS u32x4*)(base + koff + off));
            vreg[r] = __builtin_nontemporal_load((const WS_GLOBAL_AS u32x4*)(base + voff + off));
        }
        kpr = *(const WS_GLOBAL_AS uint32_t*)(base + kpoff + lane * 4);
        vpr = *(const WS_GLOBAL_AS uint32_t*)(base + vpoff + lane * 4);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int r = 0; r < CPR; ++r) {
            const int t  = lane / CPR + RPI * r;
            const int c  = lane % CPR;
            const int ks = ws_kswz<D>(t), vs = ws_vswz<D>(t);
            if constexpr (BITS == 8) {
                *(u32x4*)(Kt + t * D + ((c ^ ks) << 4)) = kreg[r];
                *(u32x4*)(Vt + t * D + ((c ^ vs) << 4)) = vreg[r];
            }
            else {  // 32 nibbles -> the two 16-byte chunks 2c, 2c + 1 of the token's image row
                u32x4 lo, hi;
                ws_expand_nibbles32(kreg[r], lo, hi);
                *(u32x4*)(Kt + t * D + (((2 * c) ^ ks) << 4))     = lo;
                *(u32x4*)(Kt + t * D + (((2 * c + 1) ^ ks) << 4)) = hi;
                ws_expand_nibbles32(vreg[r], lo, hi);
                *(u32x4*)(Vt + t * D + (((2 * c) ^ vs) << 4))     = lo;
                *(u32x4*)(Vt + t * D + (((2 * c + 1) ^ vs) << 4)) = hi;
            }
        }
        *(u32x2*)(Pm + lane * 8) = u32x2{kpr, vpr};
    };

    int tile = tile_end - 1 - wave;  // newest -> oldest, waves interleaved
    // the clamp keeps a wave with fewer tiles (or none: an empty split) on a block of the live range [tile_lo, tiles)
    auto        in_range = [&](int t) { return max(min(max(t, tile_begin), tiles - 1), tile_lo); };
    const char* ptr_cur  = block_ptr(in_range(tile));
    const char* ptr_next = block_ptr(in_range(tile - 4));
    load_tile(ptr_cur, tile, std::true_type{});

    // ---- q^T fragments (B operand of S^T = K q^T): lane (head = i16, g) holds q[head][32dd + 8g .. +8) ------------------------------
    half8_t       qf[NDD];
    float         q1 = 0.f;  // sum_d q[head][d]
    const half_t* qp = p.q + (size_t)b * p.q_stride + (size_t)(head0 + (hv ? i16 : 0)) * D;
#pragma unroll
    for (int dd = 0; dd < NDD; ++dd) {
        half8_t t = *(const half8_t*)(qp + dd * 32 + g * 8);
        if (!hv) {
            t = half8_t{};
        }
        qf[dd] = t;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q1 += (float)t[e];
        }
    }
    q1 += __shfl_xor(q1, 16);
    q1 += __shfl_xor(q1, 32);

    for (; tile >= tile_begin; tile -= 4) {
        store_tile();  // wave-private LDS: in-order DS pipeline, no barrier needed
        const int tok0 = tile * 64;
        if (tile - 4 >= tile_begin) {
            load_tile(ptr_next, tile - 4, std::false_type{});  // the next tile streams in while this one is contracted
            ptr_next = block_ptr(in_range(tile - 8));          // and the pointer of the one after it
        }

        // ---- S^T = K q^T on raw codes ---------------------------------------------------------------------------------------------
        floatx4 S[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            S[tt]        = floatx4{0.f, 0.f, 0.f, 0.f};
            const int t  = 16 * tt + i16;
            const int ks = ws_kswz<D>(t);
#pragma unroll
            for (int dd = 0; dd < NDD; ++dd) {
                const int     u  = 4 * dd + g;
                const u32x2   kb = *(const u32x2*)(Kt + t * D + (((u >> 1) ^ ks) << 4) + (u & 1) * 8);
                const half8_t a  = ws_codes8_to_f16(kb);  // code * 2^-24, exact
                S[tt]            = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[dd], S[tt], 0, 0, 0);
            }
        }

        // ---- scales, mask, online softmax (lane: head column i16, tokens 16tt + 4g + r) ----------------------------------------------
        uint32_t vp[4][4];
        float    sv[4][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const u32x4    pa_ = *(const u32x4*)(Pm + (16 * tt + 4 * g) * 8);       // tokens +0, +1
            const u32x4    pb_ = *(const u32x4*)(Pm + (16 * tt + 4 * g) * 8 + 16);  // tokens +2, +3
            const uint32_t kp[4] = {pa_[0], pa_[2], pb_[0], pb_[2]};
            vp[tt][0] = pa_[1], vp[tt][1] = pa_[3], vp[tt][2] = pb_[1], vp[tt][3] = pb_[3];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const half2_t kk = bit_cast<half2_t>(kp[r]);
                sv[tt][r]        = __builtin_fmaf((float)kk[0] * kWsTwo24, S[tt][r], (float)kk[1] * q1);
            }
        }
        // wave-uniform: only the tile the context ends in and the tile the window starts in hold tokens the query does not see
        if (tok0 + 64 > ctx || tok0 < wbeg) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int  tok  = tok0 + 16 * tt + 4 * g + r;
                    const bool seen = tok >= wbeg && tok < ctx;
                    sv[tt][r]       = seen ? sv[tt][r] : -INFINITY;  // selects: the masked values may be NaN
                    vp[tt][r]       = seen ? vp[tt][r] : 0u;
                }
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                tmax = fmaxf(tmax, sv[tt][r]);
            }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
        const float mnew  = fmaxf(m, tmax);
        const float alpha = (m == -INFINITY) ? 0.f : fast_exp2((m - mnew) * sc);
        if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m))) {  // did any head's max move?  (alpha == 1 exactly otherwise)
            lsum *= alpha;
            zacc *= alpha;
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
                const half2_t vv = bit_cast<half2_t>(vp[tt][r]);
                const float   pf = fast_exp2(__builtin_fmaf(sv[tt][r], sc, -msc));  // exp2(-inf) = +0 for a masked token
                lsum += pf;
                zacc                          = __builtin_fmaf(pf, (float)vv[1], zacc);
                pa[tt >> 1][(tt & 1) * 4 + r] = (half_t)(pf * (float)vv[0]);
            }
        }

        // ---- O = P' V on raw codes: k-slot (g, e) -> token 32a + 4g + e (e < 4) / 32a + 16 + 4g + e - 4 -----------------------------
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int   j    = i16 >> 1;
            const int   T    = 32 * a + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
            const char* vrow = Vt + T * D + (i16 & 1) * 8;
            const int   vs   = ws_vswz<D>(T);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                const v2i vb = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i*)(vrow + ((dt ^ vs) << 4)));
                const half8_t bq = ws_codes8_to_f16(u32x2{(uint32_t)vb[0], (uint32_t)vb[1]});
                O[dt]            = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa[a], bq, O[dt], 0, 0, 0);
            }
        }
    }

    // ---- per-wave totals, then merge the 4 waves through LDS ------------------------------------------------------------------------
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    zacc += __shfl_xor(zacc, 16);
    zacc += __shfl_xor(zacc, 32);

    __syncthreads();  // every wave is done with its images: the region is reused for the merge
    float* sm_o  = (float*)smem;                     // [4][16][D]
    float* sm_ml = (float*)(smem + 4 * 16 * D * 4);  // [4][16][2]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int   h  = 4 * g + r;
        const float za = __shfl(zacc, h);
        if (h < hpw) {
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt) {
                sm_o[(wave * 16 + h) * D + dt * 16 + i16] = __builtin_fmaf(O[dt][r], kWsTwo24, za);
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
        const int hq = head0 + h;
        if (p.splits == 1) {
            if (p.sinks) {  // the sink logit joins the denominator once and carries no value; exp2(-inf) = +0 changes no bit
                l += fast_exp2((float)p.sinks[hq] * 1.4426950408889634f - ms * sc);
            }
            p.out[(size_t)b * p.q_heads * D + (size_t)hq * D + d] = (half_t)(o / l);
        }
        else {  // decode_reduce_kernel merges the splits and adds the sink there; an empty split: m = -inf, l = 0, o = 0
            const size_t slot         = ((size_t)b * p.q_heads + hq) * p.splits + split;
            p.partial_o[slot * D + d] = o;
            if (d == 0) {
                p.partial_ml[slot * 2]     = ms;
                p.partial_ml[slot * 2 + 1] = l;
            }
        }
    }
}

template<int D, int BITS>
int launch_ws(const DecodeAttnParams& p, hipStream_t st)
{
    const int group = p.q_heads / p.cache.layout.kv_heads;
    int       hpw   = group;
    while (hpw > 16) {  // largest divisor of the GQA group that fits the 16 MFMA columns
        int d = 2;
        while (hpw % d) {
            ++d;
        }
        hpw /= d;
    }
    const int chunks = group / hpw;
    const dim3 grid(p.cache.layout.kv_heads * chunks, p.batch, p.splits);
    // 4 wave-private images; the merge buffers overlay them
    constexpr int lds = 4 * ws_wave_lds<D>();
    static_assert(lds >= 4 * 16 * D * 4 + 4 * 16 * 2 * 4, "merge buffers must fit");
    const auto K = decode_attention_ws_mfma_kernel<D, BITS>;
    if (const int rc = ensure_dynamic_lds((const void*)K, lds)) {
        return rc;
    }
    K<<<grid, 256, lds, st>>>(p, chunks, hpw);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

int launch_decode_attention_ws_mfma(const DecodeAttnParams& p, hipStream_t st)
{
    const KvLayout& L = p.cache.layout;
    TM_REQUIRE(L.bits == 8 || L.bits == 4, "window / sink MFMA decode attention: int8 / int4 KV only (fp16 and TurboQuant KV have kernels of their own)");
    TM_REQUIRE(L.head_dim == 64 || L.head_dim == 128, "window / sink MFMA decode attention: head_dim 64 or 128");
    TM_REQUIRE(L.block_len == 64 && L.kv_heads > 0 && p.q_heads % L.kv_heads == 0, "window / sink MFMA decode attention: block_len 64, q_heads % kv_heads");
    TM_REQUIRE(p.window >= 0, "window / sink MFMA decode attention: window must be >= 0 (0 = full attention)");
    TM_REQUIRE(!p.qkv_slabs && !p.qkv_f16, "window / sink MFMA decode attention is unfused: run kv_rope_store first");
    if (L.head_dim == 64) {
        return L.bits == 8 ? launch_ws<64, 8>(p, st) : launch_ws<64, 4>(p, st);
    }
    return L.bits == 8 ? launch_ws<128, 8>(p, st) : launch_ws<128, 4>(p, st);
}

}  // namespace tmk
