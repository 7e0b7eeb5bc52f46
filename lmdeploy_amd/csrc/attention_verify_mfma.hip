// Verify attention: split-K paged flash-decode for q_len[b] = 1 .. 8 query rows per sequence over int8 / int4 KV at head_dim 128 (gfx950)
// -- the attention of a speculative-decoding step, where every sequence carries its current token and up to 7 drafted ones.
//
// It is the non-fused instantiation of decode_attention_i8_mfma_kernel (attention_decode_mfma.hip; that file's header has the
// per-token (scale, zero) algebra, the subnormal-code contraction and the LDS image) with one change: a score column of the 16 x 16 MFMA
// tile is a (query row j, query head h) PAIR of one kv head instead of a head.  The decode kernel fills `group` of its 16 columns (4 for
// Llama-3-8B); here q_len * group columns are live, cut into chunks of 16 -- the same cache bytes and the same MFMA count per KV tile as one
// token while q_len * group <= 16.
//
// Contract (the prefill convention of launch_kv_rope_store): k_len[b] counts EVERY row of this forward and the rows' K / V are in the cache
// already (kv_store ran first; there is no fused prologue).  hist = k_len[b] - q_len[b]; query row j of sequence b sees the tokens
// t < hist + j + 1.  out is [rows][q_heads * D] in forward row order (row cu_q_len[b] + j).
//
// Column map: column c = 16 * chunk + i16 of kv head kvh is row j = c / group, head kvh * group + c % group; columns >= q_len * group carry
// q = 0 and are never written.  Each column has its own limit lim = hist + j + 1.  Only KV tiles that reach past hist + 1 -- the tiles that
// overlap [hist + 1, k_len), the sequence's partial newest tile among them -- evaluate the per-column mask (a wave-uniform branch, as the
// decode kernel's `partial`); every other tile runs the decode kernel's code.  A column whose limit lies below a whole tile (row 0 of a
// sequence whose rows straddle a block boundary) keeps m = -inf through that tile: the softmax offset is taken as 0 there, so exp2(-inf)
// = 0 and nothing is added.  Split-K partials ([rows][q_heads][splits]) and their merge are per column.
#include "tm_common.h"
#include "tm_kernels.h"
#include <type_traits>

namespace tmk {

namespace {

typedef int v2i __attribute__((ext_vector_type(2)));

// byte b -> fp16 bit pattern 0x00bb = b * 2^-24 (attention_decode_mfma.hip)
__device__ __forceinline__ half8_t codes8_to_f16_subnormal(u32x2 w)
{
    const uint32_t a0 = __builtin_amdgcn_perm(0u, w[0], 0x0c010c00u);
    const uint32_t a1 = __builtin_amdgcn_perm(0u, w[0], 0x0c030c02u);
    const uint32_t a2 = __builtin_amdgcn_perm(0u, w[1], 0x0c010c00u);
    const uint32_t a3 = __builtin_amdgcn_perm(0u, w[1], 0x0c030c02u);
    return bit_cast<half8_t>(u32x4{a0, a1, a2, a3});
}
constexpr float kScale24   = 16777216.0f;
constexpr int   kImageLds  = 16384 + 512;  // per wave: K image 8 KB | V image 8 KB | (k_param, v_param) per token
constexpr int   kCols      = 16;           // score columns of one workgroup

#define GLOBAL_AS __attribute__((address_space(1)))
#define CONST_AS __attribute__((address_space(4)))

// 32 int4 codes (cache order [0,2,4,6,1,3,5,7] per word) -> 32 bytes in element order (attention_decode_mfma.hip)
__device__ __forceinline__ void expand_nibbles32(u32x4 w, u32x4& a, u32x4& b)
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

template<int BITS>
__global__ __launch_bounds__(256, 2) void verify_attention_i8_mfma_kernel(VerifyAttnParams p, int chunks)
{
    static_assert(BITS == 8 || BITS == 4, "int8 / int4 KV");
    constexpr int D = 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    asm volatile("" ::"s"(p.q), "s"(p.q_stride), "s"(p.out), "s"(p.k_len), "s"(p.cu_q_len), "s"(p.q_heads), "s"(p.scale_log2), "s"(p.splits),
                 "s"(p.partial_o), "s"(p.partial_ml), "s"(p.cache.block_ptrs), "s"(p.cache.cu_block_nums), "s"(p.cache.block_stride),
                 "s"(p.cache.layer_offset), "s"(p.cache.layout.kv_heads), "s"(chunks));
    const KvLayout L = p.cache.layout;

    const int kv_head = blockIdx.x / chunks;
    const int chunk   = blockIdx.x - kv_head * chunks;
    const int b       = blockIdx.y;
    const int split   = blockIdx.z;
    const int group   = p.q_heads / L.kv_heads;

    const int q0    = *(const CONST_AS int*)(p.cu_q_len + b);
    const int q_len = min(*(const CONST_AS int*)(p.cu_q_len + b + 1) - q0, p.max_q_len);
    const int ctx   = *(const CONST_AS int*)(p.k_len + b);
    const int ncols = q_len * group;
    const int col0  = chunk * kCols;
    if (col0 >= ncols || ctx < q_len) {  // a chunk past this sequence's columns (the grid is sized for max_q_len rows); workgroup-uniform
        return;
    }
    const int nv   = min(kCols, ncols - col0);  // live columns of this workgroup
    const int hist = ctx - q_len;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i16  = lane & 15;
    const int g    = lane >> 4;

    char* Kt = smem + wave * kImageLds;
    char* Vt = Kt + 8192;
    char* Pm = Kt + 16384;

    const int       bstride = p.cache.block_stride;
    const uint64_t* blocks  = p.cache.block_ptrs
                             + (bstride > 0 ? (size_t)b * bstride : (size_t) * (const CONST_AS int*)(p.cache.cu_block_nums + b));
    auto block_ptr = [&](int tile) -> const char* {  // tile: wave-uniform
        return (const char*)*(const CONST_AS uint64_t*)(blocks + __builtin_amdgcn_readfirstlane(tile));
    };

    const int tiles      = (ctx + 63) >> 6;
    const int per_split  = (tiles + p.splits - 1) / p.splits;
    const int tile_begin = split * per_split;
    const int tile_end   = min(tile_begin + per_split, tiles);

    // this lane's column: (row, head) and the first token it does NOT see
    const bool hv   = i16 < nv;
    const int  colj = hv ? (col0 + i16) / group : 0;
    const int  colh = hv ? (col0 + i16) - colj * group : 0;
    const int  lim  = hist + colj + 1;

    half8_t qf[4];
    float   q1 = 0.f;  // sum_d q[column][d]

    floatx4 O[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
        O[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, lsum = 0.f, zacc = 0.f;  // per column i16, partial over this lane's tokens
    const float sc = p.scale_log2;

    const int koff  = L.k_data(kv_head, 0);
    const int voff  = L.v_data(kv_head, 0);
    const int kpoff = L.k_param(kv_head, 0);
    const int vpoff = L.v_param(kv_head, 0);

    constexpr int NR = BITS == 8 ? 8 : 4;  // 16-byte loads per lane per K (V) block
    u32x4    kreg[NR] = {}, vreg[NR] = {};
    uint32_t kpr = 0, vpr = 0;
    // FIRST: the first block a wave touches, the only one that can be the partial newest block: lanes past the context re-read the last
    // valid row (masked to nothing below).  Issued by every wave, branch-free (attention_decode_mfma.hip: load_tile)
    auto load_tile = [&](const char* blk, int tile, auto FIRST) {
        const char* base = blk + p.cache.layer_offset;
        const int   last = decltype(FIRST)::value ? (tile < tile_begin ? 0 : min(63, ctx - tile * 64 - 1)) : 63;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int row = BITS == 8 ? (lane >> 3) + 8 * r : (lane >> 2) + 16 * r;
            const int off = BITS == 8 ? min(row, last) * 128 + (lane & 7) * 16 : min(row, last) * 64 + (lane & 3) * 16;
            kreg[r]       = __builtin_nontemporal_load((const GLOBAL_AS u32x4*)(base + koff + off));
            vreg[r]       = __builtin_nontemporal_load((const GLOBAL_AS u32x4*)(base + voff + off));
        }
        kpr = *(const GLOBAL_AS uint32_t*)(base + kpoff + lane * 4);
        vpr = *(const GLOBAL_AS uint32_t*)(base + vpoff + lane * 4);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if constexpr (BITS == 8) {
                const int t   = (lane >> 3) + 8 * r;
                const int pos = t * 128 + (((lane & 7) ^ ((t >> 1) & 7)) << 4);
                *(u32x4*)(Kt + pos) = kreg[r];
                *(u32x4*)(Vt + pos) = vreg[r];
            }
            else {
                const int t  = (lane >> 2) + 16 * r;
                const int c  = (lane & 3) * 2;
                const int sw = (t >> 1) & 7;
                u32x4     a, b2;
                expand_nibbles32(kreg[r], a, b2);
                *(u32x4*)(Kt + t * 128 + ((c ^ sw) << 4))       = a;
                *(u32x4*)(Kt + t * 128 + (((c + 1) ^ sw) << 4)) = b2;
                expand_nibbles32(vreg[r], a, b2);
                *(u32x4*)(Vt + t * 128 + ((c ^ sw) << 4))       = a;
                *(u32x4*)(Vt + t * 128 + (((c + 1) ^ sw) << 4)) = b2;
            }
        }
        *(u32x2*)(Pm + lane * 8) = u32x2{kpr, vpr};
    };

    int         tile     = tile_end - 1 - wave;  // newest -> oldest, waves interleaved
    auto        in_range = [&](int t) { return max(min(max(t, tile_begin), tiles - 1), 0); };
    const char* ptr_cur  = block_ptr(in_range(tile));
    const char* ptr_next = block_ptr(in_range(tile - 4));
    load_tile(ptr_cur, tile, std::true_type{});
    {
        const half_t* qp = p.q + (size_t)(q0 + colj) * p.q_stride + (size_t)(kv_head * group + colh) * D;
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            half8_t t = *(const half8_t*)(qp + dd * 32 + g * 8);
            if (!hv) {
                t = half8_t{};
            }
            qf[dd] = t;
        }
    }
#pragma unroll
    for (int dd = 0; dd < 4; ++dd) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            q1 += (float)qf[dd][e];
        }
    }
    q1 += __shfl_xor(q1, 16);
    q1 += __shfl_xor(q1, 32);

    for (; tile >= tile_begin; tile -= 4) {
        store_tile();  // wave-private LDS: in-order DS pipeline, no barrier needed
        if (tile - 4 >= tile_begin) {
            load_tile(ptr_next, tile - 4, std::false_type{});
            ptr_next = block_ptr(in_range(tile - 8));
        }

        // ---- S^T = K q^T on raw codes ----
        floatx4 S[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            S[tt]       = floatx4{0.f, 0.f, 0.f, 0.f};
            const int t = 16 * tt + i16;
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {
                const int     u   = 4 * dd + g;
                const int     off = t * 128 + ((((u >> 1) ^ ((t >> 1) & 7))) << 4) + (u & 1) * 8;
                const u32x2   kb  = *(const u32x2*)(Kt + off);
                const half8_t a   = codes8_to_f16_subnormal(kb);
                S[tt]             = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[dd], S[tt], 0, 0, 0);
            }
        }

        // ---- scales, mask, online softmax (lane: column i16, tokens 16tt + 4g + r) ----
        uint32_t kp[4][4], vp[4][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const u32x4 pa_ = *(const u32x4*)(Pm + (16 * tt + 4 * g) * 8);
            const u32x4 pb_ = *(const u32x4*)(Pm + (16 * tt + 4 * g) * 8 + 16);
            kp[tt][0] = pa_[0], kp[tt][1] = pa_[2], kp[tt][2] = pb_[0], kp[tt][3] = pb_[2];
            vp[tt][0] = pa_[1], vp[tt][1] = pa_[3], vp[tt][2] = pb_[1], vp[tt][3] = pb_[3];
        }
        float sv[4][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const half2_t kk = bit_cast<half2_t>(kp[tt][r]);
                sv[tt][r]        = __builtin_fmaf((float)kk[0] * kScale24, S[tt][r], (float)kk[1] * q1);
            }
        }
        // wave-uniform: the tile reaches past the smallest limit of the sequence (hist + 1) -- it overlaps the forward's own rows or is the
        // partial newest tile: tokens at or behind the COLUMN's limit get score -inf and V params (0, 0) -> contribute exactly nothing
        const int rel = lim - tile * 64;  // tokens of this tile the column sees
        if (tile * 64 + 64 > hist + 1) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (16 * tt + 4 * g + r >= rel) {
                        sv[tt][r] = -INFINITY;
                        vp[tt][r] = 0u;
                    }
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
        if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m))) {
            lsum *= alpha;
            zacc *= alpha;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = __shfl(alpha, 4 * g + r);  // O rows are columns 4g + r
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) {
                    O[dt][r] *= ar;
                }
            }
        }
        m = mnew;
        // a column that has seen no token yet (its limit lies below this whole tile): offset 0, every weight exp2(-inf) = 0
        const float msc = mnew == -INFINITY ? 0.f : mnew * sc;

        half8_t pa[2];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const half2_t vv = bit_cast<half2_t>(vp[tt][r]);
                const float   pf = fast_exp2(__builtin_fmaf(sv[tt][r], sc, -msc));
                lsum += pf;
                zacc                          = __builtin_fmaf(pf, (float)vv[1], zacc);
                pa[tt >> 1][(tt & 1) * 4 + r] = (half_t)(pf * (float)vv[0]);
            }
        }

        // ---- O = P' V on raw codes: k-slot (g, e) -> token 32a + 4g + e (e<4) / 32a + 16 + 4g + e - 4 ----
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int   j    = i16 >> 1;
            const int   T    = 32 * a + (j < 4 ? 4 * g + j : 16 + 4 * g + (j - 4));
            const char* vrow = Vt + T * 128 + (i16 & 1) * 8;
            const int   swz  = (T >> 1) & 7;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const v2i vb = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                    (__attribute__((address_space(3))) v2i*)(vrow + ((dt ^ swz) << 4)));
                const half8_t bq = codes8_to_f16_subnormal(u32x2{(uint32_t)vb[0], (uint32_t)vb[1]});
                O[dt]            = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa[a], bq, O[dt], 0, 0, 0);
            }
        }
    }

    // ---- per-wave totals, then merge the 4 waves through LDS ----
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    zacc += __shfl_xor(zacc, 16);
    zacc += __shfl_xor(zacc, 32);

    __syncthreads();  // every wave is done with its K/V image: the region is reused for the merge
    float* sm_o  = (float*)smem;                        // [4][16][128]
    float* sm_ml = (float*)(smem + 4 * kCols * D * 4);  // [4][16][2]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int   h  = 4 * g + r;
        const float za = __shfl(zacc, h);
        if (h < nv) {
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                sm_o[(wave * kCols + h) * D + dt * 16 + i16] = __builtin_fmaf(O[dt][r], kScale24, za);
            }
        }
    }
    if (g == 0 && i16 < nv) {
        sm_ml[(wave * kCols + i16) * 2]     = m;
        sm_ml[(wave * kCols + i16) * 2 + 1] = lsum;
    }
    __syncthreads();

    for (int idx = threadIdx.x; idx < nv * D; idx += 256) {
        const int h  = idx / D;
        const int d  = idx - h * D;
        float     ms = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            ms = fmaxf(ms, sm_ml[(w * kCols + h) * 2]);
        }
        float o = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float mw = sm_ml[(w * kCols + h) * 2];
            const float wt = (mw == -INFINITY) ? 0.f : fast_exp2((mw - ms) * sc);
            o += wt * sm_o[(w * kCols + h) * D + d];
            l += wt * sm_ml[(w * kCols + h) * 2 + 1];
        }
        const int    j   = (col0 + h) / group;
        const int    hq  = kv_head * group + (col0 + h) - j * group;
        const size_t row = (size_t)(q0 + j);
        if (p.splits == 1) {
            p.out[(row * p.q_heads + hq) * D + d] = (half_t)(o / l);  // l > 0: token 0 is visible to every row
        }
        else {
            const size_t slot         = (row * p.q_heads + hq) * p.splits + split;
            p.partial_o[slot * D + d] = o;  // a split whose tiles the column does not see: ms = -inf, o = l = 0
            if (d == 0) {
                p.partial_ml[slot * 2]     = ms;
                p.partial_ml[slot * 2 + 1] = l;
            }
        }
    }
}

// split-K merge: one 128-thread workgroup per (query head, row j, sequence)
__global__ __launch_bounds__(128) void verify_reduce_kernel(VerifyAttnParams p)
{
    constexpr int D  = 128;
    const int     hq = blockIdx.x;
    const int     j  = blockIdx.y;
    const int     b  = blockIdx.z;
    const int     d  = threadIdx.x;
    const int     q0 = p.cu_q_len[b];
    if (j >= min(p.cu_q_len[b + 1] - q0, p.max_q_len) || p.k_len[b] < p.cu_q_len[b + 1] - q0) {
        return;
    }
    const size_t row  = (size_t)(q0 + j);
    const size_t slot = (row * p.q_heads + hq) * p.splits;
    float        ms   = -INFINITY;
    for (int s = 0; s < p.splits; ++s) {
        ms = fmaxf(ms, p.partial_ml[(slot + s) * 2]);
    }
    float o = 0.f, l = 0.f;
    for (int s = 0; s < p.splits; ++s) {
        const float mw = p.partial_ml[(slot + s) * 2];
        const float wt = (mw == -INFINITY) ? 0.f : fast_exp2((mw - ms) * p.scale_log2);
        o += wt * p.partial_o[(slot + s) * D + d];
        l += wt * p.partial_ml[(slot + s) * 2 + 1];
    }
    p.out[(row * p.q_heads + hq) * D + d] = (half_t)(o / l);
}

}  // namespace

int launch_verify_attention(const VerifyAttnParams& p, hipStream_t st)
{
    const KvLayout& L = p.cache.layout;
    TM_REQUIRE(L.head_dim == 128 && L.block_len == 64, "verify attention: head_dim 128, block_len 64");
    TM_REQUIRE(L.bits == 8 || L.bits == 4, "verify attention: int8 / int4 KV only (fp16 KV runs flatten + prefill attention)");
    TM_REQUIRE(p.q && p.out && p.cu_q_len && p.k_len, "null pointer");
    TM_REQUIRE(p.q_heads > 0 && L.kv_heads > 0 && p.q_heads % L.kv_heads == 0, "q_heads % kv_heads");
    TM_REQUIRE(p.max_q_len >= 1 && p.max_q_len <= kVerifyMaxRows, "verify attention: 1 <= q_len <= 8 rows per sequence");
    TM_REQUIRE(p.splits >= 1 && p.splits <= 128, "1 <= splits <= 128");
    TM_REQUIRE(p.splits == 1 || (p.partial_o && p.partial_ml), "split-K needs a workspace");
    if (p.batch == 0) {
        return 0;
    }
    const int group  = p.q_heads / L.kv_heads;
    const int chunks = (p.max_q_len * group + kCols - 1) / kCols;
    dim3      grid(L.kv_heads * chunks, p.batch, p.splits);
    static_assert(4 * kImageLds > 4 * kCols * 128 * 4 + 4 * kCols * 2 * 4, "merge buffers must fit");
    const int lds = 4 * kImageLds;
    if (L.bits == 4) {
        const auto K = verify_attention_i8_mfma_kernel<4>;
        if (const int rc = ensure_dynamic_lds((const void*)K, lds)) {
            return rc;
        }
        K<<<grid, 256, lds, st>>>(p, chunks);
    }
    else {
        const auto K = verify_attention_i8_mfma_kernel<8>;
        if (const int rc = ensure_dynamic_lds((const void*)K, lds)) {
            return rc;
        }
        K<<<grid, 256, lds, st>>>(p, chunks);
    }
    TM_HIP_CHECK(hipGetLastError());
    if (p.splits > 1) {
        verify_reduce_kernel<<<dim3(p.q_heads, p.max_q_len, p.batch), 128, 0, st>>>(p);
        TM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace tmk
