// Multi-head Latent Attention (DeepSeek-V2 / V3 / R1, Kimi-K2, MiniCPM3) in the absorbed form on a paged latent KV cache (gfx950):
// the cache store and one split-K flash attention kernel that serves decode, verify-sized rows and chunked prefill.
//
// Replaces: the reference's MLA arm -- invokeMLACopyQKV (src/turbomind/kernels/attention/mla_utils.cu), which expands the latent into
//           576-wide K rows, and the head_dim-576 decode kernel (decoding_sm80_576.cu: QK over 576, PV over the first 512).
//
// Geometry (fixed): kv_lora_rank Dc = 512, qk_rope_head_dim Dr = 64.  The cache holds ONE row per token, [c (512) | k_pe (64)] fp16 =
// 1152 bytes, and no V: every query head reads that row (an MQA group of H heads), as the K operand of S = Q row^T over all 576
// elements and as the V operand of O += P row[:512].  A layer inside a block is [64 tokens][576] fp16 (KvLayout{1, 576, 64, 16}).
// q is [rows][H][q_lat (512) | q_pe (64)] with q_lat = q_nope W_UK absorbed by the caller; out is the latent o_lat [rows][H * 512], the
// caller applies W_UV and o_proj.
//
// mla_kv_store_kernel: one wave per token row.  c = rmsnorm(kv_a[:512]) * w through norm_row (norm_row.h: the project's row arithmetic
// and its fp32 reduction), k_pe = rope(kv_a[512:]) and every head's q_pe rotated in place: pairs (2i, 2i + 1) by the (cos, sin) of
// table row min(pos, max_pos - 1), fp16 operation by operation as kv_rope_store_kernel states it.  F8 (the FP8 latent view of
// attention_mla_fp8.hip, 640-byte rows): the same fp16 c goes through a 1 KB LDS row and f8_quant8 (kv_cache_kernels.h), lane by lane.
//
// mla_attention_kernel.  Contract of launch_verify_attention: k_len[b] counts every row of the forward, hist = k_len[b] - q_len[b],
// row j sees the tokens t < hist + j + 1; q_len is unbounded.
//   Columns: a score column of the 16-wide MFMA tile is a (row j, head h) pair, column c = 16 chunk + i16 -> j = c / H, h = c % H
//     (attention_verify_mfma.hip with group = H).  H = 16: one decode token is exactly one chunk.  Columns >= q_len * H carry q = 0 and
//     are never written.  Each column has its own limit hist + j + 1, evaluated only in tiles that reach past hist + 1; tiles past the
//     largest limit of the chunk's columns are not visited at all (chunked prefill).
//   Work: a workgroup (4 waves) owns one sequence x one chunk x one split and walks the split's 64-token tiles oldest -> newest.  A tile
//     (72 KB) goes HBM -> registers (18 16-byte non-temporal loads per thread, issued for tile n + 1 before tile n is contracted) -> LDS
//     ONCE and feeds both contractions:
//       S^T = row Q^T : the waves split the 64 TOKENS, 16 each; A = 16 token rows by ds_read_b128, B = Q^T, the column's 576 elements
//                       resident in 72 VGPRs per lane; 18 k-steps of v_mfma_f32_16x16x32_f16.
//       column maxima (4 waves x 16) and P (fp16 [16 columns][64 tokens]) cross the waves through LDS;
//       O^T += row[:512]^T P^T : the waves split the 512 OUTPUT DIMS, 128 each = 8 floatx4 accumulators per lane; A = the transposed
//                       read ds_read_b64_tr_b16 of the same tile, B = P; 2 k-steps x 8 MFMAs.
//     An accumulator's lane holds column i16 in both products, so alpha and 1 / l apply without a shuffle.
//   Rows of the newest tile past the context are not loaded: their lanes re-read the last valid row, and the per-column mask turns their
//     scores into -inf.  A masked score gives P = exp2(-inf) = +0 by a select on the token index, whatever bytes the token's row holds.
//   Split-K: per column fp32 o[512] + (m, l); a split with no tile writes m = -inf, l = 0, o = 0; mla_reduce_kernel merges.
//
// LDS (76 288 B): tile [64][1152 B] | P [16][144 B] | wave maxima / sums [4][16] fp32.  ONE tile per workgroup and two workgroups per
// CU (152.6 of 160 KB), not a double buffer (144 KB + P, one workgroup per CU): the next tile already waits in registers, so a second
// LDS buffer would hide only the register -> LDS copy, while a second workgroup fills the matrix cores during this one's four barriers
// per tile and during its softmax; the register budget of two waves per SIMD (256) holds Q (72) + the staged tile (72) + O (32).
//
// Swizzle (bank = byte address / 4 mod 64, period 256 B).  A row is 1152 B = 4.5 periods, so consecutive rows start half a period
// apart: rows r and r + 1 together span the banks once per 16-byte chunk column, like the 128-byte rows of attention_decode_ws_mfma.hip,
// but the transposed read here fetches fp16 (4 rows x 32 B per 16 lanes), not bytes, and meets the K read in the SAME image, so neither
// of that file's terms carries over.  The 16-byte chunk index c (0 .. 71) of row r is stored at c ^ f(r),
//     f(r) = bit2(r) | bit1(r) << 1 | (bit3(r) ^ bit2(r)) << 2        (only the low three bits of c move: 72 = 9 x 8 chunks)
// and the slot of a chunk inside the period is 8 * bit0(r) + ((c ^ f(r)) & 7) (+ 8 for c & 8).
//   K read, ds_read_b128, lane (i16, g): row 16 wave + i16, chunk 4 dd + g.  If the hardware serves 16 consecutive lanes (one chunk, 16
//     rows): bit0(r) picks the half, f is a bijection of bits 1 .. 3 -> 16 slots.  If it serves {0-3, 12-15} of g with {4-11} of g + 1
//     (the grouping attention_vision.hip works with): rows {0, 2, 12, 14} give f = {0, 2, 1, 3}, rows {4, 6, 8, 10} give f ^ 1 = {4, 6, 5,
//     7} (the neighbour chunk flips bit 0) -> 8 slots per parity, 16 in all.  Conflict-free either way.
//   V read, ds_read_b64_tr_b16, 32 lanes = rows R0 + {0 .. 3, 8 .. 11}, 32 contiguous bytes (an aligned chunk pair) each: the pair's
//     octet is 4 * bit0(R) + ((c ^ f(R)) >> 1 & 3); over rows of one parity (bit1, bit3 ^ bit2) takes four values -> 8 octets.
//   The loader's ds_write_b128 covers chunks 0 .. 63 of ONE row (lane = chunk, XORed with a constant: a permutation of 1 KB of distinct
//   addresses, the minimum of four passes); the two tail instructions (chunks 64 .. 71 of eight rows each) were not analysed.  No counter
//   run has confirmed any of this.
#include "tm_common.h"
#include "tm_kernels.h"
#include "kv_cache_kernels.h"
#include "norm_row.h"

namespace tmk {

namespace {

#define MLA_GLOBAL_AS __attribute__((address_space(1)))
#define MLA_CONST_AS __attribute__((address_space(4)))
#define MLA_LDS_AS __attribute__((address_space(3)))

typedef short mla_v4s __attribute__((ext_vector_type(4)));

constexpr int kMlaRank     = 512;
constexpr int kMlaRope     = 64;
constexpr int kMlaRow      = kMlaRank + kMlaRope;  // 576 elements
constexpr int kMlaRowBytes = kMlaRow * 2;          // 1152
constexpr int kMlaChunks   = kMlaRowBytes / 16;    // 72 chunks of 16 bytes
constexpr int kMlaKSteps   = kMlaRow / 32;         // 18 MFMA k-steps of the score product
constexpr int kMlaTile     = 64 * kMlaRowBytes;    // 73 728 bytes
constexpr int kMlaStage    = 64 * kMlaChunks / 256;  // 18 chunks per thread and tile
constexpr int kMlaCols     = 16;
constexpr int kMlaPPitch   = 144;  // bytes of a P row: 64 tokens fp16 + 16
constexpr int kMlaLds      = kMlaTile + kMlaCols * kMlaPPitch + 4 * kMlaCols * 4;

// chunk swizzle term of token row r (file header)
__device__ __forceinline__ int mla_swz(int r)
{
    return ((r >> 2) & 1) | (r & 2) | ((((r >> 3) ^ (r >> 2)) & 1) << 2);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// store: one wave per token row
// ---------------------------------------------------------------------------------------------------------------------------------
template<bool F8>
__global__ __launch_bounds__(64) void mla_kv_store_kernel(const half_t* __restrict__ kv_a, int kv_stride, const half_t* __restrict__ norm_w,
                                                          float eps, half_t* __restrict__ q, int q_stride, int heads,
                                                          const int* __restrict__ cu_q_len, const int* __restrict__ k_len, int batch,
                                                          const half2_t* __restrict__ cos_sin, int max_pos, KvCacheView cache, float k_scale)
{
    constexpr int kRowBytes = F8 ? kMlaF8RowBytes : kMlaRowBytes;
    constexpr int kPeOff    = F8 ? kMlaRank : kMlaRank * 2;  // byte offset of k_pe in the cache row
    __shared__ float red[8];
    const int token = blockIdx.x;
    const int lane  = threadIdx.x;
    const int b     = find_seq(cu_q_len, batch, token);
    const int q_len = cu_q_len[b + 1] - cu_q_len[b];
    const int pos   = k_len[b] - q_len + (token - cu_q_len[b]);
    if (pos < 0) {
        return;  // workgroup-uniform; the entry point refuses k_len[b] < q_len[b] before it launches
    }
    const int blk = pos >> 6;
    char*     row = (char*)cache.block_ptrs[cache.cu_block_nums[b] + blk] + cache.layer_offset + (pos & 63) * kRowBytes;
    const half_t* src = kv_a + (size_t)token * kv_stride;

    // c = h(h(f32(x) * inv) * w) over the 512 latent elements: 64 vectors of 8, one per lane
    if constexpr (F8) {  // the lane quantises the 8 halves it wrote itself: no barrier
        __shared__ __attribute__((aligned(16))) half_t c16[kMlaRank];
        norm_row<0, false, 1>(c16, nullptr, src, nullptr, 0, nullptr, norm_w, eps, 1, kMlaRank, 0, lane, 64, red);
        *(u32x2*)(row + lane * 8) = f8_quant8(*(const half8_t*)(c16 + lane * 8), k_scale);
    }
    else {
        norm_row<0, false, 1>((half_t*)row, nullptr, src, nullptr, 0, nullptr, norm_w, eps, 1, kMlaRank, 0, lane, 64, red);
    }

    // k_pe (item `heads`) into the cache row, q_pe of every head in place: 8 lanes x 4 pairs per 64-wide rope part
    const int p = pos < max_pos ? pos : max_pos - 1;
    for (int it = lane; it < (heads + 1) * 8; it += 64) {
        const int     hh  = it >> 3;
        const int     c   = it & 7;
        const bool    isq = hh < heads;
        half_t*       qp  = q + (size_t)token * q_stride + (size_t)(isq ? hh : 0) * kMlaRow + kMlaRank + c * 8;
        const half_t* xp  = isq ? qp : src + kMlaRank + c * 8;
        half8_t       x   = *(const half8_t*)xp;
        if (cos_sin != nullptr) {  // grid-uniform
            const half8_t cs = *(const half8_t*)(cos_sin + (size_t)p * (kMlaRope / 2) + c * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // fp16 mul / sub / add, no fma (kv_rope_store_kernel)
                const half_t cc = cs[2 * i];
                const half_t s  = cs[2 * i + 1];
                const half_t x0 = x[2 * i];
                const half_t x1 = x[2 * i + 1];
                const half_t a0 = cc * x0;
                const half_t a1 = s * x1;
                const half_t b0 = cc * x1;
                const half_t b1 = s * x0;
                x[2 * i]        = a0 - a1;
                x[2 * i + 1]    = b0 + b1;
            }
        }
        *(half8_t*)(isq ? qp : (half_t*)(row + kPeOff) + c * 8) = x;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// attention
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void mla_attention_kernel(MlaAttnParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char*  Kt = smem;
    char*  Pm = smem + kMlaTile;
    float* sx = (float*)(Pm + kMlaCols * kMlaPPitch);  // [4 waves][16 columns]

    const int chunk = blockIdx.x;
    const int b     = blockIdx.y;
    const int split = blockIdx.z;
    const int H     = p.heads;

    const int q0    = *(const MLA_CONST_AS int*)(p.cu_q_len + b);
    const int q_len = *(const MLA_CONST_AS int*)(p.cu_q_len + b + 1) - q0;
    const int ctx   = *(const MLA_CONST_AS int*)(p.k_len + b);
    const long long ncols = (long long)q_len * H;
    const long long col0  = (long long)chunk * kMlaCols;
    if (col0 >= ncols || ctx < q_len) {  // a chunk past this sequence's columns (the grid is sized for the longest); workgroup-uniform
        return;
    }
    const int nv   = (int)(ncols - col0 < kMlaCols ? ncols - col0 : kMlaCols);  // live columns
    const int hist = ctx - q_len;

    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16  = lane & 15;
    const int g    = lane >> 4;

    // this lane's column: (row, head) and the first token it does NOT see
    const bool hv   = i16 < nv;
    const int  colj = hv ? (int)((col0 + i16) / H) : 0;
    const int  colh = hv ? (int)((col0 + i16) - (long long)colj * H) : 0;
    const int  lim  = hist + colj + 1;

    const int tiles      = (ctx + 63) >> 6;
    const int per_split  = (tiles + p.splits - 1) / p.splits;
    const int tile_begin = split * per_split;
    const int jmax       = (int)((col0 + nv - 1) / H);  // the chunk's newest row: no column sees a token at or past hist + jmax + 1
    const int tile_end   = min(tile_begin + per_split, (hist + jmax + 1 + 63) >> 6);

    const int       bstride = p.cache.block_stride;
    const uint64_t* blocks  = p.cache.block_ptrs
                             + (bstride > 0 ? (size_t)b * bstride : (size_t) * (const MLA_CONST_AS int*)(p.cache.cu_block_nums + b));

    // ---- the loader: the tile in flight, 18 chunks of 16 bytes per thread.  Wave w moves the token rows 16 w .. 16 w + 15: chunk `lane`
    // (0 .. 63) of row 16 w + it for it < 16 -- the row, its clamp and its swizzle term are wave-uniform, so an address is a scalar base
    // plus ONE lane term -- and chunk 64 + (lane & 7) of row 16 w + 8 k + (lane >> 3) for k < 2 ----
    u32x4     stg[kMlaStage];
    const int w16  = 16 * wave;
    const int lrow = lane >> 3, lc = lane & 7;
    auto      load_tile = [&](int tile) __attribute__((always_inline)) {
        const char* base = (const char*)*(const MLA_CONST_AS uint64_t*)(blocks + __builtin_amdgcn_readfirstlane(tile)) + p.cache.layer_offset;
        const int   last = min(63, ctx - tile * 64 - 1);  // rows past the context re-read the last valid row (masked below)
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const char* rp = base + min(w16 + it, last) * kMlaRowBytes;  // scalar
            stg[it]        = __builtin_nontemporal_load((const MLA_GLOBAL_AS u32x4*)(rp + lane * 16));
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int row = min(w16 + 8 * k + lrow, last);
            stg[16 + k]   = __builtin_nontemporal_load((const MLA_GLOBAL_AS u32x4*)(base + row * kMlaRowBytes + 1024 + lc * 16));
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
        char* wb = Kt + w16 * kMlaRowBytes;
#pragma unroll
        for (int it = 0; it < 16; ++it) {  // mla_swz(16 w + it) = mla_swz(it): a constant per instruction
            *(u32x4*)(wb + it * kMlaRowBytes + ((lane << 4) ^ (mla_swz(it) << 4))) = stg[it];
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int row = 8 * k + lrow;
            *(u32x4*)(wb + row * kMlaRowBytes + 1024 + ((lc ^ mla_swz(row)) << 4)) = stg[16 + k];
        }
    };

    const bool any_tile = tile_begin < tile_end;  // workgroup-uniform
    if (any_tile) {
        load_tile(tile_begin);
    }

    // Q^T fragments (B operand): lane (column i16, g) holds q[column][32 dd + 8 g .. + 8)
    half8_t qf[kMlaKSteps];
    {
        const half_t* qp = p.q + (size_t)(q0 + colj) * p.q_stride + (size_t)colh * kMlaRow + g * 8;
#pragma unroll
        for (int dd = 0; dd < kMlaKSteps; ++dd) {
            half8_t t = *(const MLA_GLOBAL_AS half8_t*)(qp + dd * 32);
            if (!hv) {
                t = half8_t{};
            }
            qf[dd] = t;
        }
    }

    floatx4 O[8];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
        O[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    float       m = -INFINITY, lsum = 0.f;  // column i16: m over every tile so far (the same in all lanes of the column), lsum over
    const float sc = p.scale_log2;          // this lane's tokens

    if (any_tile) {
        store_tile();
    }
    __syncthreads();

    for (int tile = tile_begin; tile < tile_end; ++tile) {
        const bool more = tile + 1 < tile_end;  // workgroup-uniform
        if (more) {
            load_tile(tile + 1);  // in flight while this tile is contracted
        }

        // ---- S^T = row Q^T: this wave's 16 tokens x 16 columns ----
        floatx4 S = {0.f, 0.f, 0.f, 0.f};
        {
            const int   tr = 16 * wave + i16;
            const char* kr = Kt + tr * kMlaRowBytes;
            const int   sw = mla_swz(tr);
            // chunk 4 dd + g: the swizzle moves its low three bits only -> two lane terms, the rest is an immediate offset
            const char* ke[2] = {kr + ((g ^ sw) << 4), kr + (((4 + g) ^ sw) << 4)};
#pragma unroll
            for (int dd = 0; dd < kMlaKSteps; ++dd) {
                const half8_t a = *(const half8_t*)(ke[dd & 1] + (dd >> 1) * 128);
                S               = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[dd], S, 0, 0, 0);
            }
        }
        // lane: S[r] = score of token 64 tile + 16 wave + 4 g + r against column i16
        float sv[4] = {S[0], S[1], S[2], S[3]};
        if (tile * 64 + 64 > hist + 1) {  // wave-uniform: the tile overlaps the forward's own rows or is the partial newest tile
            const int rel = lim - tile * 64;  // tokens of this tile the column sees
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (16 * wave + 4 * g + r >= rel) {
                    sv[r] = -INFINITY;
                }
            }
        }
        float tmax = fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3]));
        tmax       = fmaxf(tmax, __shfl_xor(tmax, 16));
        tmax       = fmaxf(tmax, __shfl_xor(tmax, 32));
        if (g == 0) {
            sx[wave * kMlaCols + i16] = tmax;
        }
        __syncthreads();  // (1) the four waves' column maxima
        tmax = fmaxf(fmaxf(sx[i16], sx[kMlaCols + i16]), fmaxf(sx[2 * kMlaCols + i16], sx[3 * kMlaCols + i16]));

        const float mnew  = fmaxf(m, tmax);
        const float alpha = (m == -INFINITY) ? 0.f : fast_exp2((m - mnew) * sc);
        // a column that has seen no token yet (its limit lies below this whole tile): offset 0, every weight exp2(-inf) = 0
        const float msc = mnew == -INFINITY ? 0.f : mnew * sc;
        half4_t     pv;
        float       psum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pf = fast_exp2(__builtin_fmaf(sv[r], sc, -msc));
            psum += pf;
            pv[r] = (half_t)pf;
        }
        lsum = lsum * alpha + psum;
        *(half4_t*)(Pm + i16 * kMlaPPitch + (16 * wave + 4 * g) * 2) = pv;
        if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m))) {  // wave-uniform: did any column's maximum move?
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                O[dt] *= alpha;  // an accumulator's column is the lane's own i16
            }
        }
        m = mnew;
        __syncthreads();  // (2) P of all 64 tokens

        // ---- O^T += row[:512]^T P^T: this wave's 128 output dims; lane (i16, g) receives V[32 a + 8 g + e][d0 + i16] ----
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const half8_t pb = *(const half8_t*)(Pm + i16 * kMlaPPitch + (32 * a + 8 * g) * 2);
            const int     R  = 32 * a + 8 * g + (i16 >> 2);
            const char*   r0 = Kt + R * kMlaRowBytes + 256 * wave + (i16 & 1) * 8;  // chunk 16 wave + 2 dt + h, h = (i16 & 3) >> 1
            const char*   r1 = r0 + 4 * kMlaRowBytes;
            const int     s0 = mla_swz(R), s1 = mla_swz(R + 4);
            const int     h  = (i16 & 3) >> 1;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {  // the swizzle moves chunk bits 0 .. 2 = (2 (dt & 3) + h); bit 3 = dt >> 2 is an immediate
                const int     lo = 2 * (dt & 3) + h;
                const half4_t v0 = bit_cast<half4_t>(
                    __builtin_amdgcn_ds_read_tr16_b64_v4i16((MLA_LDS_AS mla_v4s*)(r0 + ((lo ^ s0) << 4) + (dt >> 2) * 128)));
                const half4_t v1 = bit_cast<half4_t>(
                    __builtin_amdgcn_ds_read_tr16_b64_v4i16((MLA_LDS_AS mla_v4s*)(r1 + ((lo ^ s1) << 4) + (dt >> 2) * 128)));
                const half8_t vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                O[dt]            = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb, O[dt], 0, 0, 0);
            }
        }
        if (more) {
            __syncthreads();  // (3) every wave is done with the tile and with P
            store_tile();
            __syncthreads();  // (4) the next tile is complete
        }
    }

    // ---- column sums over the four waves; m is already the same everywhere ----
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    __syncthreads();  // the last reads of sx (maxima) are behind every wave
    if (g == 0) {
        sx[wave * kMlaCols + i16] = lsum;
    }
    __syncthreads();
    const float l = (sx[i16] + sx[kMlaCols + i16]) + (sx[2 * kMlaCols + i16] + sx[3 * kMlaCols + i16]);

    if (!hv) {
        return;  // padding column
    }
    const size_t rh = (size_t)(q0 + colj) * H + colh;  // (row, head)
    const int    d0 = 128 * wave + 4 * g;              // O[dt][r] is output dim d0 + 16 dt + r
    if (p.splits == 1) {
        const float inv = 1.0f / l;  // l > 0: token 0 is visible to every row
        half_t*     o   = p.out + rh * kMlaRank + d0;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            *(half4_t*)(o + dt * 16) = half4_t{(half_t)(O[dt][0] * inv), (half_t)(O[dt][1] * inv), (half_t)(O[dt][2] * inv), (half_t)(O[dt][3] * inv)};
        }
    }
    else {
        const size_t slot = rh * p.splits + split;
        float*       o    = p.partial_o + slot * kMlaRank + d0;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            *(floatx4*)(o + dt * 16) = O[dt];  // a split whose tiles the column does not see: m = -inf, o = l = 0
        }
        if (wave == 0 && g == 0) {
            p.partial_ml[slot * 2]     = m;
            p.partial_ml[slot * 2 + 1] = l;
        }
    }
}

// split-K merge: one 128-thread workgroup per (row, head), four output dims per thread
__global__ __launch_bounds__(128) void mla_reduce_kernel(MlaAttnParams p)
{
    const size_t rh   = (size_t)blockIdx.x * p.heads + blockIdx.y;
    const size_t slot = rh * p.splits;
    const int    d    = threadIdx.x * 4;
    float        ms   = -INFINITY;
    for (int s = 0; s < p.splits; ++s) {
        ms = fmaxf(ms, p.partial_ml[(slot + s) * 2]);
    }
    floatx4 o = {0.f, 0.f, 0.f, 0.f};
    float   l = 0.f;
    for (int s = 0; s < p.splits; ++s) {
        const float mw = p.partial_ml[(slot + s) * 2];
        const float wt = (mw == -INFINITY) ? 0.f : fast_exp2((mw - ms) * p.scale_log2);
        o += wt * *(const floatx4*)(p.partial_o + (slot + s) * kMlaRank + d);
        l += wt * p.partial_ml[(slot + s) * 2 + 1];
    }
    const float inv = 1.0f / l;
    *(half4_t*)(p.out + rh * kMlaRank + d) = half4_t{(half_t)(o[0] * inv), (half_t)(o[1] * inv), (half_t)(o[2] * inv), (half_t)(o[3] * inv)};
}

int mla_check_cache(const KvCacheView& c, bool f8_ok = false)
{
    const KvLayout& L = c.layout;
    TM_REQUIRE(L.head_dim == kMlaRow, "MLA: the latent cache row is kv_lora_rank 512 + qk_rope_head_dim 64 = head_dim 576");
    TM_REQUIRE(L.kv_heads == 1, "MLA: the latent cache has kv_heads 1 (every query head reads the same row)");
    TM_REQUIRE(L.bits == 16 || (f8_ok && L.bits == kKvBitsFp8), "MLA: latent cache of bits 16 (or TM_KV_BITS_FP8: attention_mla_fp8.hip)");
    TM_REQUIRE(L.block_len == 64, "MLA: block_len 64");
    TM_REQUIRE(c.block_ptrs && c.cu_block_nums, "null pointer");
    return 0;
}

}  // namespace

int launch_mla_kv_store(const half_t* kv_a, int kv_stride, const half_t* norm_w, float eps, half_t* q, int q_stride, int heads,
                        const int* cu_q_len, const int* k_len, int batch, int total_tokens, const half2_t* cos_sin, int max_pos,
                        KvCacheView cache, float k_scale, hipStream_t st)
{
    if (const int rc = mla_check_cache(cache, true)) {
        return rc;
    }
    TM_REQUIRE(kv_a && norm_w && q && cu_q_len && k_len, "null pointer");
    TM_REQUIRE(heads >= 1 && heads <= 128, "MLA: 1 <= H <= 128 query heads");
    TM_REQUIRE(kv_stride >= kMlaRow && kv_stride % 8 == 0 && (long long)q_stride >= (long long)heads * kMlaRow && q_stride % 8 == 0,
               "MLA store: kv_a rows hold 576 and q rows H * 576 elements, 16-byte aligned (stride % 8)");
    TM_REQUIRE(((uintptr_t)kv_a | (uintptr_t)q | (uintptr_t)norm_w | (uintptr_t)cos_sin) % 16 == 0, "MLA store: 16-byte aligned pointers");
    TM_REQUIRE(cos_sin == nullptr || max_pos >= 1, "MLA store: a RoPE table needs max_pos >= 1");
    TM_REQUIRE(batch >= 1 && total_tokens >= 0, "batch >= 1, total_tokens >= 0");
    const bool f8 = cache.layout.bits == kKvBitsFp8;
    TM_REQUIRE(!f8 || (k_scale > 0.f && k_scale <= 3.0e38f), "MLA store: k_scale of the FP8 latent cache must be finite and > 0");
    if (total_tokens == 0) {
        return 0;
    }
    const auto K = f8 ? mla_kv_store_kernel<true> : mla_kv_store_kernel<false>;
    K<<<total_tokens, 64, 0, st>>>(kv_a, kv_stride, norm_w, eps, q, q_stride, heads, cu_q_len, k_len, batch, cos_sin,
                                   cos_sin ? max_pos : 1 << 30, cache, k_scale);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mla_attention(const MlaAttnParams& p, hipStream_t st)
{
    if (const int rc = mla_check_cache(p.cache)) {
        return rc;
    }
    TM_REQUIRE(p.q && p.out && p.cu_q_len && p.k_len, "null pointer");
    TM_REQUIRE(p.heads >= 1 && p.heads <= 128, "MLA: 1 <= H <= 128 query heads");
    TM_REQUIRE(p.splits >= 1 && p.splits <= 128, "MLA attention: 1 <= splits <= 128");
    TM_REQUIRE(p.splits == 1 || (p.partial_o && p.partial_ml), "MLA attention: split-K needs a workspace");
    TM_REQUIRE(p.scale_log2 > 0.f, "MLA attention: softmax_scale must be > 0 (the latent width does not give it: 1 / sqrt(qk_nope + qk_rope), times mscale^2 under YaRN)");
    TM_REQUIRE((long long)p.q_stride >= (long long)p.heads * kMlaRow && p.q_stride % 8 == 0 && ((uintptr_t)p.q | (uintptr_t)p.out) % 16 == 0,
               "MLA attention: q rows hold H * 576 elements; q and out 16-byte aligned");
    TM_REQUIRE(p.batch >= 0 && p.batch <= 65535 && p.max_q_len >= 0 && p.rows >= 0, "MLA attention: 0 <= batch <= 65535");
    if (p.batch == 0 || p.rows == 0) {
        return 0;
    }
    const long long chunks = ((long long)p.max_q_len * p.heads + kMlaCols - 1) / kMlaCols;
    TM_REQUIRE(chunks <= 0x7fffffffLL, "MLA attention: q_len * H too large");
    const auto K = mla_attention_kernel;
    if (const int rc = ensure_dynamic_lds((const void*)K, kMlaLds)) {
        return rc;
    }
    K<<<dim3((unsigned)chunks, p.batch, p.splits), 256, kMlaLds, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    if (p.splits > 1) {
        mla_reduce_kernel<<<dim3(p.rows, p.heads), 128, 0, st>>>(p);
        TM_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

int launch_mla_reduce(const MlaAttnParams& p, hipStream_t st)
{
    mla_reduce_kernel<<<dim3(p.rows, p.heads), 128, 0, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
