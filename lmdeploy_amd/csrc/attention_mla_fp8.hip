// Multi-head Latent Attention in the absorbed form on an FP8 latent cache (gfx950): the split-K flash attention kernel that serves
// decode, verify-sized rows and chunked prefill on 640-byte rows, and the dequantising flatten of the expanded (prefill) form.
// The fp16 kernel is attention_mla.hip; this file shares its contract, its column rule and its split-K partials (mla_reduce_kernel
// merges them unchanged), and none of its data path.  The store is mla_kv_store_kernel<true> over there (it shares the RoPE code).
//
// Row (KvLayout{1, 576, 64, kKvBitsFp8}): 512 e4m3fn codes of c / k_scale, then the rotated k_pe as 64 fp16 = 640 bytes per token; a
// layer of a block is [64][640] = 40 960 bytes, no per-token parameters.  k_scale is the layer's one latent scale.
//
// Arithmetic.  A code byte widens in registers to the fp16 value code * 2^-8, exactly and always finite (f8_widen2, tm_common.h).  Q and
// P stay fp16; both products run on v_mfma_f32_16x16x32_f16 with fp32 accumulators:
//     S = softmax_scale * (k_scale * sum q_lat code + sum q_pe k_pe)        O = k_scale * sum P code / l
// kmul = k_scale * 2^8 multiplies the fp32 score accumulator ONCE, between the 16 latent and the 2 rope k-steps, and each output element
// once in the epilogue (before the 1 / l of splits == 1, or on the way into the partials).  No per-token multiply.  A masked score is
// selected to -inf, so P = +0 whatever bytes the token's row holds.
//
// mla_f8_attention_kernel.  Columns, limits, tile walk and split-K are attention_mla.hip's: a column is a (row j, head h) pair, 16 per
// workgroup; a workgroup (4 waves) owns one sequence x one chunk x one split and walks 64-token tiles oldest -> newest.  A tile (40 KB)
// goes HBM -> registers (10 16-byte non-temporal loads per thread, issued for tile n + 1 before tile n is contracted) -> LDS once, as
// BYTES, and feeds both contractions:
//     S^T = row Q^T : the waves split the 64 tokens, 16 each.  A = ds_read_b64 of one token row (8 codes), widened to 8 halves, 16
//                     k-steps; then * kmul; then 2 k-steps of ds_read_b128 on the fp16 tail.  B = Q^T, 72 VGPRs per lane, laid out as
//                     in the fp16 kernel (k-step dd, lane group g: elements 32 dd + 8 g .. + 8).
//     O^T += code^T P^T : the waves split the 512 output dims, 128 each.  A = ds_read_b64_tr_b8 of the same image (lane i16 receives
//                     channel 16 dt + i16 of the 8 token rows its 16-lane group addresses), widened; B = P.  k-slot (g, e) of k-step a
//                     is token 32 a + 4 g + e (e < 4) / 32 a + 16 + 4 g + e - 4: the byte-transposed read hands 8 rows to a 16-lane
//                     group, so P is read as two 4-token pieces.  2 k-steps x 8 MFMAs.
// Rows of the newest tile past the context are not loaded (their lanes re-read the last valid row; the mask removes their scores).
//
// Loader.  Wave w moves token rows 16 w .. 16 w + 15.  A row is 5 groups of 8 chunks (128 bytes = one cache line); instruction it
// (0 .. 9) moves group it / 2 of rows 8 (it & 1) + lane / 8, chunk lane % 8: per parity of `it` ONE lane term for the global address and
// one for the LDS address, the rest is an immediate.  Every 8 lanes read one aligned 128-byte line.
//
// LDS (43 520 B): image [64][640 B] | P [16][144 B] | wave maxima / sums [4][16] fp32.  TWO workgroups per CU, as the fp16 kernel, and
// for its reason: the next tile waits in registers, the other workgroup's MFMAs fill this one's four barriers and its softmax.  What the
// freed 32 KB of LDS and 32 VGPRs were meant to buy, and what the compiler said:
//   * a THIRD workgroup per CU (130.6 of 160 KB) needs 168 registers per lane.  Q (72) + staged tile (40) + O (32) = 144 are live across
//     the whole loop; the widening temporaries, the operands in flight and the addresses do not fit the remaining 24:
//     __launch_bounds__(256, 3) compiles to 168 VGPRs with 97 spilled (232 bytes of scratch per lane).  No scratch is the rule here, so
//     the kernel is built for two (234 VGPRs, no spill) and the third workgroup is NOT built.  It would take Q out of registers (18 KB of
//     LDS per workgroup: 3 x 61.9 KB > 160 KB) or a staged half tile; neither was tried.
//   * a 128-token tile (2 barriers per 64 tokens): 80 KB + P is one workgroup short of two per CU (2 x 84.7 KB > 160 KB) and the staged
//     tile would again cost 80 VGPRs.  Not built.
//   * a double-buffered image at two workgroups per CU: 2 x (80 KB + P) = 165 KB, 5 KB over; at one workgroup per CU it hides only the
//     register -> LDS copy (the fp16 file's argument).  Not built.
//   * K through registers only, as attention_decode_fp8_mfma.hip does: the image is needed for the transposed read anyway, and here all
//     four waves read every row of it (each wave its own output dims), so a register-only K would load the codes twice.  Not built.
// So the gain over the fp16 kernel is the bytes alone: 0.56 of the HBM traffic, of the LDS writes and of the LDS reads per tile, paid
// for with ~12 VALU instructions of widening per MFMA operand (32 operands per tile and wave).
//
// Swizzle (bank = byte address / 4 mod 64, period 256 B).  A row is 640 B = 2.5 periods: rows r and r + 1 start half a period apart,
// bit0(r) picks the half.  The 16-byte chunk c (0 .. 39) of row r is stored at c ^ f(r),
//     f(r) = bit1(r) | bit2(r) << 1 | (bit3(r) ^ bit4(r)) << 2              (the low three bits of c move: 40 = 5 x 8 chunks)
// so a chunk's slot in the half period is (c ^ f(r)) & 7.  The 1152-byte rule (bits 2, 1, 3 ^ 2) fails here: the byte-transposed read
// meets rows that differ in bit 4, which that term does not see; f8_vswz is built for 128-byte rows that all start at bank 0 or 32 with
// no K read in the same image.
//   K read, ds_read_b64, lane (i16, g): row 16 wave + i16, chunk 2 dd + g / 2, half g % 2.  32 lanes (g = 0, 1 or 2, 3) = 16 rows x one
//     whole chunk: bit 0 picks the half period, f is a bijection of bits 1 .. 3 (bit 4 = wave & 1 is fixed) onto its 8 slots -> 64
//     distinct banks.
//   V read, ds_read_b64_tr_b8, 16 lanes of group g = rows 32 a + {4 g .. 4 g + 3} and + 16, 16 bytes each (two lanes): row bits 0, 1, 4
//     vary.  32 lanes add bit 2; bit 3 (= g / 2) is fixed.  Rows of one parity: (bit1, bit2, bit4 ^ const) takes all 8 values -> 16 rows x
//     4 banks = 64 distinct banks.  These two reads are why f carries bit3 ^ bit4: each read fixes one of the two bits.
//   Rope read, ds_read_b128, lane (i16, g): row 16 wave + i16, chunk 32 + 4 s + g: 16 consecutive lanes = 16 rows x one chunk, distinct as
//     for the K read.  Two instructions per tile; other lane groupings were not analysed.
//   Store, ds_write_b128: 8 rows x 8 chunks (a permutation inside each row's half period): 1 KB of distinct addresses, four passes.
//   No counter run has confirmed any of this.
//
// Resource report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): mla_f8_attention_kernel 234 VGPRs, 0 AGPRs, 65
// SGPRs, scratch 0, no spills, occupancy 2 waves / SIMD, dynamic LDS 43 520 B; mla_f8_flatten_kernel 20 VGPRs, scratch 0, occupancy 8.
//
// mla_f8_flatten_kernel: one workgroup per (64-token block, sequence): code -> f16(f32(code) * k_scale) through load_dequant_flatten_f8
// (kv_cache_kernels.h: the FP8 KV cache's flatten rule), k_pe copied; fp16 [rows][576] out, rows past k_len untouched.
#include "tm_common.h"
#include "tm_kernels.h"
#include "kv_cache_kernels.h"

namespace tmk {

namespace {

#define MF8_GLOBAL_AS __attribute__((address_space(1)))
#define MF8_CONST_AS __attribute__((address_space(4)))
#define MF8_LDS_AS __attribute__((address_space(3)))

typedef int mf8_v2i __attribute__((ext_vector_type(2)));

constexpr int kF8Rank     = 512;
constexpr int kF8Row      = 576;                  // q elements per head, out elements of a flattened row
constexpr int kF8RowBytes = kMlaF8RowBytes;       // 640: 512 codes + 64 fp16
constexpr int kF8Tile     = 64 * kF8RowBytes;     // 40 960 bytes
constexpr int kF8Stage    = 64 * (kF8RowBytes / 16) / 256;  // 10 chunks per thread and tile
constexpr int kF8LatSteps = kF8Rank / 32;         // 16 k-steps on codes
constexpr int kF8Cols     = 16;
constexpr int kF8PPitch   = 144;  // bytes of a P row: 64 tokens fp16 + 16
constexpr int kF8Lds      = kF8Tile + kF8Cols * kF8PPitch + 4 * kF8Cols * 4;
constexpr int kF8WgPerCu  = 2;  // file header: three spill

// chunk swizzle term of token row r (file header)
__device__ __forceinline__ int mf8_swz(int r)
{
    return ((r >> 1) & 3) | ((((r >> 3) ^ (r >> 4)) & 1) << 2);
}

// 8 code bytes -> 8 fp16 lanes of code * 2^-8
__device__ __forceinline__ half8_t mf8_widen8(uint32_t w0, uint32_t w1)
{
    return bit_cast<half8_t>(u32x4{f8_widen2(w0, false), f8_widen2(w0, true), f8_widen2(w1, false), f8_widen2(w1, true)});
}

__global__ __launch_bounds__(256, kF8WgPerCu) void mla_f8_attention_kernel(MlaAttnParams p, float kmul)
{
    extern __shared__ __attribute__((aligned(128))) char smem[];
    char*  Kt = smem;
    char*  Pm = smem + kF8Tile;
    float* sx = (float*)(Pm + kF8Cols * kF8PPitch);  // [4 waves][16 columns]

    const int chunk = blockIdx.x;
    const int b     = blockIdx.y;
    const int split = blockIdx.z;
    const int H     = p.heads;

    const int q0    = *(const MF8_CONST_AS int*)(p.cu_q_len + b);
    const int q_len = *(const MF8_CONST_AS int*)(p.cu_q_len + b + 1) - q0;
    const int ctx   = *(const MF8_CONST_AS int*)(p.k_len + b);
    const long long ncols = (long long)q_len * H;
    const long long col0  = (long long)chunk * kF8Cols;
    if (col0 >= ncols || ctx < q_len) {  // a chunk past this sequence's columns (the grid is sized for the longest); workgroup-uniform
        return;
    }
    const int nv   = (int)(ncols - col0 < kF8Cols ? ncols - col0 : kF8Cols);  // live columns
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
                             + (bstride > 0 ? (size_t)b * bstride : (size_t) * (const MF8_CONST_AS int*)(p.cache.cu_block_nums + b));

    // ---- the loader (file header): 10 chunks of 16 bytes per thread ----
    u32x4     stg[kF8Stage];
    const int w16  = 16 * wave;
    const int lrow = lane >> 3, lc = lane & 7;
    auto      load_tile = [&](int tile) __attribute__((always_inline)) {
        const char* base = (const char*)*(const MF8_CONST_AS uint64_t*)(blocks + __builtin_amdgcn_readfirstlane(tile)) + p.cache.layer_offset;
        const int   last = min(63, ctx - tile * 64 - 1);  // rows past the context re-read the last valid row (masked below)
        const char* rp[2] = {base + min(w16 + lrow, last) * kF8RowBytes + lc * 16, base + min(w16 + 8 + lrow, last) * kF8RowBytes + lc * 16};
#pragma unroll
        for (int it = 0; it < kF8Stage; ++it) {
            stg[it] = __builtin_nontemporal_load((const MF8_GLOBAL_AS u32x4*)(rp[it & 1] + (it >> 1) * 128));
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
        const int r0 = w16 + lrow, r1 = r0 + 8;
        char*     wp[2] = {Kt + r0 * kF8RowBytes + ((lc ^ mf8_swz(r0)) << 4), Kt + r1 * kF8RowBytes + ((lc ^ mf8_swz(r1)) << 4)};
#pragma unroll
        for (int it = 0; it < kF8Stage; ++it) {
            *(u32x4*)(wp[it & 1] + (it >> 1) * 128) = stg[it];
        }
    };

    const bool any_tile = tile_begin < tile_end;  // workgroup-uniform
    if (any_tile) {
        load_tile(tile_begin);
    }

    // Q^T fragments (B operand): lane (column i16, g) holds q[column][32 dd + 8 g .. + 8); dd 16, 17 are q_pe
    half8_t qf[kF8LatSteps + 2];
    {
        const half_t* qp = p.q + (size_t)(q0 + colj) * p.q_stride + (size_t)colh * kF8Row + g * 8;
#pragma unroll
        for (int dd = 0; dd < kF8LatSteps + 2; ++dd) {
            half8_t t = *(const MF8_GLOBAL_AS half8_t*)(qp + dd * 32);
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
            const char* kr = Kt + tr * kF8RowBytes;
            const int   sw = mf8_swz(tr);
            // codes: chunk 2 dd + g / 2 -- the swizzle moves its low three bits 2 (dd & 3) + g / 2, dd / 4 is an immediate offset
            const char* kc = kr + (g & 1) * 8;
#pragma unroll
            for (int dd = 0; dd < kF8LatSteps; ++dd) {
                const u32x2 w = *(const u32x2*)(kc + (((2 * (dd & 3) + (g >> 1)) ^ sw) << 4) + (dd >> 2) * 128);
                S             = __builtin_amdgcn_mfma_f32_16x16x32_f16(mf8_widen8(w[0], w[1]), qf[dd], S, 0, 0, 0);
            }
            S *= kmul;  // the latent part leaves the code domain: k_scale * 2^8, once
#pragma unroll
            for (int s = 0; s < 2; ++s) {  // k_pe: chunk 32 + 4 s + g
                const half8_t a = *(const half8_t*)(kr + kF8Rank + (((4 * s + g) ^ sw) << 4));
                S               = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[kF8LatSteps + s], S, 0, 0, 0);
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
            sx[wave * kF8Cols + i16] = tmax;
        }
        __syncthreads();  // (1) the four waves' column maxima
        tmax = fmaxf(fmaxf(sx[i16], sx[kF8Cols + i16]), fmaxf(sx[2 * kF8Cols + i16], sx[3 * kF8Cols + i16]));

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
        *(half4_t*)(Pm + i16 * kF8PPitch + (16 * wave + 4 * g) * 2) = pv;
        if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m))) {  // wave-uniform: did any column's maximum move?
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                O[dt] *= alpha;  // an accumulator's column is the lane's own i16
            }
        }
        m = mnew;
        __syncthreads();  // (2) P of all 64 tokens

        // ---- O^T += code^T P^T: this wave's 128 output dims = chunks 8 wave .. 8 wave + 7 of every row ----
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const char*   pr = Pm + i16 * kF8PPitch + (32 * a + 4 * g) * 2;
            const half4_t p0 = *(const half4_t*)pr, p1 = *(const half4_t*)(pr + 32);
            const half8_t pb = {p0[0], p0[1], p0[2], p0[3], p1[0], p1[1], p1[2], p1[3]};
            const int     j  = i16 >> 1;  // the row this lane addresses for its 16-lane group: k-slot e = j
            const int     R  = 32 * a + 4 * g + (j & 3) + 16 * (j >> 2);
            const char*   vr = Kt + R * kF8RowBytes + 128 * wave + (i16 & 1) * 8;
            const int     vs = mf8_swz(R);
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const mf8_v2i vb = __builtin_amdgcn_ds_read_tr8_b64_v2i32((MF8_LDS_AS mf8_v2i*)(vr + ((dt ^ vs) << 4)));
                O[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(mf8_widen8((uint32_t)vb[0], (uint32_t)vb[1]), pb, O[dt], 0, 0, 0);
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
        sx[wave * kF8Cols + i16] = lsum;
    }
    __syncthreads();
    const float l = (sx[i16] + sx[kF8Cols + i16]) + (sx[2 * kF8Cols + i16] + sx[3 * kF8Cols + i16]);

    if (!hv) {
        return;  // padding column
    }
    const size_t rh = (size_t)(q0 + colj) * H + colh;  // (row, head)
    const int    d0 = 128 * wave + 4 * g;              // O[dt][r] is output dim d0 + 16 dt + r
    if (p.splits == 1) {
        const float inv = 1.0f / l;  // l > 0: token 0 is visible to every row
        half_t*     o   = p.out + rh * kF8Rank + d0;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            const floatx4 v          = O[dt] * kmul;  // back from the code domain, once per element
            *(half4_t*)(o + dt * 16) = half4_t{(half_t)(v[0] * inv), (half_t)(v[1] * inv), (half_t)(v[2] * inv), (half_t)(v[3] * inv)};
        }
    }
    else {
        const size_t slot = rh * p.splits + split;
        float*       o    = p.partial_o + slot * kF8Rank + d0;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            *(floatx4*)(o + dt * 16) = O[dt] * kmul;  // a split whose tiles the column does not see: m = -inf, o = l = 0
        }
        if (wave == 0 && g == 0) {
            p.partial_ml[slot * 2]     = m;
            p.partial_ml[slot * 2 + 1] = l;
        }
    }
}

// flatten: 72 items per token row -- 64 x 8 codes -> 8 halves, 8 x 16 bytes of k_pe
__global__ __launch_bounds__(256) void mla_f8_flatten_kernel(char* __restrict__ out, const int* __restrict__ cu_k_off,
                                                             const int* __restrict__ k_len, KvCacheView cache, float k_scale)
{
    const int b  = blockIdx.y;
    const int t0 = blockIdx.x * 64;
    const int n  = k_len[b];
    if (t0 >= n) {
        return;  // workgroup-uniform; the grid is sized for the longest context
    }
    const int   items = min(64, n - t0) * 72;
    const char* src   = (const char*)cache.block_ptrs[cache.cu_block_nums[b] + blockIdx.x] + cache.layer_offset;
    char*       dst   = out + ((size_t)cu_k_off[b] + t0) * (kF8Row * 2);
    for (int i = threadIdx.x; i < items; i += 256) {
        const int   row = i / 72, u = i - row * 72;
        const char* s   = src + row * kF8RowBytes;
        char*       d   = dst + (size_t)row * (kF8Row * 2) + u * 16;
        if (u < 64) {
            *(half8_t*)d = load_dequant_flatten_f8(s, u, k_scale);
        }
        else {
            *(u32x4*)d = *(const u32x4*)(s + kF8Rank + (u - 64) * 16);
        }
    }
}

int mf8_check_cache(const KvCacheView& c, float k_scale)
{
    const KvLayout& L = c.layout;
    TM_REQUIRE(L.head_dim == kF8Row && L.kv_heads == 1 && L.bits == kKvBitsFp8 && L.block_len == 64,
               "MLA FP8: the latent cache is kv_heads 1, head_dim 576 (kv_lora_rank 512 + qk_rope_head_dim 64), TM_KV_BITS_FP8, block_len 64");
    TM_REQUIRE(c.block_ptrs && c.cu_block_nums, "null pointer");
    TM_REQUIRE(c.layer_offset % 16 == 0, "MLA FP8: the layer must be 16-byte aligned");
    TM_REQUIRE(k_scale > 0.f && k_scale <= 3.0e38f, "MLA FP8: k_scale must be finite and > 0");
    return 0;
}

}  // namespace

int launch_mla_attention_fp8(const MlaAttnParams& p, float k_scale, hipStream_t st)
{
    if (const int rc = mf8_check_cache(p.cache, k_scale)) {
        return rc;
    }
    TM_REQUIRE(p.q && p.out && p.cu_q_len && p.k_len, "null pointer");
    TM_REQUIRE(p.heads >= 1 && p.heads <= 128, "MLA: 1 <= H <= 128 query heads");
    TM_REQUIRE(p.splits >= 1 && p.splits <= 128, "MLA attention: 1 <= splits <= 128");
    TM_REQUIRE(p.splits == 1 || (p.partial_o && p.partial_ml), "MLA attention: split-K needs a workspace");
    TM_REQUIRE(p.scale_log2 > 0.f, "MLA attention: softmax_scale must be > 0 (the latent width does not give it: 1 / sqrt(qk_nope + qk_rope), times mscale^2 under YaRN)");
    TM_REQUIRE((long long)p.q_stride >= (long long)p.heads * kF8Row && p.q_stride % 8 == 0 && ((uintptr_t)p.q | (uintptr_t)p.out) % 16 == 0,
               "MLA attention: q rows hold H * 576 elements; q and out 16-byte aligned");
    TM_REQUIRE(p.batch >= 0 && p.batch <= 65535 && p.max_q_len >= 0 && p.rows >= 0, "MLA attention: 0 <= batch <= 65535");
    if (p.batch == 0 || p.rows == 0) {
        return 0;
    }
    const long long chunks = ((long long)p.max_q_len * p.heads + kF8Cols - 1) / kF8Cols;
    TM_REQUIRE(chunks <= 0x7fffffffLL, "MLA attention: q_len * H too large");
    const auto K = mla_f8_attention_kernel;
    if (const int rc = ensure_dynamic_lds((const void*)K, kF8Lds)) {
        return rc;
    }
    K<<<dim3((unsigned)chunks, p.batch, p.splits), 256, kF8Lds, st>>>(p, k_scale * 256.0f);
    TM_HIP_CHECK(hipGetLastError());
    return p.splits > 1 ? launch_mla_reduce(p, st) : 0;
}

int launch_mla_flatten_fp8(half_t* lat_out, const int* cu_k_off, const int* k_len, int batch, int max_k_len, KvCacheView cache,
                           float k_scale, hipStream_t st)
{
    if (const int rc = mf8_check_cache(cache, k_scale)) {
        return rc;
    }
    TM_REQUIRE(lat_out && cu_k_off && k_len, "null pointer");
    TM_REQUIRE((uintptr_t)lat_out % 16 == 0, "tm_mla_flatten: lat_out must be 16-byte aligned");
    TM_REQUIRE(batch >= 0 && batch <= 65535 && max_k_len >= 0, "tm_mla_flatten: 0 <= batch <= 65535, max_k_len >= 0");
    if (batch == 0 || max_k_len == 0) {
        return 0;
    }
    mla_f8_flatten_kernel<<<dim3((max_k_len + 63) / 64, batch), 256, 0, st>>>((char*)lat_out, cu_k_off, k_len, cache, k_scale);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
