// Multi-head Latent Attention prefill in the EXPANDED form (gfx950): causal varlen flash attention at qk width 192 / v width 128 on
// v_mfma_f32_16x16x32_f16, and the gather that brings the paged latent rows into linear memory in front of the kv_b_proj expansion.
//
// Replaces: the 192-wide prefill arm the reference keeps next to its 576 decode arm -- dispatchAttention at head_dim 192 behind
//           invokeMLACopyQKV (src/turbomind/kernels/attention/mla_utils.cu, attention.cu).
//
// Why a second form: the absorbed kernel (attention_mla.hip) contracts 576 + 512 wide per (row, head, key), 2176 flop, and re-reads the
// latent history once per 16 (row, head) columns; per head k_nope = W_UK c and v = c W_UV cost one GEMM over the context and leave
// 2 (192 + 128) = 640 flop per (row, head, key).  Geometry (fixed): kv_lora_rank 512, qk_rope 64, qk_nope 128, v 128.
//
// mla_flatten_kernel: one workgroup per (64-token block, sequence).  A layer of a latent block is 64 contiguous 1152-byte rows and so is
// its destination, lat_out row cu_k_off[b] + 64 blk: min(64, k_len - 64 blk) * 72 chunks of 16 bytes are copied unchanged, one per lane
// and pass.  Rows past k_len[b] are not read and not written.
//
// mla_prefill_kernel.  Operands: q [rows][q_stride], head h at h * 192 = q_nope (128) | rotated q_pe (64); kv [tokens][kv_stride], head h
// at h * 256 = k_nope (128) | v (128), kv_b_proj's output as it stands (V is NOT transposed in memory); k_pe [tokens][pe_stride], 64
// wide, rotated, ONE row per token for all heads; out [rows][heads * 128].  Row j of sequence b sees the tokens t < hist + j + 1, hist =
// k_len[b] - q_len[b], at kv / k_pe row cu_k_off[b] + t.
//   Layout (attention_prefill.hip, attention_vision.hip): scores are computed transposed, S^T = K Q^T with K = k_nope | k_pe over 6
//     k-steps, so a lane's accumulator (column = query row, 4 consecutive keys) is, after exp2 and a cast, the B operand of O^T = V^T P^T
//     (8 output column tiles): P never leaves the registers.  Score tile A row 4g + r <-> key 8g + r, tile B <-> key 8g + 4 + r of a
//     32-key step: a lane's 8 probabilities are 8 consecutive keys.  V is row-major, so its A operand comes out of LDS through
//     ds_read_b64_tr_b16 (two reads = the lane's 8 keys of head-dim row 16 dt + i16).
//   Rows per wave: 32 = two 16-row column groups.  Q costs 2 x 24 VGPRs, O 2 x 32, and every K fragment (ds_read_b128) and V fragment
//     (two transposed reads) read from LDS feeds TWO MFMAs: per 32-key step and wave 12 + 16 LDS fragment reads stand against 24 + 16
//     MFMAs, where 16 rows per wave would pay the same reads for half the MFMAs.  A workgroup is 4 waves = 128 query rows of ONE head of
//     one sequence (not 64 = 2 waves: a stage is then shared by half as many rows, and the loader's 10 chunks per thread become 20).
//   Stages: 64 keys = 16 KB k_nope + 8 KB k_pe + 16 KB v = 40 KB, ONE 24 KB K tile of 384-byte rows (k_nope | k_pe) and one 16 KB V tile
//     of 256-byte rows.  A stage travels through REGISTERS: ten 16-byte global loads per thread (8 of the head's contiguous 512-byte
//     k_nope | v row, 2 of k_pe) for stage s + 1 are issued before stage s is contracted and written to the other LDS buffer behind
//     it -- not by LDS-DMA as in attention_prefill.hip: the 40 staging VGPRs are there (report below), the loader places every chunk
//     freely (the key permutations and both swizzles sit on the LDS write address, k_nope and v of one 512-byte row part into two
//     tiles), and rows past the workgroup's last visible key are simply never addressed.  TWO stages (80 KB), one barrier per stage;
//     two workgroups per CU take exactly the 160 KB and the register budget of two waves per SIMD.
//   The shared k_pe: a workgroup serving two heads of one query block would load the 8 KB k_pe tile and its 2 of 6 K fragments once
//     for both.  Not built: at 32 rows per wave a second head doubles Q and O to 224 VGPRs, which leaves no room for the stage in
//     flight, and at 16 rows per wave and two heads the k_nope and V fragments -- 22 of the 28 fragment reads per step -- lose the
//     reuse that 32 rows of one head give ALL 28.  The global side is served instead by the grid order: blockIdx.x is the head, so
//     the workgroups that run together read the same k_pe rows out of L2.
//   Causality: a workgroup visits the stages below kend = hist + its last row + 1 and nothing behind; stage rows at or past kend are
//     not loaded (their lanes re-read row kend - 1 <= k_len - 1: finite bytes under P = 0).  A wave skips a 32-key step at or past its
//     own last row's limit, and masks (select to -inf, P = exp2(-inf) = +0) only in steps that reach past its FIRST row's limit: steps
//     entirely in the wave's past take no mask.  The running maximum starts at attention_prefill.hip's finite kMinScore; every row
//     sees key 0 in the first step, so l > 0.
//   Work order, no work list and no read-back: grid = (heads, batch, ceil(max_q_len / 128)) and blockIdx.z counts query blocks from the
//     sequence's END, so the dispatcher (x fastest, z slowest) hands out every sequence's longest block first, then every second-longest,
//     ...; inside a sequence that is exactly longest-first, across sequences it is ordered by distance from the end, not by length.
//     Workgroups past a sequence's block count leave at once.  A sequence with k_len[b] < q_len[b] is skipped (nothing is read back
//     to refuse it): the call is asynchronous.
//
// Banks (rule: bank = byte address / 4 mod 64, period 256 B; a ds_read_b128 is served 16 lanes at a time, a 64-bit read 32).
//   K tile, 384-byte rows = 1.5 periods: consecutive rows start half a period apart, the situation of attention_mla.hip's 1152-byte
//     rows, and its term carries over: chunk c (0 .. 23) of tile row r is stored at c ^ f(r), f(r) = bit2(r) | bit1(r) << 1 |
//     (bit3(r) ^ bit2(r)) << 2 (the low three bits of c move: 24 = 3 x 8 chunks), slot in the period 8 (bit0(r) ^ bit3(c)) + ((c ^ f(r))
//     & 7).  Fragment read, lane (i16, g): row 32 sub + 16 tile + i16, chunk 4 dd + g.  16 consecutive lanes (one chunk, 16 rows): bit0
//     picks the half, f is a bijection of bits 1 .. 3.  The grouping {0-3, 12-15} of g with {4-11} of g + 1: rows {0, 2, 12, 14} give
//     f = {0, 2, 1, 3}, rows {4, 6, 8, 10} give f ^ 1 = {4, 6, 5, 7}; 8 slots per parity, 16 in all.  Conflict-free either way.
//   V tile, 256-byte rows = one period: every row starts at bank 0.  The loader swaps bits 2 and 3 of the key (attention_vision.hip),
//     so the 32 lanes of a transposed read address 8 CONSECUTIVE rows, 32 contiguous bytes (an aligned chunk pair = one octet of banks)
//     each; chunk c is stored at c ^ 2 (r & 7), i.e. pair dt at octet dt ^ (r & 7): eight rows, eight distinct octets.
//   The loader's ds_write_b128 were not analysed.  No counter run has confirmed any of this.
//
// Compiler report (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): mla_prefill_kernel 254 VGPRs, 0 AGPRs, 46 SGPRs,
// scratch 0, no spills, occupancy 2 waves / SIMD, dynamic LDS 81 920 B; mla_flatten_kernel 10 VGPRs, scratch 0, occupancy 8.
// Measured: 0.77 PFLOP/s at 640 flop per (row, head, key) on one 4096-token prompt of 128 heads (kernel trace).
#include "tm_common.h"
#include "tm_kernels.h"

namespace tmk {

namespace {

#define MLP_GLOBAL_AS __attribute__((address_space(1)))
#define MLP_LDS_AS __attribute__((address_space(3)))

typedef short    mlp_v4s __attribute__((ext_vector_type(4)));
typedef unsigned mlp_u32x2 __attribute__((ext_vector_type(2)));

constexpr float kMlpMinScore = -1.0e30f;  // finite start of the running maximum: see attention_prefill.hip

constexpr int kMlpNope   = 128;
constexpr int kMlpRope   = 64;
constexpr int kMlpV      = 128;
constexpr int kMlpQk     = kMlpNope + kMlpRope;  // 192
constexpr int kMlpKv     = kMlpNope + kMlpV;     // 256: a head's part of a kv row
constexpr int kMlpKSteps = kMlpQk / 32;          // 6
constexpr int kMlpVTiles = kMlpV / 16;           // 8
constexpr int kMlpKPitch = kMlpQk * 2;           // 384 bytes
constexpr int kMlpVPitch = kMlpV * 2;            // 256 bytes
constexpr int kMlpKTile  = 64 * kMlpKPitch;      // 24 576
constexpr int kMlpStage  = kMlpKTile + 64 * kMlpVPitch;  // 40 960
constexpr int kMlpLds    = 2 * kMlpStage;        // 81 920
constexpr int kMlpRows   = 128;                  // query rows of a workgroup
constexpr int kLatRowBytes = 576 * 2;

// max / sum over the lane pairs l ^ 16 and l ^ 32 by gfx950's row / half swaps (as in attention_prefill.hip)
__device__ __forceinline__ float mlp_max_xor16_xor32(float v)
{
    unsigned        b = __builtin_bit_cast(unsigned, v);
    const mlp_u32x2 r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    b = __builtin_bit_cast(unsigned, fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1])));
    const mlp_u32x2 q = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return fmaxf(__builtin_bit_cast(float, (unsigned)q[0]), __builtin_bit_cast(float, (unsigned)q[1]));
}
__device__ __forceinline__ float mlp_sum_xor16_xor32(float v)
{
    unsigned        b = __builtin_bit_cast(unsigned, v);
    const mlp_u32x2 r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    b                 = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]));
    const mlp_u32x2 q = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return __builtin_bit_cast(float, (unsigned)q[0]) + __builtin_bit_cast(float, (unsigned)q[1]);
}

// chunk swizzle term of K-tile row r (file header; attention_mla.hip's mla_swz)
__device__ __forceinline__ int mlp_swz(int r)
{
    return ((r >> 2) & 1) | (r & 2) | ((((r >> 3) ^ (r >> 2)) & 1) << 2);
}

__global__ __launch_bounds__(256) void mla_flatten_kernel(char* __restrict__ out, const int* __restrict__ cu_k_off,
                                                          const int* __restrict__ k_len, KvCacheView cache)
{
    const int b  = blockIdx.y;
    const int t0 = blockIdx.x * 64;
    const int n  = k_len[b];
    if (t0 >= n) {
        return;  // workgroup-uniform; the grid is sized for the longest context
    }
    const int    chunks = min(64, n - t0) * (kLatRowBytes / 16);
    const u32x4* src    = (const u32x4*)((const char*)cache.block_ptrs[cache.cu_block_nums[b] + blockIdx.x] + cache.layer_offset);
    u32x4*       dst    = (u32x4*)(out + ((size_t)cu_k_off[b] + t0) * kLatRowBytes);
    for (int i = threadIdx.x; i < chunks; i += 256) {
        dst[i] = src[i];
    }
}

__global__ __launch_bounds__(256, 2) void mla_prefill_kernel(MlaPrefillParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int head = blockIdx.x;
    const int b    = blockIdx.y;
    const int tid  = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16  = lane & 15;
    const int g    = lane >> 4;

    const int row0  = p.cu_q_len[b];
    const int q_len = p.cu_q_len[b + 1] - row0;
    const int ctx   = p.k_len[b];
    const int nblk  = (q_len + kMlpRows - 1) / kMlpRows;
    if ((int)blockIdx.z >= nblk || ctx < q_len) {
        return;  // workgroup-uniform: past this sequence's blocks (the grid is sized for the longest), or lengths that contradict
    }
    const int    qb   = nblk - 1 - (int)blockIdx.z;  // query blocks are handed out from the sequence's end: longest first
    const int    hist = ctx - q_len;
    const int    kend = hist + min(qb * kMlpRows + kMlpRows, q_len);  // keys the workgroup's last row sees; 1 <= kend <= ctx
    const size_t tok0 = (size_t)p.cu_k_off[b];

    const int  qw     = qb * kMlpRows + 32 * wave;          // the wave's first row
    const bool active = qw < q_len;                         // wave-uniform; an inactive wave still stages tiles and meets the barriers
    const int  wend   = hist + min(qw + 32, q_len);         // keys the wave's last row sees
    const int  wfree  = hist + qw + 1;                      // keys EVERY row of the wave sees

    // Q^T fragments (B operand) of the two 16-row groups: lane (j = query row, g) holds q[row][32 dd + 8g .. + 8)
    half8_t qf[2][kMlpKSteps];
    int     lim[2];
#pragma unroll
    for (int gr = 0; gr < 2; ++gr) {
        const int     row  = min(qw + 16 * gr + i16, q_len - 1);  // a padding column repeats the last row and is never written
        const half_t* qptr = p.q + (size_t)(row0 + row) * p.q_stride + (size_t)head * kMlpQk + g * 8;
        lim[gr]            = hist + row + 1;
#pragma unroll
        for (int dd = 0; dd < kMlpKSteps; ++dd) {
            qf[gr][dd] = *(const MLP_GLOBAL_AS half8_t*)(qptr + dd * 32);
        }
    }

    // ---- the loader: the stage in flight, ten 16-byte chunks per thread --------------------------------------------------------
    // kv: chunk c (0 .. 31) of key it * 8 + tid / 32 -- a wave reads two 512-byte rows; k_pe: chunk c (0 .. 7) of key it * 32 + tid / 8
    u32x4         kvx[8], pex[2];
    const half_t* kvb = p.kv + (size_t)head * kMlpKv;
    auto stage_load = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const size_t tok = tok0 + min(ks + it * 8 + (tid >> 5), kend - 1);
            kvx[it]          = *(const MLP_GLOBAL_AS u32x4*)(kvb + tok * p.kv_stride + (tid & 31) * 8);
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const size_t tok = tok0 + min(ks + it * 32 + (tid >> 3), kend - 1);
            pex[it]          = *(const MLP_GLOBAL_AS u32x4*)(p.k_pe + tok * p.pe_stride + (tid & 7) * 8);
        }
    };
    // K tile row of a key = its score-tile row (key 32s + 8q + 4t + j -> row 32s + 16t + 4q + j), V tile row = key bits 2 and 3 swapped
    auto krow = [](int key) { return (key & 32) | ((key & 4) << 2) | ((key & 24) >> 1) | (key & 3); };
    auto stage_store = [&](int buf) __attribute__((always_inline)) {
        char* kt = smem + buf * kMlpStage;
        char* vt = kt + kMlpKTile;
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int key = it * 8 + (tid >> 5), c = tid & 31;
            const int kr  = krow(key);
            const int vr  = (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1);
            char*     ka  = kt + kr * kMlpKPitch + ((c ^ mlp_swz(kr)) << 4);                // c < 16: k_nope chunk c
            char*     va  = vt + vr * kMlpVPitch + (((c - 16) ^ ((vr & 7) << 1)) << 4);     // c >= 16: v chunk c - 16
            *(u32x4*)(c < 16 ? ka : va) = kvx[it];
        }
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int key = it * 32 + (tid >> 3), c = tid & 7;
            const int kr  = krow(key);
            *(u32x4*)(kt + kr * kMlpKPitch + ((16 + (c ^ mlp_swz(kr))) << 4)) = pex[it];
        }
    };

    floatx4 O[2][kMlpVTiles];
#pragma unroll
    for (int gr = 0; gr < 2; ++gr) {
#pragma unroll
        for (int dt = 0; dt < kMlpVTiles; ++dt) {
            O[gr][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
    }
    float       m[2] = {kMlpMinScore, kMlpMinScore}, l[2] = {0.f, 0.f};
    const float sc   = p.scale_log2;

    // lane terms of the fragment addresses
    const int ksw   = mlp_swz(i16);                                      // = mlp_swz(i16 + 16) = mlp_swz(i16 + 32 sub)
    const int koff0 = i16 * kMlpKPitch + ((g ^ ksw) << 4);               // chunk 4 dd + g, dd even
    const int koff1 = i16 * kMlpKPitch + (((4 + g) ^ ksw) << 4);         //                 dd odd
    const int vrow  = 16 * (g >> 1) + 4 * (g & 1) + (i16 >> 2);          // + 32 sub (+ 8): keys 8g (+ 4) + (i16 >> 2)
    const int voff  = vrow * kMlpVPitch + (i16 & 3) * 8;
    const int vsw   = vrow & 7;

    stage_load(0);
    stage_store(0);
    __syncthreads();
    int buf = 0;
    for (int ks0 = 0; ks0 < kend; ks0 += 64, buf ^= 1) {
        const bool more = ks0 + 64 < kend;  // workgroup-uniform
        if (more) {
            stage_load(ks0 + 64);  // in flight while this stage is contracted
        }
        const char* kt = smem + buf * kMlpStage;
        const char* vt = kt + kMlpKTile;
#pragma nounroll
        for (int sub = 0; sub < 2; ++sub) {
            const int ks = ks0 + 32 * sub;
            if (!active || ks >= wend) {  // wave-uniform: no row of the wave sees this step
                continue;
            }
            // ---- S^T = K Q^T: 2 score tiles x 2 row groups, every K fragment feeds two MFMAs ----
            floatx4 s4[2][2];
#pragma unroll
            for (int gr = 0; gr < 2; ++gr) {
                s4[gr][0] = floatx4{0.f, 0.f, 0.f, 0.f};
                s4[gr][1] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
            {
                const char* ra = kt + 32 * sub * kMlpKPitch;
#pragma unroll
                for (int dd = 0; dd < kMlpKSteps; ++dd) {
                    const char*   fa = ra + ((dd & 1) ? koff1 : koff0) + (dd >> 1) * 128;
                    const half8_t ka = *(const half8_t*)fa;
                    const half8_t kb = *(const half8_t*)(fa + 16 * kMlpKPitch);
#pragma unroll
                    for (int gr = 0; gr < 2; ++gr) {
                        s4[gr][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, qf[gr][dd], s4[gr][0], 0, 0, 0);
                        s4[gr][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kb, qf[gr][dd], s4[gr][1], 0, 0, 0);
                    }
                }
            }
            // ---- online softmax per group; lane holds S[key ks + 8g + e][row i16] ----
            const bool masked = ks + 32 > wfree;  // wave-uniform: the step reaches past the first row's limit
            half8_t    pf[2];
#pragma unroll
            for (int gr = 0; gr < 2; ++gr) {
                float s[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[r]     = s4[gr][0][r];
                    s[4 + r] = s4[gr][1][r];
                }
                if (masked) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        s[e] = ks + 8 * g + e < lim[gr] ? s[e] : -INFINITY;
                    }
                }
                float tmax = s[0];
#pragma unroll
                for (int e = 1; e < 8; ++e) {
                    tmax = fmaxf(tmax, s[e]);
                }
                tmax              = mlp_max_xor16_xor32(tmax);
                const float mnew  = fmaxf(m[gr], tmax);  // finite (kMlpMinScore at least)
                const float alpha = fast_exp2((m[gr] - mnew) * sc);
                const float ms    = mnew * sc;
                float       psum  = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float pv = fast_exp2(__builtin_fmaf(s[e], sc, -ms));  // masked score: exp2(-inf) = 0
                    psum += pv;
                    pf[gr][e] = (half_t)pv;
                }
                l[gr] = l[gr] * alpha + psum;
                if (__builtin_amdgcn_readfirstlane((int)__any(mnew != m[gr]))) {  // wave-uniform: did any row's max move?
#pragma unroll
                    for (int dt = 0; dt < kMlpVTiles; ++dt) {
                        O[gr][dt] *= alpha;
                    }
                }
                m[gr] = mnew;
            }
            // ---- O^T += V^T P^T: the transposed read hands lane (i16, g) V[keys ks + 8g + 4h .. + 3][16 dt + i16]; two MFMAs each ----
            const char* vr = vt + 32 * sub * kMlpVPitch + voff;
#pragma unroll
            for (int dt = 0; dt < kMlpVTiles; ++dt) {
                const int     o  = (dt ^ vsw) << 5;
                const half4_t v0 = bit_cast<half4_t>(__builtin_amdgcn_ds_read_tr16_b64_v4i16((MLP_LDS_AS mlp_v4s*)(vr + o)));
                const half4_t v1 = bit_cast<half4_t>(__builtin_amdgcn_ds_read_tr16_b64_v4i16((MLP_LDS_AS mlp_v4s*)(vr + 8 * kMlpVPitch + o)));
                const half8_t vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
                for (int gr = 0; gr < 2; ++gr) {
                    O[gr][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[gr], O[gr][dt], 0, 0, 0);
                }
            }
        }
        if (more) {
            stage_store(buf ^ 1);  // every wave is past the barrier behind its reads of that buffer
        }
        __syncthreads();  // the next stage is complete, and everybody is done reading this one
    }

#pragma unroll
    for (int gr = 0; gr < 2; ++gr) {
        const float lh  = mlp_sum_xor16_xor32(l[gr]);  // all lanes: the swaps pair lanes of one column
        const int   row = qw + 16 * gr + i16;
        if (row < q_len) {
            const float inv  = 1.0f / lh;  // l > 0: token 0 is visible to every row
            half_t*     optr = p.out + ((size_t)(row0 + row) * p.heads + head) * kMlpV + g * 4;
#pragma unroll
            for (int dt = 0; dt < kMlpVTiles; ++dt) {
                *(half4_t*)(optr + dt * 16) = half4_t{(half_t)(O[gr][dt][0] * inv), (half_t)(O[gr][dt][1] * inv),
                                                      (half_t)(O[gr][dt][2] * inv), (half_t)(O[gr][dt][3] * inv)};
            }
        }
    }
}

}  // namespace

int launch_mla_flatten(half_t* lat_out, const int* cu_k_off, const int* k_len, int batch, int max_k_len, KvCacheView cache, hipStream_t st)
{
    const KvLayout& L = cache.layout;
    TM_REQUIRE(L.head_dim == 576 && L.kv_heads == 1 && L.bits == 16 && L.block_len == 64,
               "tm_mla_flatten: the latent cache is kv_heads 1, head_dim 576 (kv_lora_rank 512 + qk_rope_head_dim 64), bits 16, block_len 64");
    TM_REQUIRE(lat_out && cu_k_off && k_len && cache.block_ptrs && cache.cu_block_nums, "null pointer");
    TM_REQUIRE((uintptr_t)lat_out % 16 == 0 && cache.layer_offset % 16 == 0, "tm_mla_flatten: lat_out and the layer must be 16-byte aligned");
    TM_REQUIRE(batch >= 0 && batch <= 65535 && max_k_len >= 0, "tm_mla_flatten: 0 <= batch <= 65535, max_k_len >= 0");
    if (batch == 0 || max_k_len == 0) {
        return 0;
    }
    mla_flatten_kernel<<<dim3((max_k_len + 63) / 64, batch), 256, 0, st>>>((char*)lat_out, cu_k_off, k_len, cache);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_mla_prefill_attention(const MlaPrefillParams& p, hipStream_t st)
{
    TM_REQUIRE(p.out && p.q && p.kv && p.k_pe && p.cu_q_len && p.cu_k_off && p.k_len, "null pointer");
    TM_REQUIRE(p.heads >= 1 && p.heads <= 128, "MLA prefill: 1 <= H <= 128 query heads");
    TM_REQUIRE(p.scale_log2 > 0.f,
               "MLA prefill: softmax_scale must be > 0 (1 / sqrt(qk_nope + qk_rope), times mscale^2 under YaRN: the caller's to give)");
    TM_REQUIRE((long long)p.q_stride >= (long long)p.heads * kMlpQk, "MLA prefill: q_stride < heads * 192 (q_nope 128 | q_pe 64 per head)");
    TM_REQUIRE((long long)p.kv_stride >= (long long)p.heads * kMlpKv, "MLA prefill: kv_stride < heads * 256 (k_nope 128 | v 128 per head)");
    TM_REQUIRE(p.pe_stride >= kMlpRope, "MLA prefill: pe_stride < 64 (qk_rope_head_dim)");
    TM_REQUIRE(p.q_stride % 8 == 0 && p.kv_stride % 8 == 0 && p.pe_stride % 8 == 0
                   && ((uintptr_t)p.q | (uintptr_t)p.kv | (uintptr_t)p.k_pe | (uintptr_t)p.out) % 16 == 0,
               "MLA prefill: q, kv, k_pe and out rows must be 16-byte aligned (pointers % 16, strides % 8)");
    TM_REQUIRE(p.batch >= 0 && p.batch <= 65535 && p.max_q_len >= 0 && (p.max_q_len + kMlpRows - 1) / kMlpRows <= 65535,
               "MLA prefill: 0 <= batch <= 65535, 0 <= max_q_len <= 65535 * 128");
    if (p.batch == 0 || p.max_q_len == 0) {
        return 0;
    }
    const auto K = mla_prefill_kernel;
    if (const int rc = ensure_dynamic_lds((const void*)K, kMlpLds)) {
        return rc;
    }
    K<<<dim3(p.heads, p.batch, (p.max_q_len + kMlpRows - 1) / kMlpRows), 256, kMlpLds, st>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
