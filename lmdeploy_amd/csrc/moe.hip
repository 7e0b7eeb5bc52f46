// Mixture-of-experts routing for gfx950: router (gate) + top-k + routing tables + weighted combine.
//
// Replaces: MoeFfnLayerImpl::Gate, invokeMoeGate_V2 (softmax / top-k / norm_topk / routed_scale and the f2n / en2f /
// offsets tables) and invokeMoeCombine (src/turbomind/models/llama/moe_ffn_layer.cc:43-53,133-325;
// kernels/gemm/moe_utils_v2.cu:355-690).  The expert FFNs run as grouped GEMMs (gemm_w4a16.hip, `groups` descriptors)
// over the token rows listed per expert: u4 (AWQ) and fp16 experts in gemm_kernel's grouped mode, e4m3 experts on the fp8 matrix
// cores (gemm_fp8.hip; x and the gated-SiLU output are quantised per row first) or, with TM_FP8_MFMA=0, weight-only in gemm_kernel.
//   gate:   logits[t][e] = sum_h x[t][h] * Wg[h][e] in fp32; top-k on the logits (ties: lower expert id);
//           norm_topk: w_j = exp(l_j - max) / sum over the SELECTED experts, else softmax over all experts;
//           w_j *= routed_scale.
//   route:  for every expert the tokens that selected it, in ascending token order:
//           offsets[e] .. offsets[e+1] index the flat pair list; f2n[f] = token; en2f[j][t] = f.
//   combine: out[t] = fp16( sum_j w[t][j] * float(y[en2f[j][t]]) ).
//   gpt-oss block (lmdeploy/turbomind/models/gpt_oss.py; MoeBlock::act / gate_bias / b13 / b2, fp16 and MXFP4 experts): a router bias
//           (logit += bias[e] in fp32 before the top-k), per-expert biases on both linears and the clamped activation
//           gate * sigmoid(1.702 gate) * (1 + up) -- the w1w3 bias and the activation in the grouped GEMM's epilogue (gemm_mxfp4.hip),
//           the w2 bias per routed row in the combine (moe_combine_bias_kernel).  Off by default: nothing else launches differently.
//   shared expert (Qwen2-MoE; unified_decoder.cc:295-318, moe_ffn_layer.cc:295-325, moe_utils_v2.cu:1032-1105): the layer's dense
//           feed_forward output `shared` is scaled per token by sigmoid(x . w_shared_gate) and the routed sum is added on top, in
//           the same launch (moe_combine_shared_kernel): out[t] = fp16( float(shared[t]) * sigma_t + sum_j w[t][j] * float(y[..]) ).
// Two routers fill the same tables: the serial kernels (8-expert Mixtral, the default for experts <= 64) and the wide ones
// (moe_gate_wide_kernel / moe_route_wide_kernel, 1 <= experts <= 256: Qwen3-MoE), chosen by the expert count or TM_MOE_ROUTER.
#include "tm_common.h"
#include "tm_kernels.h"

#define TM_TRY_RC(expr)       \
    do {                     \
        const int _rc = (expr); \
        if (_rc) {           \
            return _rc;      \
        }                    \
    } while (0)

namespace tmk {

constexpr int kMaxExperts = 64;
constexpr int kMaxTopK    = 8;
constexpr int kMaxExpertsWide = 256;  // the wide router below

// one 256-thread workgroup per token; Wg fp16 [H][E] (input-major like every other weight)
// BIAS (gpt-oss router): logit[e] += bias[e], one fp32 add before the top-k; compiled out otherwise
template<bool BIAS>
__global__ __launch_bounds__(256) void moe_gate_kernel(int* __restrict__ topk_ids,      // [T][k]
                                                       float* __restrict__ topk_w,      // [T][k]
                                                       float* __restrict__ logits_out,  // [T][E] or nullptr
                                                       const half_t* __restrict__ x,
                                                       int ldx,
                                                       const half_t* __restrict__ wg,
                                                       int H,
                                                       int E,
                                                       int k,
                                                       int norm_topk,
                                                       float routed_scale,
                                                       const float* __restrict__ bias)
{
    __shared__ float part[4][kMaxExperts];
    __shared__ float logit[kMaxExperts];
    const int        t    = blockIdx.x;
    const int        lane = threadIdx.x & 63;
    const int        wave = threadIdx.x >> 6;
    const half_t*    xr   = x + (size_t)t * ldx;
    for (int e = 0; e < E; ++e) {
        float acc = 0.f;
        for (int h = threadIdx.x; h < H; h += 256) {
            acc = __builtin_fmaf((float)xr[h], (float)wg[(size_t)h * E + e], acc);
        }
        acc = group_sum<64>(acc);
        if (lane == 0) {
            part[wave][e] = acc;
        }
    }
    __syncthreads();
    if (threadIdx.x < E) {
        logit[threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if constexpr (BIAS) {
            logit[threadIdx.x] += bias[threadIdx.x];
        }
        if (logits_out) {
            logits_out[(size_t)t * E + threadIdx.x] = logit[threadIdx.x];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int      ids[kMaxTopK];
        float    val[kMaxTopK];
        uint64_t taken = 0;
        float    mx    = -INFINITY;
        for (int e = 0; e < E; ++e) {
            mx = fmaxf(mx, logit[e]);
        }
        for (int j = 0; j < k; ++j) {
            int   best = -1;
            float bv   = -INFINITY;
            for (int e = 0; e < E; ++e) {
                if (!((taken >> e) & 1) && (best < 0 || logit[e] > bv)) {
                    best = e;
                    bv   = logit[e];
                }
            }
            taken |= 1ull << best;
            ids[j] = best;
            val[j] = bv;
        }
        float denom = 0.f;
        if (norm_topk) {
            for (int j = 0; j < k; ++j) {
                denom += __builtin_expf(val[j] - mx);
            }
        }
        else {
            for (int e = 0; e < E; ++e) {
                denom += __builtin_expf(logit[e] - mx);
            }
        }
        const float inv = 1.0f / denom;
        for (int j = 0; j < k; ++j) {
            topk_ids[(size_t)t * k + j] = ids[j];
            topk_w[(size_t)t * k + j]   = __builtin_expf(val[j] - mx) * inv * routed_scale;
        }
    }
}

// single workgroup: routing tables.  offsets [E+1], f2n [T*k], en2f [k][T]
__global__ __launch_bounds__(1024) void moe_route_kernel(int* __restrict__ offsets, int* __restrict__ f2n, int* __restrict__ en2f,
                                                         const int* __restrict__ topk_ids, int T, int E, int k)
{
    __shared__ int s_scan[16];
    __shared__ int s_base;
    const int      tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        s_base     = 0;
        offsets[0] = 0;
    }
    __syncthreads();
    for (int e = 0; e < E; ++e) {
        int running = s_base;
        for (int t0 = 0; t0 < T; t0 += 1024) {
            const int t = t0 + tid;
            int       j = -1;
            if (t < T) {
                for (int q = 0; q < k; ++q) {
                    if (topk_ids[(size_t)t * k + q] == e) {
                        j = q;
                    }
                }
            }
            const int flag = j >= 0;
            int       x    = flag;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d);
                if (lane >= d) {
                    x += y;
                }
            }
            if (lane == 63) {
                s_scan[wave] = x;
            }
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < 16; ++w) {
                if (w < wave) {
                    before += s_scan[w];
                }
                total += s_scan[w];
            }
            if (flag) {
                const int f             = running + before + x - 1;
                f2n[f]                  = t;
                en2f[(size_t)j * T + t] = f;
            }
            running += total;
            __syncthreads();
        }
        if (tid == 0) {
            s_base         = running;
            offsets[e + 1] = running;
        }
        __syncthreads();
    }
}

// ---- wide router: 1 <= E <= 256 ------------------------------------------------------------------------------------------
// (value, lower id) arg-max exchange with the lane CTRL pairs this one with; every pairing is an involution, so both lanes of a
// pair end up with the same winner
__device__ __forceinline__ void argmax_take(float& v, int& id, float ov, int oid)
{
    if (ov > v || (ov == v && oid < id)) {
        v  = ov;
        id = oid;
    }
}
__device__ __forceinline__ void wave_argmax(float& v, int& id)
{
    argmax_take(v, id, dpp_f32<DPP_XOR1>(v), (int)dpp_u32<DPP_XOR1>((uint32_t)id));
    argmax_take(v, id, dpp_f32<DPP_XOR2>(v), (int)dpp_u32<DPP_XOR2>((uint32_t)id));
    argmax_take(v, id, dpp_f32<DPP_HMIRR>(v), (int)dpp_u32<DPP_HMIRR>((uint32_t)id));
    argmax_take(v, id, dpp_f32<DPP_ROR8>(v), (int)dpp_u32<DPP_ROR8>((uint32_t)id));
    argmax_take(v, id, __shfl_xor(v, 16), __shfl_xor(id, 16));
    argmax_take(v, id, __shfl_xor(v, 32), __shfl_xor(id, 32));
}
__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        v += __shfl_xor(v, d);
    }
    return v;
}

constexpr int kGateTile = 16;   // tokens per workgroup: Wg comes from L2 once per 16 tokens
constexpr int kLogitLd  = 260;  // fp32 row stride of the logit tile in LDS: rows 4g apart land 16 banks apart

// Gate + top-k in one launch.  One 256-thread workgroup per 16 tokens: logits[16][E] = x[16][H] . Wg[H][E] on
// v_mfma_f32_16x16x32_f16 (A = x: row = token, B = Wg: column = expert, 8 consecutive h per lane; fp32 accumulators), the 16-expert
// column tiles dealt round-robin to the four waves (NT = ceil(tiles / 4) <= 4 each, a template argument so that the k loop is
// branch-free and unrolls: four k-steps of loads are in flight per wave).  The tile goes to LDS once; then every wave selects for four tokens:
// a lane holds the logits of experts lane, lane + 64, lane + 128, lane + 192 and the k winners come from k wave-wide arg-max rounds.
// NaN logits (a NaN in x or Wg) are not ordered: no comparison replaces a NaN or takes one, so such a token may list an expert twice;
// its ids stay in [0, E) and the tables stay consistent (every pair is placed once), its output is NaN through the weights anyway.
// BIAS: as in moe_gate_kernel, added where the accumulators go to the logit tile.
template<int NT, bool BIAS>
__global__ __launch_bounds__(256) void moe_gate_wide_kernel(int* __restrict__ topk_ids,      // [T][k]
                                                            float* __restrict__ topk_w,      // [T][k]
                                                            float* __restrict__ logits_out,  // [T][E] or nullptr
                                                            const half_t* __restrict__ x,
                                                            int ldx,
                                                            const half_t* __restrict__ wg,
                                                            int T,
                                                            int H,
                                                            int E,
                                                            int k,
                                                            int norm_topk,
                                                            float routed_scale,
                                                            const float* __restrict__ bias)
{
    __shared__ float s_logit[kGateTile][kLogitLd];
    const int        lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int        col = lane & 15, g = lane >> 4;
    const int        t0     = blockIdx.x * kGateTile;
    const int        ntiles = (E + 15) >> 4;
    // rows past T repeat the last token (their logits are never read); columns past E read column 0 (never read either)
    const half_t* xr = x + (size_t)min(t0 + col, T - 1) * ldx + g * 8;
    const half_t* wr = wg + (size_t)(g * 8) * E;
    int           ecol[NT];
    floatx4       acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int e = (wave + 4 * i) * 16 + col;
        ecol[i]     = e < E ? e : 0;
        acc[i]      = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    for (int h0 = 0; h0 < H; h0 += 128) {  // H % 128 == 0: four 32-wide k-steps, their loads issued together
        half8_t a[4], b[4][NT];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u]            = *(const half8_t*)(xr + h0 + 32 * u);
            const half_t* w = wr + (size_t)(h0 + 32 * u) * E;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    b[u][i][j] = w[(size_t)j * E + ecol[i]];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[u], b[u][i], acc[i], 0, 0, 0);
            }
        }
    }
    // accumulator of a lane: rows (tokens) 4g .. 4g+3 of column (expert) tile * 16 + col
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (wave + 4 * i < ntiles) {  // wave-uniform: a wave's last tile may lie past E
            [[maybe_unused]] float be = 0.f;
            if constexpr (BIAS) {
                be = bias[ecol[i]];  // (columns past E read expert 0's: never read back)
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (BIAS) {
                    s_logit[4 * g + r][(wave + 4 * i) * 16 + col] = acc[i][r] + be;
                }
                else {
                    s_logit[4 * g + r][(wave + 4 * i) * 16 + col] = acc[i][r];
                }
            }
        }
    }
    __syncthreads();
    if (logits_out) {
        for (int idx = threadIdx.x; idx < kGateTile * E; idx += 256) {
            const int r = idx / E, e = idx - r * E;
            if (t0 + r < T) {
                logits_out[(size_t)(t0 + r) * E + e] = s_logit[r][e];
            }
        }
    }
    for (int rr = 0; rr < 4; ++rr) {
        const int r = wave * 4 + rr, t = t0 + r;
        if (t >= T) {  // wave-uniform
            break;
        }
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = lane + 64 * i < E ? s_logit[r][lane + 64 * i] : -INFINITY;
        }
        float all = 0.f;   // softmax over every expert (norm_topk == 0): needs the maximum, which is round 0's winner
        float mx = 0.f, sel_v = -INFINITY;
        int   sel_i = 0;
        for (int j = 0; j < k; ++j) {
            float bv = v[0];
            int   bi = lane;
#pragma unroll
            for (int i = 1; i < 4; ++i) {
                if (v[i] > bv) {
                    bv = v[i];
                    bi = lane + 64 * i;
                }
            }
            wave_argmax(bv, bi);
            if (j == 0) {
                mx = bv;
                if (!norm_topk) {
                    all = (__builtin_expf(v[0] - mx) + __builtin_expf(v[1] - mx)) + (__builtin_expf(v[2] - mx) + __builtin_expf(v[3] - mx));
                    all = group_sum<64>(all);
                }
            }
            if (lane == j) {
                sel_v = bv;
                sel_i = bi;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (bi == lane + 64 * i) {
                    v[i] = -INFINITY;
                }
            }
        }
        const float p     = lane < k ? __builtin_expf(sel_v - mx) : 0.f;
        const float denom = norm_topk ? group_sum<64>(p) : all;
        const float inv   = 1.0f / denom;
        if (lane < k) {
            topk_ids[(size_t)t * k + lane] = min(sel_i, E - 1);  // (in range whatever the logits are: the tables index by it)
            topk_w[(size_t)t * k + lane]   = p * inv * routed_scale;
        }
    }
}

// Routing tables, one workgroup per expert, no walk over E: the waves split the token-major pair list into contiguous segments.
// Pass 1 counts, per wave, the pairs of lower experts (-> offsets[e]) and of this expert; one barrier; pass 2 places this expert's
// pairs by __ballot + popcount prefix behind the waves before it, so the tokens of an expert come in ascending order and the
// tables are those of moe_route_kernel on the same ids.  No atomics: the placement does not depend on timing.
__global__ __launch_bounds__(1024) void moe_route_wide_kernel(int* __restrict__ offsets, int* __restrict__ f2n, int* __restrict__ en2f,
                                                              const int* __restrict__ topk_ids, int T, int E, int k)
{
    __shared__ int s_lt[16], s_eq[16];
    const int      e = blockIdx.x;
    const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int      P     = T * k;
    const int      seg   = ((P + waves - 1) / waves + 63) / 64 * 64;  // pairs per wave, whole 64-pair chunks
    const int      begin = min(wave * seg, P), end = min(begin + seg, P);
    int            lt = 0, eq = 0;
    for (int p0 = begin; p0 < end; p0 += 64) {
        const int p  = p0 + lane;
        const int id = p < end ? topk_ids[p] : E;
        lt += id < e;
        eq += id == e;
    }
    lt = wave_sum_i32(lt);
    eq = wave_sum_i32(eq);
    if (lane == 0) {
        s_lt[wave] = lt;
        s_eq[wave] = eq;
    }
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < waves; ++w) {
        base += s_lt[w] + (w < wave ? s_eq[w] : 0);
        total += s_lt[w];
    }
    if (threadIdx.x == 0) {
        offsets[e] = total;
        if (e == E - 1) {
            offsets[E] = P;
        }
    }
    for (int p0 = begin; p0 < end; p0 += 64) {
        const int      p    = p0 + lane;
        const bool     hit  = p < end && topk_ids[p] == e;
        const uint64_t mask = __ballot(hit);
        if (hit) {
            const int f = base + __popcll(mask & ((1ull << lane) - 1));
            const int t = p / k;
            f2n[f]      = t;
            en2f[(size_t)(p - t * k) * T + t] = f;
        }
        base += __popcll(mask);
    }
}

// out[t][h] = fp16( sum_j w[t][j] * y[en2f[j][t]][h] ); 8 columns per thread
__global__ __launch_bounds__(256) void moe_combine_kernel(half_t* __restrict__ out, int ldo, const half_t* __restrict__ y, int ldy,
                                                          const float* __restrict__ topk_w, const int* __restrict__ en2f, int T,
                                                          int H, int k)
{
    const int t = blockIdx.y;
    const int h = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (h >= H) {
        return;
    }
    float acc[8] = {};
    for (int j = 0; j < k; ++j) {
        const int     f = en2f[(size_t)j * T + t];
        const float   w = topk_w[(size_t)t * k + j];
        const half8_t v = *(const half8_t*)(y + (size_t)f * ldy + h);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[e] = __builtin_fmaf(w, (float)v[e], acc[e]);
        }
    }
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] = (half_t)acc[e];
    }
    *(half8_t*)(out + (size_t)t * ldo + h) = o;
}

// The combine of a block whose w2 linears have a bias (gpt-oss; moe_ffn_layer.cc:310-313): the bias of the row's expert is added to the
// routed row in fp16 first, then moe_combine_kernel's fp32 chain in the order j = 0..k-1:
//   out[t][h] = fp16( sum_j w[t][j] * f32( h(y[en2f[j][t]][h] + b2[topk_ids[t][j]][h]) ) )
// The expert of pair (t, j) is topk_ids[t][j] itself, so no flat-row -> expert table is needed and the route kernels stay as they are.
__global__ __launch_bounds__(256) void moe_combine_bias_kernel(half_t* __restrict__ out, int ldo, const half_t* __restrict__ y, int ldy,
                                                               const float* __restrict__ topk_w, const int* __restrict__ en2f,
                                                               const int* __restrict__ topk_ids, const half_t* __restrict__ b2, int T,
                                                               int H, int k)
{
    const int t = blockIdx.y;
    const int h = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (h >= H) {
        return;
    }
    float acc[8] = {};
    for (int j = 0; j < k; ++j) {
        const int     f = en2f[(size_t)j * T + t];
        const float   w = topk_w[(size_t)t * k + j];
        const int     x = topk_ids[(size_t)t * k + j];
        const half8_t v = *(const half8_t*)(y + (size_t)f * ldy + h) + *(const half8_t*)(b2 + (size_t)x * H + h);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[e] = __builtin_fmaf(w, (float)v[e], acc[e]);
        }
    }
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] = (half_t)acc[e];
    }
    *(half8_t*)(out + (size_t)t * ldo + h) = o;
}

// The combine of a block with a shared expert (Qwen2-MoE), gate and combine in ONE launch:
//   logit[t] = sum_h f32(x[t][h]) * f32(g[h]),  sigma = 1 / (1 + expf(-logit))   (expf overflow: 1 / inf = 0, no NaN)
//   out[t][h] = fp16( fma(w[t][k-1], y[..], ... fma(w[t][0], y[en2f[0][t]][h], f32(shared[t][h]) * sigma)) )
// i.e. moe_combine_kernel's chain started from the shared term instead of zero (MoeReduceKernel).  Same grid as moe_combine_kernel
// (2048 columns per workgroup); EVERY workgroup of a token computes the token's whole logit with one summation tree that does not
// depend on the grid: thread i sums its 8-channel chunks i, i + 256, ... in channel order (fma chain), the 64 lanes of a wave
// combine by the group_sum<64> butterfly, the four wave sums as (p0 + p1) + (p2 + p3) -- so all workgroups of a token, and all
// launches, scale by the same bits.  x and g come from L2 for every workgroup but the first (2 H bytes each per token).
// `out` may alias `shared` (the reference combines in place): a thread reads its 8 shared columns before it writes them.
__global__ __launch_bounds__(256) void moe_combine_shared_kernel(half_t* out, int ldo, const half_t* __restrict__ y, int ldy,
                                                                 const float* __restrict__ topk_w, const int* __restrict__ en2f,
                                                                 const half_t* shared, int lds, const half_t* __restrict__ x, int ldx,
                                                                 const half_t* __restrict__ g, int T, int H, int k)
{
    __shared__ float part[4];
    const int        t  = blockIdx.y;
    const half_t*    xr = x + (size_t)t * ldx;
    float            lg = 0.f;
    for (int c = threadIdx.x * 8; c < H; c += 256 * 8) {
        const half8_t xv = *(const half8_t*)(xr + c);
        const half8_t gv = *(const half8_t*)(g + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            lg = __builtin_fmaf((float)xv[e], (float)gv[e], lg);
        }
    }
    lg = group_sum<64>(lg);
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = lg;
    }
    __syncthreads();
    const float logit = (part[0] + part[1]) + (part[2] + part[3]);
    const float sigma = 1.0f / (1.0f + __builtin_expf(-logit));
    const int   h     = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (h >= H) {
        return;
    }
    const half8_t sv = *(const half8_t*)(shared + (size_t)t * lds + h);
    float         acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] = (float)sv[e] * sigma;
    }
    for (int j = 0; j < k; ++j) {
        const int     f = en2f[(size_t)j * T + t];
        const float   w = topk_w[(size_t)t * k + j];
        const half8_t v = *(const half8_t*)(y + (size_t)f * ldy + h);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            acc[e] = __builtin_fmaf(w, (float)v[e], acc[e]);
        }
    }
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] = (half_t)acc[e];
    }
    *(half8_t*)(out + (size_t)t * ldo + h) = o;
}

// TM_MOE_ROUTER: auto (default) = the serial kernels up to 64 experts and the wide ones above, wide = the wide ones for every
// expert count.  Read once; tm_debug_set_moe_router overrides it for A/B runs in one process (a plain global read by every launch:
// not thread-safe, for tests and the benchmark tool only, set while no forward is being enqueued).
static int g_moe_router_override = -1;
void moe_router_override(int mode)
{
    g_moe_router_override = mode;
}
bool moe_router_wide(int E)
{
    static const bool env_wide = [] {
        const char* v = getenv("TM_MOE_ROUTER");
        return v && std::string(v) == "wide";
    }();
    return E > kMaxExperts || (g_moe_router_override >= 0 ? g_moe_router_override == 1 : env_wide);
}

int launch_moe_gate(int* topk_ids, float* topk_w, float* logits_out, const half_t* x, int ldx, const half_t* wg, int T, int H,
                    int E, int k, bool norm_topk, float routed_scale, hipStream_t st, const float* bias)
{
    TM_REQUIRE(E >= 1 && E <= kMaxExpertsWide && k >= 1 && k <= kMaxTopK && k <= E, "moe: 1 <= top_k <= experts <= 256, top_k <= 8");
    if (T == 0) {
        return 0;
    }
    if (moe_router_wide(E)) {
        TM_REQUIRE(H % 128 == 0 && ldx % 8 == 0, "moe wide router: hidden % 128 == 0 and 16-byte aligned rows of x");
        const dim3 grid((T + kGateTile - 1) / kGateTile);
        const int  nt = ((E + 15) / 16 + 3) / 4;  // column tiles per wave
#define TM_GATE_WIDE(NT)                                                                                                                   \
    if (bias) {                                                                                                                            \
        moe_gate_wide_kernel<NT, true><<<grid, 256, 0, st>>>(topk_ids, topk_w, logits_out, x, ldx, wg, T, H, E, k, norm_topk ? 1 : 0,    \
                                                             routed_scale, bias);                                                        \
    }                                                                                                                                      \
    else {                                                                                                                                 \
        moe_gate_wide_kernel<NT, false><<<grid, 256, 0, st>>>(topk_ids, topk_w, logits_out, x, ldx, wg, T, H, E, k, norm_topk ? 1 : 0,   \
                                                              routed_scale, nullptr);                                                    \
    }
        if (nt == 1) {
            TM_GATE_WIDE(1);
        }
        else if (nt == 2) {
            TM_GATE_WIDE(2);
        }
        else if (nt == 3) {
            TM_GATE_WIDE(3);
        }
        else {
            TM_GATE_WIDE(4);
        }
#undef TM_GATE_WIDE
        TM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    if (bias) {
        moe_gate_kernel<true><<<T, 256, 0, st>>>(topk_ids, topk_w, logits_out, x, ldx, wg, H, E, k, norm_topk ? 1 : 0, routed_scale, bias);
    }
    else {
        moe_gate_kernel<false><<<T, 256, 0, st>>>(topk_ids, topk_w, logits_out, x, ldx, wg, H, E, k, norm_topk ? 1 : 0, routed_scale, nullptr);
    }
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_moe_route(int* offsets, int* f2n, int* en2f, const int* topk_ids, int T, int E, int k, hipStream_t st)
{
    if (moe_router_wide(E)) {
        // one workgroup per expert; four waves are enough to walk a decode-sized pair list
        moe_route_wide_kernel<<<E, (size_t)T * k <= 4096 ? 256 : 1024, 0, st>>>(offsets, f2n, en2f, topk_ids, T, E, k);
        TM_HIP_CHECK(hipGetLastError());
        return 0;
    }
    moe_route_kernel<<<1, 1024, 0, st>>>(offsets, f2n, en2f, topk_ids, T, E, k);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_moe_combine(half_t* out, int ldo, const half_t* y, int ldy, const float* topk_w, const int* en2f, int T, int H, int k,
                       hipStream_t st)
{
    TM_REQUIRE(H % 8 == 0, "moe combine: H % 8 == 0");
    if (T == 0) {
        return 0;
    }
    moe_combine_kernel<<<dim3((H / 8 + 255) / 256, T), 256, 0, st>>>(out, ldo, y, ldy, topk_w, en2f, T, H, k);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_moe_combine_bias(half_t* out, int ldo, const half_t* y, int ldy, const float* topk_w, const int* en2f, const int* topk_ids,
                            const half_t* b2, int T, int H, int k, hipStream_t st)
{
    TM_REQUIRE(H % 8 == 0 && ldo % 8 == 0 && ldy % 8 == 0, "moe combine: H and the row strides % 8 == 0");
    TM_REQUIRE(topk_ids && b2, "moe combine: the expert ids and the w2 biases");
    if (T == 0) {
        return 0;
    }
    moe_combine_bias_kernel<<<dim3((H / 8 + 255) / 256, T), 256, 0, st>>>(out, ldo, y, ldy, topk_w, en2f, topk_ids, b2, T, H, k);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_moe_combine_shared(half_t* out, int ldo, const half_t* y, int ldy, const float* topk_w, const int* en2f, const half_t* shared,
                              int lds, const half_t* x, int ldx, const half_t* gate, int T, int H, int k, hipStream_t st)
{
    TM_REQUIRE(H % 8 == 0 && ldo % 8 == 0 && ldy % 8 == 0 && lds % 8 == 0 && ldx % 8 == 0, "moe combine: H and the row strides % 8 == 0");
    TM_REQUIRE(shared && x && gate, "moe combine: shared expert output, x and the shared gate");
    if (T == 0) {
        return 0;
    }
    moe_combine_shared_kernel<<<dim3((H / 8 + 255) / 256, T), 256, 0, st>>>(out, ldo, y, ldy, topk_w, en2f, shared, lds, x, ldx, gate, T,
                                                                            H, k);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- one MoE FFN block (host object shared by the C-ABI operator and the engine) -------------------------------------
size_t moe_workspace_bytes(const MoeBlock& m, int tokens)
{
    const size_t pairs = (size_t)tokens * m.top_k;
    size_t       b     = 0;
    b += pairs * 4;                  // topk_ids
    b += pairs * 4;                  // topk_w
    b += (size_t)(m.experts + 1) * 4;  // offsets
    b += pairs * 4;                  // f2n
    b += pairs * 4;                  // en2f
    b  = (b + 255) / 256 * 256;
    b += pairs * m.inter * 2;        // act  [pairs][I]
    b  = (b + 255) / 256 * 256;
    b += pairs * m.hidden * 2;       // y2   [pairs][H]
    b  = (b + 255) / 256 * 256;
    // fp8 x fp8 experts: codes + scales of x (per token) and of the gated-SiLU output (per (token, expert) row); unused by u4 / fp16
    b += fp8_act_workspace_bytes(tokens, m.hidden) + fp8_act_workspace_bytes((int)pairs, m.inter);
    return b + 256;
}

int moe_prepare(MoeBlock& m, hipStream_t st)
{
    TM_REQUIRE((int)m.w13.size() == m.experts && (int)m.w2.size() == m.experts && m.gate, "moe: gate and every expert must be set");
    const int wt = m.w13[0].type;
    TM_REQUIRE((m.act == 0 && !m.b13 && !m.b2) || wt == 1 || wt == 3,
               "moe: the gpt-oss activation and expert biases are built for fp16 and MXFP4 experts only (not u4 / fp8)");
    TM_REQUIRE(m.act == 0 || m.act == 1, "moe: activation 0 (SiLU) or 1 (gpt-oss)");
    TM_REQUIRE((m.b13 != nullptr) == (m.b2 != nullptr), "moe: expert biases come for both linears (w1w3 and w2)");
    TM_REQUIRE(!m.b13 || m.act == 1, "moe: expert biases are built with the gpt-oss activation only");
    TM_REQUIRE(!m.shared_gate || (!m.b2 && m.act == 0), "moe: a shared expert with the gpt-oss activation or expert biases is not built");
    TM_REQUIRE(m.w13[0].fmt != LinearFormat::FP8_CHANNEL || (fp8_mfma_supported(m.w13[0]) && fp8_mfma_supported(m.w2[0])),
               "moe: channel-scaled fp8 experts run on the fp8 matrix cores only (TM_FP8_MFMA=0 is not offered for them)");
    TM_TRY_RC(moe_build_groups(&m.groups13, m.w13.data(), m.experts, st));
    TM_TRY_RC(moe_build_groups(&m.groups2, m.w2.data(), m.experts, st));
    if (fp8_mfma_supported(m.w13[0]) && fp8_mfma_supported(m.w2[0])) {  // device tables of the experts' P8 unit pointers
        std::vector<const void*> h13(m.experts), h2(m.experts);
        for (int e = 0; e < m.experts; ++e) {
            TM_REQUIRE(m.w13[e].packed8 && m.w2[e].packed8, "moe: fp8 expert without its P8 image");
            TM_REQUIRE(m.w13[e].fmt == m.w13[0].fmt && m.w2[e].fmt == m.w13[0].fmt,
                       "moe: fp8 experts of one block share one scale mode (block 128 or channel)");
            h13[e] = m.w13[e].packed8;
            h2[e]  = m.w2[e].packed8;
        }
        if (!m.groups13_p8) {
            TM_HIP_CHECK(hipMalloc(&m.groups13_p8, sizeof(void*) * m.experts));
            TM_HIP_CHECK(hipMalloc(&m.groups2_p8, sizeof(void*) * m.experts));
        }
        TM_HIP_CHECK(hipMemcpyAsync(m.groups13_p8, h13.data(), sizeof(void*) * m.experts, hipMemcpyHostToDevice, st));
        TM_HIP_CHECK(hipMemcpyAsync(m.groups2_p8, h2.data(), sizeof(void*) * m.experts, hipMemcpyHostToDevice, st));
        TM_HIP_CHECK(hipStreamSynchronize(st));
    }
    return 0;
}

// out[t] = sum_j w_j * W2_e( silu(W1_e x_t) * (W3_e x_t) ) over the top_k experts e of token t
// (+ sigmoid(x_t . shared_gate) * shared[t] when the block has a shared gate: `shared` [tokens][ld = ldo] is the shared expert's FFN
// output, required exactly then, read by the combine stage only, and may be `out`)
// `stages` (kMoeGate .. kMoeCombine) selects the launches: every one of them is a whole forward; a subset runs on the tables and
// activations an earlier forward left in the same workspace (tools/bench_moe_router.py times the launches one by one)
int moe_forward(const MoeBlock& m, half_t* out, int ldo, const half_t* x, int ldx, int tokens, void* workspace, int* topk_ids_out,
                float* topk_w_out, hipStream_t st, unsigned stages, const half_t* shared)
{
    TM_REQUIRE(m.groups13 && m.groups2, "moe: not prepared");
    TM_REQUIRE((m.shared_gate != nullptr) == (shared != nullptr),
               "moe: the shared expert's output is required exactly when the block has a shared gate");
    if (tokens == 0) {
        return 0;
    }
    const size_t pairs = (size_t)tokens * m.top_k;
    char*        w     = (char*)workspace;
    int*         ids   = (int*)w;
    float*       tw    = (float*)(w + pairs * 4);
    int*         offs  = (int*)(w + pairs * 8);
    int*         f2n   = offs + (m.experts + 1);
    int*         en2f  = f2n + pairs;
    size_t       o     = ((char*)(en2f + pairs) - w + 255) / 256 * 256;
    half_t*      act   = (half_t*)(w + o);
    o                  = (o + pairs * m.inter * 2 + 255) / 256 * 256;
    half_t*      y2    = (half_t*)(w + o);
    if (stages & kMoeGate) {
        TM_TRY_RC(launch_moe_gate(ids, tw, nullptr, x, ldx, m.gate, tokens, m.hidden, m.experts, m.top_k, m.norm_topk, m.routed_scale, st,
                                  m.gate_bias));
    }
    if (stages & kMoeRoute) {
        TM_TRY_RC(launch_moe_route(offs, f2n, en2f, ids, tokens, m.experts, m.top_k, st));
    }
    // expert FFNs: gathered rows of x -> act (gated SiLU fused) -> y2, both grouped over the experts
    const int hint = (int)((pairs + m.experts - 1) / m.experts);  // expected rows per expert
    if (m.groups13_p8) {
        // e4m3 experts on the fp8 matrix cores (the reference's fp8 path: QuantizeSymm + fp8 GEMM, LlamaLinear.cu:67-127):
        // x is quantised once per token, the gated-SiLU output once per (token, expert) row
        o                  = (o + pairs * m.hidden * 2 + 255) / 256 * 256;
        uint8_t*     xq    = (uint8_t*)(w + o);
        const int    ldsx1 = (tokens + 3) / 4 * 4;
        float*       sx1   = (float*)(xq + (size_t)tokens * m.hidden);
        o                  = (o + fp8_act_workspace_bytes(tokens, m.hidden) + 255) / 256 * 256;
        uint8_t*     aq    = (uint8_t*)(w + o);
        const int    ldsx2 = ((int)pairs + 3) / 4 * 4;
        float*       sx2   = (float*)(aq + pairs * m.inter);
        TM_REQUIRE(ldx == m.hidden || tokens == 1, "moe fp8: x must be row-contiguous");
        const bool chan = m.w13[0].fmt == LinearFormat::FP8_CHANNEL;  // channel-scaled experts: one activation scale per row, over all of K
        if (stages & kMoeW13) {
            TM_TRY_RC(chan ? launch_quant_fp8_token(xq, sx1, x, ldx, tokens, m.hidden, st)
                           : launch_quant_fp8_rows(xq, sx1, x, ldx, tokens, m.hidden, ldsx1, st));
            TM_TRY_RC(launch_linear_fp8_grouped(m.w13[0], m.groups13_p8, m.experts, xq, sx1, ldsx1, tokens, act, m.inter, tokens, hint, true,
                                                offs, f2n, st));
        }
        if (stages & kMoeW2) {
            TM_TRY_RC(chan ? launch_quant_fp8_token(aq, sx2, act, m.inter, (int)pairs, m.inter, st)
                           : launch_quant_fp8_rows(aq, sx2, act, m.inter, (int)pairs, m.inter, ldsx2, st));
            TM_TRY_RC(launch_linear_fp8_grouped(m.w2[0], m.groups2_p8, m.experts, aq, sx2, ldsx2, (int)pairs, y2, m.hidden, tokens, hint, false,
                                                offs, nullptr, st));
        }
    }
    else {
        if (stages & kMoeW13) {
            TM_TRY_RC(launch_linear_grouped(m.w13[0], m.groups13, m.experts, x, ldx, tokens, act, m.inter, tokens, hint, true, offs, f2n, st,
                                            m.act, m.b13));
        }
        if (stages & kMoeW2) {
            TM_TRY_RC(launch_linear_grouped(m.w2[0], m.groups2, m.experts, act, m.inter, (int)pairs, y2, m.hidden, tokens, hint, false, offs,
                                            nullptr, st));
        }
    }
    if ((stages & kMoeCombine) && m.shared_gate) {
        TM_TRY_RC(launch_moe_combine_shared(out, ldo, y2, m.hidden, tw, en2f, shared, ldo, x, ldx, m.shared_gate, tokens, m.hidden, m.top_k,
                                            st));
    }
    else if ((stages & kMoeCombine) && m.b2) {
        TM_TRY_RC(launch_moe_combine_bias(out, ldo, y2, m.hidden, tw, en2f, ids, m.b2, tokens, m.hidden, m.top_k, st));
    }
    else if (stages & kMoeCombine) {
        TM_TRY_RC(launch_moe_combine(out, ldo, y2, m.hidden, tw, en2f, tokens, m.hidden, m.top_k, st));
    }
    if (topk_ids_out) {
        TM_HIP_CHECK(hipMemcpyAsync(topk_ids_out, ids, pairs * 4, hipMemcpyDeviceToDevice, st));
    }
    if (topk_w_out) {
        TM_HIP_CHECK(hipMemcpyAsync(topk_w_out, tw, pairs * 4, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

void moe_free(MoeBlock& m)
{
    for (auto& l : m.w13) {
        linear_weight_free(l);
    }
    for (auto& l : m.w2) {
        linear_weight_free(l);
    }
    for (void* q : {(void*)m.gate, (void*)m.shared_gate, m.groups13, m.groups2, m.groups13_p8, m.groups2_p8, (void*)m.gate_bias, (void*)m.b13,
                    (void*)m.b2}) {
        if (q) {
            (void)hipFree(q);
        }
    }
    m.gate = m.shared_gate = nullptr;
    m.groups13 = m.groups2 = nullptr;
    m.groups13_p8 = m.groups2_p8 = nullptr;
    m.gate_bias = nullptr;
    m.b13 = m.b2 = nullptr;
}

}  // namespace tmk
