// Static-batch decode engine around the HIP kernels: the MI355X-native counterpart of
//   TurboMind::CreateEngine / ModelExecutor::Run / LanguageModel::Forward / UnifiedDecoder::Forward
//   (src/turbomind/turbomind.cc:281-361, engine/model_executor.cc:68-101, models/language_model.cc:493-542,
//    models/llama/unified_decoder.cc:163-380, unified_attention_layer.cc:365-441, LlamaFfnLayer.cc:28-91).
//
// One process per GPU.  All per-step state (context lengths, current token ids, generated tokens, step
// counter) lives in device memory so a whole decode step is a fixed kernel sequence that is captured ONCE in
// a hipGraph and replayed (the reference keeps ids on the device too: language_model.cc:540).  Tensor
// parallelism: column-parallel w_qkv / w1w3, row-parallel wo / w2 followed by an RCCL all-reduce of the
// fp16 [M,H] partial sums (comm/nccl/nccl.cu:356-398), lm_head sharded over the vocabulary with a
// (value, index) all-gather instead of gathering logits.
//
// This file: engine configuration, weight slots / synthetic weights / weight processing, start-up allocation, fetch / stats /
// destroy.  The forward pass lives in engine_forward.hip, collectives in engine_comm.hip, the start-up tuner in engine_tune.hip,
// continuous batching and the engine thread in engine_serve.hip (shared declarations: engine_internal.h).
#include "engine_internal.h"

namespace tmk {

// ---------------------------------------------------------------------------------------------
// device-side helpers for the engine
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// out[i] = h(mean + std * N(0,1)), counter-based (Box-Muller on splitmix64), 2 values per thread
__global__ void fill_normal_kernel(half_t* out, size_t n, float mean, float stddev, uint64_t seed)
{
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 2;
    if (i >= n) {
        return;
    }
    const uint64_t r  = splitmix64(seed ^ (i * 0x9E3779B97F4A7C15ull + 0x1234567ull));
    const float    u1 = ((float)(uint32_t)(r >> 40) + 1.0f) * (1.0f / 16777217.0f);  // (0,1)
    const float    u2 = (float)(uint32_t)((r >> 8) & 0xffffffu) * (1.0f / 16777216.0f);
    const float    rr = sqrtf(-2.0f * __logf(u1));
    float          s, c;
    __sincosf(6.283185307179586f * u2, &s, &c);
    out[i] = (half_t)(mean + stddev * rr * c);
    if (i + 1 < n) {
        out[i + 1] = (half_t)(mean + stddev * rr * s);
    }
}

__global__ void fill_fp8_kernel(uint8_t* out, size_t n, uint64_t seed)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull + seed * 0xD1B54A32D192ED03ull;
        z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        uint8_t b  = (uint8_t)(z >> 33);
        if ((b & 0x7f) == 0x7f) {
            b &= 0xf7;  // never NaN
        }
        out[i] = b;
    }
}

// synthetic MXFP4 experts: uniform code bytes, or scale bytes in {base - 1, base, base + 1}
__global__ void fill_mxfp4_kernel(uint8_t* out, size_t n, uint64_t seed, int scale_base)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint64_t z = splitmix64(seed ^ ((i + 1) * 0x9E3779B97F4A7C15ull));
        out[i]           = scale_base ? (uint8_t)(scale_base - 1 + (int)((z >> 33) % 3)) : (uint8_t)(z >> 33);
    }
}

__global__ void f16_to_f32_kernel(float* out, const half_t* in, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out[i] = (float)in[i];
    }
}

__global__ void fill_const_f32_kernel(float* out, size_t n, float v)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        out[i] = v;
    }
}

__global__ void set_int_kernel(int* dst, int v)
{
    *dst = v;
}

static tm_rope_param model_rope_param(const tm_engine* e)
{
    const tm_model_config& m = e->cfg.model;
    tm_rope_param          p{};
    p.dim = e->D, p.base = m.rope_base, p.type = m.rope_type, p.factor = m.rope_factor;
    p.low_freq_factor = m.rope_low_freq_factor, p.high_freq_factor = m.rope_high_freq_factor;
    p.original_max_position   = m.rope_original_max_position;
    p.max_position_embeddings = m.rope_max_position_embeddings;
    p.yarn_beta_fast = m.rope_yarn_beta_fast, p.yarn_beta_slow = m.rope_yarn_beta_slow;
    p.yarn_attention_factor = m.rope_yarn_attention_factor;
    p.yarn_truncate         = m.rope_yarn_truncate;
    return p;
}

// Admission of a sequence into batch slot `slot` (static prefill, continuous-batching admit, scoring): its RoPE base is fixed from its
// prompt length (init_dynamic_ntk, unified_attention_layer.cc:228-243) and never changes while it generates.  A base of its own ->
// the slot's table region is rebuilt on the engine stream, in front of the sequence's first forward, and the slot's row offset points
// at it; the model's base -> offset 0, the shared table.  No-op on an engine with one table.
int rope_admit(tm_engine* e, int slot, int prompt_len)
{
    if (!e->d_rope_row0) {
        return 0;
    }
    const tm_model_config& m = e->cfg.model;
    TM_REQUIRE(slot >= 0 && slot < e->cfg.max_batch_size, "internal: rope_admit slot");
    const float base = tm_rope_dynamic_base(m.rope_base, m.rope_factor, e->D, m.rope_max_position_embeddings, prompt_len);
    int         row0 = 0;
    if (base != m.rope_base) {
        row0            = (1 + slot) * e->rope_max_pos;
        tm_rope_param p = model_rope_param(e);
        p.base          = base;
        RopeInvFreq f;
        TM_TRY(rope_inv_freq(&f, p));
        TM_TRY(launch_rope_table(e->d_rope + (size_t)row0 * (e->D / 2), e->rope_max_pos, e->D, f, e->stream));
    }
    if (row0 != e->h_rope_row0[slot]) {
        set_int_kernel<<<1, 1, 0, e->stream>>>(e->d_rope_row0 + slot, row0);
        TM_HIP_CHECK(hipGetLastError());
        e->h_rope_row0[slot] = row0;
    }
    return 0;
}

// the slots [slot0, slot0 + n) go back to the shared table (release, a parked slot, the end of a scoring call)
int rope_reset(tm_engine* e, int slot0, int n)
{
    if (!e->d_rope_row0 || n <= 0) {
        return 0;
    }
    TM_HIP_CHECK(hipMemsetAsync(e->d_rope_row0 + slot0, 0, (size_t)n * sizeof(int), e->stream));
    std::fill(e->h_rope_row0.begin() + slot0, e->h_rope_row0.begin() + slot0 + n, 0);
    return 0;
}

// declares a linear: its format is resolved here, once, and its staging slots are the format's parts (linear_staging)
static void add_linear(tm_engine* e, LinearSlots& l, const std::string& prefix, int K, int N, int type, int role = 0, bool gated = false,
                       bool expert = false)
{
    l.prefix  = prefix;
    l.gated   = gated;
    l.expert  = expert;
    l.w.role  = role;  // dispatch-table key next to (K, N, M): the tuner times each role with its own consumer
    l.w.K     = K;
    l.w.N     = N;
    l.w.group = e->cfg.model.group_size;
    l.w.type  = type;
    l.w.fmt   = linear_format(type, e->cfg.model.fp8_scale_mode, expert, l.w.group);
    l.w.gated = gated;
    const LinearStaging sg = linear_staging(l.w.fmt, K, N, l.w.group);
    for (int i = 0; i < sg.n; ++i) {
        e->slots[prefix + "." + sg.suffix[i]].bytes = (int64_t)sg.bytes[i];
    }
}

// every linear of this rank's shard against the general kernel's addressing limit (its packed image is addressed with 32-bit offsets,
// gemm_w4a16.hip): add_linear cannot report an error, so engine creation refuses such a model up front
static int check_linear_images(const tm_model_config& m, int tp)
{
    const int q = m.q_heads / tp, kv = std::max(1, m.kv_heads / tp), inter = m.inter / tp, shared = m.moe_shared_inter / tp;
    const struct {
        const char* name;
        int         K, N, type;
    } lin[] = {{"w_qkv", m.hidden, (q + 2 * kv) * m.head_dim, m.weight_type}, {"wo", q * m.head_dim, m.hidden, m.weight_type},
               {"w1w3", m.hidden, 2 * inter, m.weight_type}, {"w2", inter, m.hidden, m.weight_type},
               {"lm_head", m.hidden, m.vocab / tp, TM_WEIGHT_F16},
               {"shared w1w3", m.hidden, 2 * shared, m.weight_type}, {"shared w2", shared, m.hidden, m.weight_type}};
    for (const auto& l : lin) {
        if (l.K == 0 || l.N == 0) {  // no shared expert
            continue;
        }
        if (l.type == TM_WEIGHT_U4 && m.group_size == 32) {  // no general-kernel image: the G32 image of gemm_u4_g32.hip
            TM_REQUIRE(l.K % 128 == 0 && l.N % 32 == 0 && g32_bytes(l.K, l.N) < kGeneralImageLimit,
                       std::string(l.name) + " " + std::to_string(l.K) + " x " + std::to_string(l.N)
                           + ": a u4 group-32 linear needs K % 128 == 0, N % 32 == 0 and an image below 2^31 bytes");
            continue;
        }
        if (l.type == TM_WEIGHT_I8) {  // no general-kernel image: the P8 image + column scales of gemm_int8.hip, same limit
            TM_REQUIRE(l.K % 128 == 0 && l.N % 32 == 0 && p8_bytes(l.K, l.N) + (size_t)l.N * 4 < kGeneralImageLimit,
                       std::string(l.name) + " " + std::to_string(l.K) + " x " + std::to_string(l.N)
                           + ": an int8 linear needs K % 128 == 0, N % 32 == 0 and an image below 2^31 bytes");
            continue;
        }
        const size_t bytes = gemm_general_image_bytes(l.K, l.N, l.type);
        TM_REQUIRE(bytes < kGeneralImageLimit, std::string(l.name) + " " + std::to_string(l.K) + " x " + std::to_string(l.N)
                                                   + ": its general-kernel image of " + std::to_string(bytes)
                                                   + " bytes reaches 2^31 (the kernel addresses it with 32-bit offsets)");
    }
    return 0;
}

static int ensure_slot(tm_engine* e, const std::string& name, Slot** out)
{
    auto it = e->slots.find(name);
    TM_REQUIRE(it != e->slots.end(), "unknown weight slot: " + name);
    Slot& s = it->second;
    if (!s.dev) {
        TM_HIP_CHECK(hipMalloc(&s.dev, s.bytes));
    }
    *out = &s;
    return 0;
}

static int fill_normal(tm_engine* e, void* dst, size_t n, float mean, float stddev, uint64_t seed)
{
    const size_t thr = (n + 1) / 2;
    fill_normal_kernel<<<(thr + 255) / 256, 256, 0, e->stream>>>((half_t*)dst, n, mean, stddev, seed);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// staged parts -> device image(s): check filled, prepare, synchronise, free the parts
static int prepare_linear(tm_engine* e, LinearSlots& l)
{
    if (l.w.K == 0 || linear_weight_prepared(l.w)) {  // not declared (the dense FFN of a MoE layer without a shared expert) / done
        return 0;
    }
    const LinearStaging sg = linear_staging(l.w.fmt, l.w.K, l.w.N, l.w.group);
    Slot*               slot[3];
    const void*         part[3];
    for (int i = 0; i < sg.n; ++i) {
        slot[i] = &e->slots[l.prefix + "." + sg.suffix[i]];
        TM_REQUIRE(slot[i]->filled, "weight not loaded: " + l.prefix);
        part[i] = slot[i]->dev;
    }
    // u4 policy: dense linears whose every M goes to gemm_decode.hip keep ONE HBM image (P32); MoE experts run the grouped mode of
    // gemm_kernel and keep the 16-column image as well
    const bool p32_only = !l.expert && dec32_serves_every_m(l.w.K, l.w.N);
    // the resident fp16 image for prefill-sized forwards (gemm_prefill_f16.hip): dense linears of engines whose prefill forwards are
    // large enough to use it (the 256 x 256 tile is proposed from 1024 rows); TM_PREFILL_F16_IMAGE=1 builds it
    // (opt-in: measured +15 % on w_qkv, +2 % on wo, -1 .. -5 % on w1w3 / w2 against the fused tiles at M = 8192 -- the tile is bound by the
    // CU's load path, not by the dequantisation it removes: profiles/r06_prefill_f16_image_ablations.txt -- for 2 bytes per parameter)
    static const bool f16img = [] {
        const char* v = getenv("TM_PREFILL_F16_IMAGE");
        return v && atoi(v) != 0;
    }();
    TM_TRY(linear_weight_prepare(l.w, part, e->stream, p32_only, f16img && p32_only && e->cfg.max_prefill_token_num >= 1024 && l.w.N >= 256));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    for (int i = 0; i < sg.n; ++i) {
        TM_HIP_CHECK(hipFree(slot[i]->dev));
        slot[i]->dev = nullptr;
    }
    return 0;
}

}  // namespace tmk

extern "C" {

int tm_engine_create(tm_engine** out, const tm_engine_config* c)
{
    TM_REQUIRE(out && c, "null pointer");
    const tm_model_config& m = c->model;
    TM_REQUIRE(m.head_dim == 64 || m.head_dim == 128, "head_dim must be 64 or 128");
    TM_REQUIRE(m.head_dim == 128 || !m.qk_norm, "qk_norm (per-head q/k RMSNorm) needs head_dim 128: not built for head_dim 64");
    TM_REQUIRE(m.attn_window >= 0, "attn_window must be >= 0 (0 = full attention)");
    TM_REQUIRE(m.group_size == 128 || (m.group_size == 32 && m.weight_type == TM_WEIGHT_U4),
               "group_size " + std::to_string(m.group_size) + " is not served: u4 weights come in groups of 128 or -- dense models -- 32, every "
               "other weight_type is created with 128");
    if (m.weight_type == TM_WEIGHT_U4 && m.group_size == 32) {  // gemm_u4_g32.hip: dense linears only
        TM_REQUIRE(m.moe_experts == 0, "group_size 32 with moe_experts > 0 is not built: the group-32 u4 kernel serves dense linears only");
        TM_REQUIRE(m.hidden_valid == 0 || m.hidden_valid == m.hidden, "group_size 32 with padded widths (hidden_valid) is not built");
    }
    TM_REQUIRE(c->tp >= 1 && c->rank >= 0 && c->rank < c->tp, "0 <= rank < tp");
    TM_REQUIRE(m.q_heads % c->tp == 0 && m.inter % c->tp == 0 && m.vocab % c->tp == 0, "heads/inter/vocab % tp");
    TM_REQUIRE(m.kv_heads % c->tp == 0 || c->tp % m.kv_heads == 0, "kv_heads vs tp");
    TM_REQUIRE(m.rope_type >= 0 && m.rope_type <= 4, "rope_type in {0 default, 1 linear, 2 llama3, 3 yarn, 4 dynamic}");
    TM_REQUIRE(c->quant_policy == 0 || c->quant_policy == 4 || c->quant_policy == 8 || c->quant_policy == 42,
               "quant_policy in {0,4,8,42} (lmdeploy/messages.py:351-358)");
    // TurboQuant KV (turboquant.h): the 128-wide rotation, full attention, one rank
    TM_REQUIRE(c->quant_policy != 42 || m.head_dim == 128, "quant_policy 42 (TurboQuant KV) needs head_dim 128: head_dim 64 is not built");
    TM_REQUIRE(c->quant_policy != 42 || (m.attn_window == 0 && m.attn_sinks == 0),
               "quant_policy 42 (TurboQuant KV) with a sliding window or attention sinks is not built");
    TM_REQUIRE(c->quant_policy != 42 || c->tp == 1, "quant_policy 42 (TurboQuant KV) with tp > 1 is not built (run with tp = 1)");
    TM_REQUIRE(c->cache_block_seq_len == 64, "cache_block_seq_len must be 64");
    TM_REQUIRE(m.weight_type == TM_WEIGHT_U4 || m.weight_type == TM_WEIGHT_F16 || m.weight_type == TM_WEIGHT_FP8
                   || m.weight_type == TM_WEIGHT_MXFP4 || m.weight_type == TM_WEIGHT_I8,
               "weight_type");
    if (m.weight_type == TM_WEIGHT_I8) {  // dense W8A8 models on the int8 matrix cores
        TM_REQUIRE(m.moe_experts == 0, "weight_type int8 (W8A8 dense linears) with moe_experts > 0 is not built: int8 experts are not served");
        TM_REQUIRE(m.hidden_valid == 0 || m.hidden_valid == m.hidden, "weight_type int8 (W8A8 dense linears) with padded widths (hidden_valid) is not built");
        TM_REQUIRE(std::max(m.hidden, m.inter) <= kFp8TokenMaxK, "weight_type int8: the per-token quantiser serves rows of up to 32768 channels");
    }
    if (m.weight_type == TM_WEIGHT_MXFP4) {  // dense W4A4 models on the block-scaled FP4 matrix cores
        TM_REQUIRE(c->tp == 1, "weight_type mxfp4 (W4A4 dense linears) with tp > 1 is not built (run with tp = 1)");
        TM_REQUIRE(m.moe_experts == 0,
                   "weight_type mxfp4 (W4A4 dense linears) with moe_experts > 0 is not built: MXFP4 experts run weight-only under "
                   "moe_expert_format 3 with fp16 dense linears");
        TM_REQUIRE(m.hidden_valid == 0 || m.hidden_valid == m.hidden,
                   "weight_type mxfp4 (W4A4 dense linears) with padded widths (hidden_valid) is not built");
    }
    TM_REQUIRE(m.fp8_scale_mode == 0 || (m.fp8_scale_mode == 1 && m.weight_type == TM_WEIGHT_FP8),
               "fp8_scale_mode: 0 (128 x 128 blocks) or, with weight_type fp8, 1 (one scale per output channel)");
    TM_REQUIRE(m.fp8_scale_mode == 0 || std::max(m.hidden, std::max(m.inter, m.moe_shared_inter)) <= kFp8TokenMaxK,
               "fp8_scale_mode 1: the per-token quantiser serves rows of up to 32768 channels");
    TM_REQUIRE(c->max_batch_size >= 1 && c->max_batch_size <= 1024 && c->session_len >= 1,
               "1 <= max_batch_size <= 1024, session_len >= 1");
    TM_REQUIRE(m.moe_shared_inter >= 0 && (m.moe_shared_inter == 0 || m.moe_experts > 0), "moe_shared_inter needs moe_experts > 0");
    TM_REQUIRE(m.moe_shared_inter % c->tp == 0 && (m.moe_shared_inter / c->tp) % 128 == 0,
               "moe_shared_inter / tp must be a multiple of 128");
    TM_REQUIRE(m.moe_expert_format == 0 || m.moe_expert_format == TM_WEIGHT_MXFP4, "moe_expert_format: 0 (follow weight_type) or 3 (MXFP4)");
    TM_REQUIRE((m.moe_expert_format == 0 && m.moe_act == 0 && m.moe_bias == 0) || m.moe_experts > 0,
               "moe_expert_format / moe_act / moe_bias need moe_experts > 0");
    TM_REQUIRE(m.moe_act == 0 || m.moe_act == 1, "moe_act: 0 (SiLU) or 1 (gpt-oss)");
    TM_REQUIRE((m.moe_act == 0 && m.moe_bias == 0) || m.moe_expert_format == TM_WEIGHT_MXFP4 || m.weight_type == TM_WEIGHT_F16,
               "moe_act / moe_bias: the gpt-oss activation and expert biases are built for fp16 and MXFP4 experts only (not u4 / fp8)");
    TM_REQUIRE(m.moe_bias == 0 || m.moe_act == 1, "moe_bias needs moe_act = 1 (the gpt-oss activation)");
    TM_REQUIRE((m.moe_act == 0 && m.moe_bias == 0) || m.moe_shared_inter == 0, "moe_act / moe_bias with a shared expert is not built");
    TM_REQUIRE((m.moe_expert_format != TM_WEIGHT_MXFP4 && m.moe_bias == 0) || c->tp == 1,
               "MXFP4 experts / expert biases with tp > 1 are not built: the w2 bias would need a per-rank rule (run with tp = 1)");
    TM_REQUIRE(m.hidden_valid == 0 || (m.hidden_valid > 0 && m.hidden_valid <= m.hidden && m.hidden_valid % 8 == 0),
               "hidden_valid: 0 or a multiple of 8 in (0, hidden]");
    TM_REQUIRE(m.hidden_valid == 0 || m.hidden_valid == m.hidden || c->tp == 1,
               "hidden_valid != hidden (a zero-padded model) with tp > 1 is not built: the fused all-reduce + norm has no valid-width variant "
               "(run with tp = 1)");
    TM_REQUIRE(m.attn_out_bias == 0 || c->tp == 1,
               "attn_out_bias with tp > 1 is not built: the o_proj bias would have to be added on one rank only (run with tp = 1)");
    TM_TRY(check_linear_images(m, c->tp));
    TM_HIP_CHECK(hipSetDevice(c->device));

    auto* e        = new tm_engine();
    e->cfg         = *c;
    e->hidden      = m.hidden;
    e->hidden_valid = m.hidden_valid ? m.hidden_valid : m.hidden;
    e->q_heads     = m.q_heads / c->tp;
    e->kv_heads    = std::max(1, m.kv_heads / c->tp);
    e->inter       = m.inter / c->tp;
    e->shared_inter = m.moe_shared_inter / c->tp;
    e->vocab_local = m.vocab / c->tp;
    {
        const char* fc = getenv("TM_FORCE_COMM");
        e->use_comm    = c->tp > 1 || (fc && atoi(fc));
        const char* ms    = getenv("TM_MIXED_STEP");
        const char* gc    = getenv("TM_GRAPH_COMM");
        e->mixed_steps_on = !(ms && !atoi(ms));
        e->graph_comm     = !(gc && !atoi(gc));
        const char* kr    = getenv("TM_KV_RING");  // 0: sliding-window models reserve whole contexts too (A/B arm of the block ring)
        e->kv_ring_on     = !(kr && !atoi(kr));
    }
    e->D           = m.head_dim;
    e->qkv_n       = (e->q_heads + 2 * e->kv_heads) * e->D;
    TM_REQUIRE((e->inter * 1) % 128 == 0 && (e->q_heads * e->D) % 128 == 0 && m.hidden % 128 == 0,
               "K dims must be multiples of 128 after TP sharding");
    TM_REQUIRE(m.moe_experts == 0 || (m.moe_experts <= 256 && m.moe_top_k >= 1 && m.moe_top_k <= 8 && m.moe_top_k <= m.moe_experts),
               "moe: 1 <= top_k <= experts <= 256, top_k <= 8 (u4, fp8 or fp16 expert weights)");
    // the grouped expert GEMMs put experts x 64-row blocks of one forward on grid.z: refuse here what the first large prefill would hit
    TM_REQUIRE(m.moe_experts == 0
                   || (int64_t)m.moe_experts * ((std::max(c->max_batch_size, std::max(64, c->max_prefill_token_num)) + 63) / 64) <= 65535,
               "moe: experts x ceil(max_prefill_token_num / 64) exceeds the grouped GEMMs' grid.z (65535): lower max_prefill_token_num");
    TM_HIP_CHECK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));

    e->layers.resize(m.layers);
    for (int i = 0; i < m.layers; ++i) {
        const std::string p = "layers." + std::to_string(i);
        Layer&            L = e->layers[i];
        add_linear(e, L.qkv, p + ".attention.w_qkv", m.hidden, e->qkv_n, m.weight_type, 1);
        add_linear(e, L.wo, p + ".attention.wo", e->q_heads * e->D, m.hidden, m.weight_type, 2);
        if (m.moe_experts > 0) {
            L.is_moe = true;
            L.ex13.resize(m.moe_experts);
            L.ex2.resize(m.moe_experts);
            e->slots[p + ".moe_ffn.gate.weight"].bytes = (int64_t)m.hidden * m.moe_experts * 2;  // fp16 [H][E], replicated
            for (int x = 0; x < m.moe_experts; ++x) {
                const std::string q = p + ".moe_ffn.experts." + std::to_string(x);
                const int xt = m.moe_expert_format ? m.moe_expert_format : m.weight_type;
                add_linear(e, L.ex13[x], q + ".w1w3", m.hidden, 2 * e->inter, xt, 0, true, true);
                add_linear(e, L.ex2[x], q + ".w2", e->inter, m.hidden, xt, 0, false, true);
                if (m.moe_bias) {
                    e->slots[q + ".w1w3.bias"].bytes = (int64_t)2 * e->inter * 2;  // fp16, (gate_j, up_j)-interleaved
                    e->slots[q + ".w2.bias"].bytes   = (int64_t)m.hidden * 2;
                }
            }
            if (m.moe_bias) {
                e->slots[p + ".moe_ffn.gate.bias"].bytes = (int64_t)m.moe_experts * 4;  // fp32 [E], replicated
            }
            if (e->shared_inter > 0) {  // the shared expert: the layer's dense feed_forward at its own width + the sigmoid gate [H]
                L.has_shared = true;
                add_linear(e, L.w13, p + ".feed_forward.w1w3", m.hidden, 2 * e->shared_inter, m.weight_type, 3, true);
                add_linear(e, L.w2, p + ".feed_forward.w2", e->shared_inter, m.hidden, m.weight_type, 4);
                e->slots[p + ".moe_ffn.shared_gate.weight"].bytes = (int64_t)m.hidden * 2;  // fp16 [H], replicated
            }
        }
        else {
            add_linear(e, L.w13, p + ".feed_forward.w1w3", m.hidden, 2 * e->inter, m.weight_type, 3, true);
            add_linear(e, L.w2, p + ".feed_forward.w2", e->inter, m.hidden, m.weight_type, 4);
        }
        e->slots[p + ".attention_norm.weight"].bytes = (int64_t)m.hidden * 2;
        e->slots[p + ".ffn_norm.weight"].bytes       = (int64_t)m.hidden * 2;
        if (m.attn_bias) {  // this rank's Q | K | V columns, q / k channel-permuted like the weights
            e->slots[p + ".attention.w_qkv.bias"].bytes = (int64_t)e->qkv_n * 2;
        }
        if (m.attn_sinks) {  // this rank's q heads
            e->slots[p + ".attention.sinks"].bytes = (int64_t)e->q_heads * 2;
        }
        if (m.attn_out_bias) {  // tp == 1
            e->slots[p + ".attention.wo.bias"].bytes = (int64_t)m.hidden * 2;
        }
        if (m.qk_norm) {  // one head, permuted like one head of q / k; replicated over the ranks
            e->slots[p + ".attention.q_norm.weight"].bytes = (int64_t)e->D * 2;
            e->slots[p + ".attention.k_norm.weight"].bytes = (int64_t)e->D * 2;
        }
    }
    e->slots["tok_embeddings.weight"].bytes = (int64_t)m.vocab * m.hidden * 2;  // replicated
    e->slots["norm.weight"].bytes           = (int64_t)m.hidden * 2;
    add_linear(e, e->output, "output", m.hidden, e->vocab_local, TM_WEIGHT_F16, 5);
    *out = e;
    return 0;
}

int tm_engine_set_layer_windows(tm_engine* e, const int* window, int layers)
{
    TM_REQUIRE(e && window, "null pointer");
    TM_REQUIRE(!e->started, "tm_engine_set_layer_windows: call before tm_engine_start");
    TM_REQUIRE(layers == e->cfg.model.layers, "tm_engine_set_layer_windows: one window per layer of the model");
    for (int i = 0; i < layers; ++i) {
        TM_REQUIRE(window[i] >= 0, "tm_engine_set_layer_windows: window must be >= 0 (0 = full attention)");
    }
    e->layer_windows.assign(window, window + layers);
    return 0;
}

int tm_engine_set_mrope_section(tm_engine* e, int sec_t, int sec_h, int sec_w)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(!e->started, "tm_engine_set_mrope_section: call before tm_engine_start");
    const tm_model_config& m = e->cfg.model;
    TM_REQUIRE(sec_t >= 0 && sec_h >= 0 && sec_w >= 0, "mrope_section: three non-negative sizes (0 / 0 / 0 = none)");
    if (sec_t + sec_h + sec_w > 0) {
        TM_REQUIRE(m.head_dim == 128, "mrope_section needs head_dim 128: M-RoPE is not built for head_dim 64");
        TM_REQUIRE(sec_t + sec_h + sec_w == m.head_dim / 2, "mrope_section must sum to head_dim / 2");
        TM_REQUIRE(m.rope_type != 4, "mrope_section with rope_type 4 (dynamic NTK, per-sequence tables) is not built");
    }
    e->mrope_section[0] = sec_t;
    e->mrope_section[1] = sec_h;
    e->mrope_section[2] = sec_w;
    return 0;
}

int64_t tm_engine_weight_bytes(tm_engine* e, const char* name)
{
    if (!e || !name) {
        return 0;
    }
    auto it = e->slots.find(name);
    if (it == e->slots.end()) {
        set_last_error(std::string("unknown weight slot: ") + name);
        return 0;
    }
    return it->second.bytes;
}

int tm_engine_weight_copy(tm_engine* e, const char* name, const void* host_src, int64_t bytes)
{
    TM_REQUIRE(e && name && host_src, "null pointer");
    TM_REQUIRE(!e->weights_ready, "weights already processed");
    Slot* s = nullptr;
    TM_TRY(ensure_slot(e, name, &s));
    TM_REQUIRE(bytes == s->bytes, std::string("byte size mismatch for ") + name + ": got " + std::to_string(bytes)
                                      + " expected " + std::to_string(s->bytes));
    TM_HIP_CHECK(hipMemcpy(s->dev, host_src, bytes, hipMemcpyHostToDevice));
    s->filled = true;
    return 0;
}

int tm_engine_init_synthetic(tm_engine* e, uint64_t seed)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(!e->weights_ready, "weights already processed");
    const tm_model_config& m = e->cfg.model;
    uint64_t               sd = seed * 1000003ull + 17;
    half_t*                master = nullptr;  // fp16 master of the largest linear, reused
    size_t                 master_elems = 0;
    auto                   linear = [&](LinearSlots& l) -> int {
        const size_t        n  = (size_t)l.w.K * l.w.N;
        const LinearStaging sg = linear_staging(l.w.fmt, l.w.K, l.w.N, l.w.group);
        Slot*               part[3];
        for (int i = 0; i < sg.n; ++i) {
            TM_TRY(ensure_slot(e, l.prefix + "." + sg.suffix[i], &part[i]));
            part[i]->filled = true;
        }
        const float std_w = 0.1f / std::sqrt((float)l.w.K);  // the weights' magnitude in every format
        for (int i = 0; i < sg.n; ++i) {  // random values of what each part holds (LinearStaging::kind)
            const size_t nb = (size_t)part[i]->bytes;
            const dim3   grid((unsigned)((nb + 255) / 256));
            switch (sg.kind[i]) {
                case PartKind::F16: TM_TRY(fill_normal(e, part[i]->dev, n, 0.f, std_w, ++sd)); break;
                case PartKind::E4M3: fill_fp8_kernel<<<grid, 256, 0, e->stream>>>((uint8_t*)part[i]->dev, nb, ++sd); break;  // random e4m3 codes (no NaN) ...
                case PartKind::I8: fill_mxfp4_kernel<<<grid, 256, 0, e->stream>>>((uint8_t*)part[i]->dev, nb, ++sd, 0); break;  // uniform int8 codes ...
                case PartKind::F32_SCALES:  // ... under one constant scale: E|code value| ~ 30 (e4m3) / rms 74 (int8) -> weights ~ 0.1 / sqrt(K)
                    fill_const_f32_kernel<<<(nb / 4 + 255) / 256, 256, 0, e->stream>>>(
                        (float*)part[i]->dev, nb / 4, (sg.kind[0] == PartKind::I8 ? 0.00135f : 0.0027f) / std::sqrt((float)l.w.K));
                    break;
                case PartKind::E2M1: fill_mxfp4_kernel<<<grid, 256, 0, e->stream>>>((uint8_t*)part[i]->dev, nb, ++sd, 0); break;
                case PartKind::UE8M0: {
                    // uniform e2m1 codes (E|value| = 2.25) under scale bytes around 127 - 6: weights of the other synthetic formats' magnitude
                    // (dense W4A4 linears: around the byte that puts 2.25 * 2^(s - 127) next to their 0.1 / sqrt(K))
                    const int sbase = !l.expert ? 127 + (int)std::lround(std::log2(0.1 / std::sqrt((double)l.w.K) / 2.25)) : 127 - 6;
                    fill_mxfp4_kernel<<<grid, 256, 0, e->stream>>>((uint8_t*)part[i]->dev, nb, ++sd, sbase);
                    break;
                }
                case PartKind::AWQ_QWEIGHT: {  // an fp16 master, quantised group-wise into this part and the two behind it
                    if (n > master_elems) {
                        if (master) {
                            TM_HIP_CHECK(hipStreamSynchronize(e->stream));
                            TM_HIP_CHECK(hipFree(master));
                        }
                        TM_HIP_CHECK(hipMalloc((void**)&master, n * 2));
                        master_elems = n;
                    }
                    // TM_SYNTH_WEIGHT_SCALE (diagnostics only: `0` = all-zero linear weights, the low-toggle arm of the power experiment in DESIGN 3.8)
                    static const float wscale = [] {
                        const char* v = getenv("TM_SYNTH_WEIGHT_SCALE");
                        return v ? (float)atof(v) : 1.0f;
                    }();
                    TM_TRY(fill_normal(e, master, n, 0.f, wscale * 0.1f / std::sqrt((float)l.w.K), ++sd));
                    TM_TRY(launch_quantize_groupwise_u4((int32_t*)part[0]->dev, (half_t*)part[1]->dev, (half_t*)part[2]->dev, nullptr, master,
                                                        l.w.K, l.w.N, l.w.group, e->stream));
                    break;
                }
                case PartKind::AWQ_SCALES:
                case PartKind::AWQ_ZEROS: break;  // written with the qweight part
            }
            TM_HIP_CHECK(hipGetLastError());
        }
        return prepare_linear(e, l);  // repack right away so that staging never holds more than one linear
    };
    auto vec = [&](const std::string& name, size_t n, float mean, float stddev) -> int {
        Slot* s = nullptr;
        TM_TRY(ensure_slot(e, name, &s));
        TM_TRY(fill_normal(e, s->dev, n, mean, stddev, ++sd));
        s->filled = true;
        return 0;
    };
    for (int i = 0; i < m.layers; ++i) {
        const std::string p = "layers." + std::to_string(i);
        Layer&            L = e->layers[i];
        TM_TRY(linear(L.qkv));
        TM_TRY(linear(L.wo));
        if (L.is_moe) {
            TM_TRY(vec(p + ".moe_ffn.gate.weight", (size_t)m.hidden * m.moe_experts, 0.f, 0.05f));
            for (int x = 0; x < m.moe_experts; ++x) {
                TM_TRY(linear(L.ex13[x]));
                TM_TRY(linear(L.ex2[x]));
                if (m.moe_bias) {
                    TM_TRY(vec(L.ex13[x].prefix + ".bias", (size_t)2 * e->inter, 0.f, 0.05f));
                    TM_TRY(vec(L.ex2[x].prefix + ".bias", m.hidden, 0.f, 0.02f));
                }
            }
            if (m.moe_bias) {  // fp32 [E]: drawn in fp16, then widened
                Slot* gb = nullptr;
                TM_TRY(ensure_slot(e, p + ".moe_ffn.gate.bias", &gb));
                half_t* tmp = nullptr;
                TM_HIP_CHECK(hipMalloc((void**)&tmp, (size_t)m.moe_experts * 2));
                TM_TRY(fill_normal(e, tmp, m.moe_experts, 0.f, 0.5f, ++sd));
                f16_to_f32_kernel<<<(m.moe_experts + 255) / 256, 256, 0, e->stream>>>((float*)gb->dev, tmp, m.moe_experts);
                TM_HIP_CHECK(hipGetLastError());
                TM_HIP_CHECK(hipStreamSynchronize(e->stream));
                TM_HIP_CHECK(hipFree(tmp));
                gb->filled = true;
            }
            if (L.has_shared) {
                TM_TRY(linear(L.w13));
                TM_TRY(linear(L.w2));
                TM_TRY(vec(p + ".moe_ffn.shared_gate.weight", m.hidden, 0.f, 0.05f));
            }
        }
        else {
            TM_TRY(linear(L.w13));
            TM_TRY(linear(L.w2));
        }
        TM_TRY(vec(p + ".attention_norm.weight", m.hidden, 1.f, 0.02f));
        TM_TRY(vec(p + ".ffn_norm.weight", m.hidden, 1.f, 0.02f));
        if (m.attn_bias) {
            TM_TRY(vec(p + ".attention.w_qkv.bias", e->qkv_n, 0.f, 0.02f));
        }
        if (m.attn_sinks) {
            TM_TRY(vec(p + ".attention.sinks", e->q_heads, 0.f, 1.f));
        }
        if (m.attn_out_bias) {
            TM_TRY(vec(p + ".attention.wo.bias", m.hidden, 0.f, 0.02f));
        }
        if (m.qk_norm) {
            TM_TRY(vec(p + ".attention.q_norm.weight", e->D, 1.f, 0.05f));
            TM_TRY(vec(p + ".attention.k_norm.weight", e->D, 1.f, 0.05f));
        }
    }
    TM_TRY(vec("tok_embeddings.weight", (size_t)m.vocab * m.hidden, 0.f, 0.02f));
    TM_TRY(vec("norm.weight", m.hidden, 1.f, 0.02f));
    TM_TRY(linear(e->output));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    if (master) {
        TM_HIP_CHECK(hipFree(master));
    }
    return 0;
}

int tm_engine_process_weights(tm_engine* e)
{
    TM_REQUIRE(e, "null pointer");
    if (e->weights_ready) {
        return 0;
    }
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    const tm_model_config& m = e->cfg.model;
    auto norm = [&](const std::string& name, half_t** dst) -> int {
        Slot& s = e->slots[name];
        TM_REQUIRE(s.filled, "weight not loaded: " + name);
        *dst = (half_t*)s.dev;  // used in place
        return 0;
    };
    for (int i = 0; i < m.layers; ++i) {
        const std::string p = "layers." + std::to_string(i);
        Layer&            L = e->layers[i];
        for (LinearSlots* l : {&L.qkv, &L.wo, &L.w13, &L.w2}) {
            TM_TRY(prepare_linear(e, *l));
        }
        if (L.is_moe) {
            L.moe.hidden       = m.hidden;
            L.moe.inter        = e->inter;
            L.moe.experts      = m.moe_experts;
            L.moe.top_k        = m.moe_top_k;
            L.moe.norm_topk    = m.moe_norm_topk != 0;
            L.moe.routed_scale = m.moe_routed_scale > 0.f ? m.moe_routed_scale : 1.f;
            L.moe.w13.resize(m.moe_experts);
            L.moe.w2.resize(m.moe_experts);
            for (int x = 0; x < m.moe_experts; ++x) {
                TM_TRY(prepare_linear(e, L.ex13[x]));
                TM_TRY(prepare_linear(e, L.ex2[x]));
                linear_weight_take(L.moe.w13[x], L.ex13[x].w);  // the MoE block owns the packed weights from here on
                linear_weight_take(L.moe.w2[x], L.ex2[x].w);
            }
            L.moe.act = m.moe_act;
            if (m.moe_bias) {  // the experts' biases side by side ([E][2I], [E][H]: what the grouped GEMM and the combine index)
                const size_t n13 = (size_t)2 * e->inter, n2 = (size_t)m.hidden;
                TM_HIP_CHECK(hipMalloc((void**)&L.moe.b13, n13 * m.moe_experts * 2));
                TM_HIP_CHECK(hipMalloc((void**)&L.moe.b2, n2 * m.moe_experts * 2));
                for (int x = 0; x < m.moe_experts; ++x) {
                    Slot &s13 = e->slots[L.ex13[x].prefix + ".bias"], &s2 = e->slots[L.ex2[x].prefix + ".bias"];
                    TM_REQUIRE(s13.filled && s2.filled, "weight not loaded: " + L.ex13[x].prefix + ".bias / " + L.ex2[x].prefix + ".bias");
                    TM_HIP_CHECK(hipMemcpyAsync(L.moe.b13 + n13 * x, s13.dev, n13 * 2, hipMemcpyDeviceToDevice, e->stream));
                    TM_HIP_CHECK(hipMemcpyAsync(L.moe.b2 + n2 * x, s2.dev, n2 * 2, hipMemcpyDeviceToDevice, e->stream));
                }
                TM_HIP_CHECK(hipStreamSynchronize(e->stream));
                for (int x = 0; x < m.moe_experts; ++x) {
                    for (Slot* sl : {&e->slots[L.ex13[x].prefix + ".bias"], &e->slots[L.ex2[x].prefix + ".bias"]}) {
                        TM_HIP_CHECK(hipFree(sl->dev));
                        sl->dev = nullptr;
                    }
                }
                Slot& gb = e->slots[p + ".moe_ffn.gate.bias"];
                TM_REQUIRE(gb.filled, "weight not loaded: " + p + ".moe_ffn.gate.bias");
                L.moe.gate_bias = (float*)gb.dev;  // used in place (freed by moe_free)
                gb.dev          = nullptr;
            }
            Slot& g = e->slots[p + ".moe_ffn.gate.weight"];
            TM_REQUIRE(g.filled, "weight not loaded: " + p + ".moe_ffn.gate.weight");
            L.moe.gate = (half_t*)g.dev;  // used in place (freed by moe_free)
            g.dev      = nullptr;
            if (L.has_shared) {
                Slot& sg = e->slots[p + ".moe_ffn.shared_gate.weight"];
                TM_REQUIRE(sg.filled, "weight not loaded: " + p + ".moe_ffn.shared_gate.weight");
                L.moe.shared_gate = (half_t*)sg.dev;  // used in place (freed by moe_free)
                sg.dev            = nullptr;
            }
            TM_TRY(moe_prepare(L.moe, e->stream));
        }
        TM_TRY(norm(p + ".attention_norm.weight", &L.attn_norm));
        TM_TRY(norm(p + ".ffn_norm.weight", &L.ffn_norm));
        if (m.attn_bias) {
            TM_TRY(norm(p + ".attention.w_qkv.bias", &L.qkv_bias));
        }
        if (m.attn_sinks) {
            TM_TRY(norm(p + ".attention.sinks", &L.sinks));
        }
        if (m.attn_out_bias) {
            TM_TRY(norm(p + ".attention.wo.bias", &L.wo_bias));
        }
        if (m.qk_norm) {
            TM_TRY(norm(p + ".attention.q_norm.weight", &L.q_norm));
            TM_TRY(norm(p + ".attention.k_norm.weight", &L.k_norm));
        }
    }
    TM_TRY(norm("tok_embeddings.weight", &e->tok_embeddings));
    TM_TRY(norm("norm.weight", &e->final_norm));
    TM_TRY(prepare_linear(e, e->output));
    e->weights_ready = true;
    return 0;
}

int tm_engine_start(tm_engine* e)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(e->weights_ready, "process_weights first");
    if (e->started) {
        return 0;
    }
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    const tm_engine_config& c = e->cfg;
    const tm_model_config&  m = c.model;
    const int bits = c.quant_policy == 0 ? 16 : c.quant_policy;
    e->layout      = KvLayout{e->kv_heads, e->D, c.cache_block_seq_len, bits};
    e->block_bytes = (int64_t)m.layers * e->layout.layer_size();
    e->max_blocks_per_seq = (c.session_len + 63) / 64;

    const int B   = c.max_batch_size;
    e->max_tokens = std::max(B, std::max(64, c.max_prefill_token_num));
    const size_t T = e->max_tokens;
    TM_TRY(dmalloc(&e->d_resid, T * e->hidden));
    TM_TRY(dmalloc(&e->d_x, T * e->hidden));
    TM_TRY(dmalloc(&e->d_tmp, T * e->hidden));
    TM_TRY(dmalloc(&e->d_qkv, T * e->qkv_n));
    TM_TRY(dmalloc(&e->d_attn, T * e->q_heads * e->D));
    TM_TRY(dmalloc(&e->d_act, T * std::max(e->inter, e->shared_inter)));
    if (e->shared_inter > 0) {
        TM_TRY(dmalloc(&e->d_shared, T * e->hidden));
    }
    TM_TRY(dmalloc(&e->d_logits, (size_t)B * e->vocab_local));
    TM_TRY(dmalloc(&e->d_last, (size_t)B * e->hidden));
    // split-K workspace: decode-sized problems only (M <= 64 rows x widest N x 16 slabs)
    const int wide_n = std::max(std::max(e->qkv_n, 2 * std::max(e->inter, e->shared_inter)), e->hidden);  // widest linear output
    e->gemm_ws_bytes = (size_t)16 * 64 * wide_n * sizeof(float);
    TM_HIP_CHECK(hipMalloc((void**)&e->d_gemm_ws, e->gemm_ws_bytes));
    e->scratch.ws = e->d_gemm_ws, e->scratch.ws_bytes = e->gemm_ws_bytes, e->scratch.rows = e->max_tokens;
    // a dense format that needs its GEMM input quantised (the engine brings buffers to no other): codes and scales of ONE GEMM input (the
    // widest K of a dense linear), written by the quantiser in front of every dense GEMM -- sized here, nothing is allocated in a forward
    if (const ActQuant q = linear_act_quant(linear_format(m.weight_type, m.fp8_scale_mode, false, m.group_size), false); q != ActQuant::NONE) {
        const size_t wide_k = std::max(std::max(e->hidden, e->q_heads * e->D), std::max(e->inter, e->shared_inter));
        const bool   mx     = q == ActQuant::MXFP4_ROW32;  // e2m1 pairs + an e8m0 byte per 32 channels; else e4m3 / int8 codes + one fp32 scale per token
        TM_HIP_CHECK(hipMalloc(&e->scratch.xq, T * (mx ? wide_k / 2 : wide_k)));
        TM_HIP_CHECK(hipMalloc(&e->scratch.sx, T * (mx ? wide_k / 32 : sizeof(float))));
    }
    {
        const size_t tiles = (size_t)(e->hidden + 63) / 64;
        TM_TRY(dmalloc(&e->d_ss, tiles * kFoldMaxRows));
        // arrival counters: one per (column tile, row block) of the widest decode linear at its narrowest tile (64 columns, 32 rows)
        const size_t ntk = (size_t)(wide_n + 63) / 64 * (kFoldMaxRows / 32);
        const char* fm   = getenv("TM_FOLD_MAX_M");
        // default 64: at batch 128 (BASELINE config 3) the folded layer is parity-green but measured SLOWER than the reduce-norm launches it
        // removes (InternLM2-20B: 10.83 .. 10.91 vs 10.43 ms per step, profiles/r06_fold128_*): its producers are limited to the 32-row-block
        // tiles (every weight unit read by four row blocks), the 128-row tile with 10 slices + the fused reduce-norm wins w2 by 4 us
        e->fold_max_rows = fm ? std::min(kFoldMaxRows, std::max(1, atoi(fm))) : 64;
        TM_TRY(dmalloc(&e->d_tickets, ntk));
        TM_HIP_CHECK(hipMemset(e->d_tickets, 0, ntk * sizeof(unsigned)));
        // Default 0 since round 6: the folded layer is a departure from the reference's rounding sequence (one fp16 rounding
        // of the normalised activations instead of two) and a default-on departure has to pay more than box noise -- four interleaved runs per arm
        // on one box: 19 278.6 (fold 3) vs 19 283.5 tok/s (fold 0) on the driver command, 17 632.6 vs 17 619.5 over the 1k-out run
        // (profiles/r06_fold_ab.txt).  TM_FOLD_NORM=3 runs it (bit 0: wo -> w1w3, bit 1: w2 -> w_qkv); every test of it stays.
        const char* fold = getenv("TM_FOLD_NORM");
        e->fold_norm     = (!e->use_comm && m.weight_type == 0 && m.moe_experts == 0 && e->hidden % 64 == 0) ? (fold ? atoi(fold) & 3 : 0) : 0;
    }
    {
        // sliding windows: a window that covers the whole session is full attention; an engine left without a windowed layer and without
        // sinks is the engine it was before the feature (fused MFMA path, same launches)
        e->windowed = m.attn_sinks != 0;
        for (int i = 0; i < m.layers; ++i) {
            const int w         = e->layer_windows.empty() ? m.attn_window : e->layer_windows[i];
            e->layers[i].window = w >= c.session_len ? 0 : w;
            e->windowed |= e->layers[i].window > 0;
        }
        TM_REQUIRE(c.quant_policy != 42 || !e->windowed,
                   "quant_policy 42 (TurboQuant KV) with a sliding window or attention sinks is not built");
        // the folded norm divides by hidden and has no bias term: a zero-padded model or an o_proj bias runs the norm launches
        if (e->windowed || e->hidden_valid != e->hidden || m.attn_out_bias) {
            e->fold_norm = 0;
        }
        // block ring: only when EVERY layer is windowed (one KV block holds all layers, so one full-attention layer keeps every
        // block of the context alive); the ring is sized by the largest window and by max_tokens, the most tokens prefill_slots
        // hands one sequence per forward.  A ring as long as the longest block table row would save nothing: off.
        int w_max = 0, w_min = m.layers > 0 ? e->layers[0].window : 0;
        for (int i = 0; i < m.layers; ++i) {
            w_max = std::max(w_max, e->layers[i].window);
            w_min = std::min(w_min, e->layers[i].window);
        }
        e->ring_blocks = 0;
        if (e->kv_ring_on && w_min > 0) {
            const int r    = kv_ring_blocks(w_max, e->max_tokens);
            e->ring_blocks = r < e->max_blocks_per_seq ? r : 0;
        }
    }
    if (m.moe_experts > 0) {
        TM_HIP_CHECK(hipMalloc(&e->d_moe_ws, moe_workspace_bytes(e->layers[0].moe, e->max_tokens)));
    }
    // prefill scratch: every sequence padded to a multiple of 64 keys
    e->kflat_stride = ((e->max_tokens + c.session_len + 63) / 64) * 64 + 64 * (std::min(B, e->max_tokens) + 1);
    TM_TRY(dmalloc(&e->d_kflat, (size_t)e->kv_heads * e->kflat_stride * e->D));
    TM_TRY(dmalloc(&e->d_vflat, (size_t)e->kv_heads * e->kflat_stride * e->D));

    // RoPE table
    e->rope_max_pos = c.session_len + 1;
    {
        std::vector<half_t> tab((size_t)e->rope_max_pos * e->D);
        TM_TRY(build_rope_table_ex(tab.data(), e->rope_max_pos, model_rope_param(e)));
        // dynamic NTK: only a prompt longer than rope_max_position_embeddings takes a base of its own, so an engine whose session_len
        // does not exceed it keeps the one table (type 4 at the model's base IS the default table) and everything that goes with it
        const bool per_seq = m.rope_type == 4 && m.rope_factor > 1.f && m.rope_max_position_embeddings > 0
                             && c.session_len > m.rope_max_position_embeddings;
        const size_t regions = per_seq ? (size_t)1 + B : 1;
        TM_REQUIRE(regions * e->rope_max_pos < ((size_t)1 << 31), "per-sequence RoPE tables: (1 + max_batch_size) x (session_len + 1) rows reach 2^31");
        // (allocated in front of the KV pool: the pool is derived from what is free after this)
        if (hipMalloc((void**)&e->d_rope, regions * tab.size() * sizeof(half_t)) != hipSuccess) {
            (void)hipGetLastError();
            set_last_error("RoPE table allocation failed");
            return TM_OOM;
        }
        TM_HIP_CHECK(hipMemcpy(e->d_rope, tab.data(), tab.size() * 2, hipMemcpyHostToDevice));
        if (e->mrope_section[0] + e->mrope_section[1] + e->mrope_section[2] > 0 && c.tp == 1 && c.quant_policy != 42) {
            // M-RoPE model that can take multimodal input: the slots' position deltas, read by every static decode step
            TM_TRY(dmalloc(&e->d_pos_delta, (size_t)B));
            TM_HIP_CHECK(hipMemset(e->d_pos_delta, 0, (size_t)B * sizeof(int)));
        }
        if (per_seq) {
            TM_TRY(dmalloc(&e->d_rope_row0, (size_t)B));
            TM_HIP_CHECK(hipMemset(e->d_rope_row0, 0, (size_t)B * sizeof(int)));
            e->h_rope_row0.assign(B, 0);
        }
    }

    TM_TRY(dmalloc(&e->d_ids, (size_t)B));
    TM_TRY(dmalloc(&e->d_next_ids, (size_t)B));
    TM_TRY(dmalloc(&e->d_k_len, (size_t)B));
    TM_TRY(dmalloc(&e->d_cu_q, (size_t)B + 1));
    TM_TRY(dmalloc(&e->d_cu_q_b, (size_t)B + 1));
    TM_TRY(dmalloc(&e->d_cu_koff, (size_t)B + 1));
    TM_TRY(dmalloc(&e->d_rows, (size_t)B));
    TM_TRY(dmalloc(&e->d_generated, (size_t)B * c.session_len));
    TM_TRY(dmalloc(&e->d_step, (size_t)1));
    TM_TRY(dmalloc(&e->d_prefill_ids, T));
    TM_TRY(dmalloc(&e->d_argmax_val, (size_t)B));
    TM_TRY(dmalloc(&e->d_cand, (size_t)B * 2));
    TM_TRY(dmalloc(&e->d_cand_all, (size_t)B * 2 * c.tp));
    TM_TRY(dmalloc(&e->d_block_ptrs, (size_t)B * e->max_blocks_per_seq));
    TM_TRY(dmalloc(&e->d_cu_block_nums, (size_t)B + 1));
    {
        std::vector<int> cu(B + 1);
        for (int b = 0; b <= B; ++b) {
            cu[b] = b * e->max_blocks_per_seq;
        }
        TM_HIP_CHECK(hipMemcpy(e->d_cu_block_nums, cu.data(), cu.size() * 4, hipMemcpyHostToDevice));
    }
    const int max_splits = 16;
    TM_HIP_CHECK(hipMalloc((void**)&e->d_attn_ws, decode_attention_workspace_bytes(B, e->q_heads, e->D, max_splits)));

    // KV pool
    int64_t blocks = c.cache_blocks;
    if (blocks <= 0) {
        size_t free_b = 0, total_b = 0;
        TM_HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        const float frac = c.cache_max_entry_count > 0.f ? c.cache_max_entry_count : 0.8f;
        blocks           = (int64_t)((double)free_b * frac / (double)e->block_bytes);
        const int64_t need = (int64_t)B * kv_blocks_owned(e->max_blocks_per_seq, e->ring_blocks);  // no sequence can own more
        blocks           = std::min(blocks, need);
    }
    TM_REQUIRE(blocks >= 1, "no memory for KV blocks");
    if (hipMalloc((void**)&e->pool, (size_t)blocks * e->block_bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_last_error("KV pool allocation failed");
        return TM_OOM;
    }
    TM_HIP_CHECK(hipMemsetAsync(e->pool, 0, (size_t)blocks * e->block_bytes, e->stream));
    e->num_blocks = blocks;
    e->free_blocks.resize(blocks);
    for (int64_t i = 0; i < blocks; ++i) {
        e->free_blocks[i] = (int)(blocks - 1 - i);
    }
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    e->started = true;
    // the reference's switches: TM_GEMM_IMPORT=<file> loads a dispatch table, TM_GEMM_TUNE=1 measures the decode batch
    // (max_batch_size rows) now, TM_GEMM_EXPORT=<file> writes the table
    if (const char* imp = getenv("TM_GEMM_IMPORT")) {
        if (dec32_table_import(imp)) {
            fprintf(stderr, "[tm] TM_GEMM_IMPORT: nothing read from %s\n", imp);
        }
    }
    const char* tune = getenv("TM_GEMM_TUNE");
    if (tune && atoi(tune) && B <= 256) {
        const char* v = getenv("TM_GEMM_TUNE_VERBOSE");
        if (tune_decode_gemms(e, B, v && atoi(v))) {  // not fatal: the heuristic tilings stay
            fprintf(stderr, "[tm] TM_GEMM_TUNE failed (%s); keeping the heuristic tilings\n", tm_last_error());
        }
    }
    if (const char* exp = getenv("TM_GEMM_EXPORT")) {
        TM_TRY(dec32_table_export(exp));
    }
    return 0;
}

int tm_engine_sync(tm_engine* e)
{
    TM_REQUIRE(e, "null pointer");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    TM_TRY(device_marks_fetch(e, false));
    return device_marks_check(e);
}

int tm_engine_fetch(tm_engine* e, int* host_out, int* n_generated)
{
    TM_REQUIRE(e && host_out && n_generated, "null pointer");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    TM_TRY(device_marks_fetch(e, false));
    // the tokens are handed over in any case (those of the steps before a communicator give-up are valid); the status says
    // whether every step behind them was
    TM_HIP_CHECK(hipMemcpy(host_out, e->d_generated, (size_t)e->batch * e->max_new * 4, hipMemcpyDeviceToHost));
    const int rc = device_marks_check(e);
    if (rc && e->steps_valid < 0) {
        e->steps_valid = e->steps_fetched;  // the mark was first seen now: what an earlier, clean fetch reported is known to be valid
    }
    // after a communicator give-up *n_generated = the columns known to be valid (the step count of the last clean fetch): the
    // caller can keep those and must discard the rest; the status says so
    *n_generated = rc ? (e->steps_valid < 0 ? 0 : e->steps_valid) : e->steps_done;
    if (!rc) {
        e->steps_fetched = e->steps_done;
    }
    return rc;
}

int tm_engine_fetch_logits(tm_engine* e, void* host_out)
{
    TM_REQUIRE(e && host_out, "null pointer");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    TM_HIP_CHECK(hipMemcpy(host_out, e->d_logits, (size_t)e->batch * e->vocab_local * 2, hipMemcpyDeviceToHost));
    return 0;
}

int tm_engine_debug_read(tm_engine* e, int what, int a, int b, void* host_out, int64_t bytes)
{
    TM_REQUIRE(e && host_out && e->started, "null pointer / engine not started");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    if (what == 0) {  // residual stream of the last forward: rows [0, a)
        TM_REQUIRE(a >= 1 && a <= e->max_tokens && bytes == (int64_t)a * e->hidden * 2, "residual rows / byte count");
        TM_HIP_CHECK(hipMemcpy(host_out, e->d_resid, (size_t)bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    if (what == 1) {  // KV block b of static-batch sequence a (all layers, the reference's block byte layout)
        // b is a LOGICAL block.  With a block ring h_blocks[a] is the ring: logical block b lives in h_blocks[a][b % R] until logical
        // block b + R is written over it, i.e. while b >= ceil(ctx / 64) - R (ctx = the tokens cached so far)
        TM_REQUIRE(a >= 0 && a < (int)e->h_blocks.size() && a < (int)e->h_len.size() && b >= 0, "sequence / block index");
        const int owned   = (int)e->h_blocks[a].size();
        const int logical = (e->h_len[a] + e->max_new + 63) / 64;
        const int written = (e->h_len[a] + std::max(e->steps_done, 1) - 1 + 63) / 64;
        TM_REQUIRE(owned > 0 && b < logical, "sequence / block index");
        TM_REQUIRE(b >= written - owned, "KV block was overwritten by the sequence's block ring (it lies in front of the window)");
        TM_REQUIRE(bytes == (int64_t)e->block_bytes, "byte count must be the block size");
        TM_HIP_CHECK(hipMemcpy(host_out, e->pool + (int64_t)e->h_blocks[a][b % owned] * e->block_bytes, (size_t)bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    if (what == 2) {  // int64: scheduler steps whose decode rows rode on a prefill forward (mixed steps)
        TM_REQUIRE(bytes == 8, "byte count must be 8");
        *(int64_t*)host_out = e->mixed_steps;
        return 0;
    }
    if (what == 3) {  // int64: decode steps issued while the previous one was unretired (two-phase overlap, TM_ASYNC_STEP)
        TM_REQUIRE(bytes == 8, "byte count must be 8");
        *(int64_t*)host_out = e->overlapped_steps;
        return 0;
    }
    set_last_error("tm_engine_debug_read: unknown selector");
    return 1;
}

int tm_engine_rope_info(tm_engine* e, int* per_seq_tables, int64_t* table_bytes)
{
    TM_REQUIRE(e && e->started, "null pointer / engine not started");
    const bool on = e->d_rope_row0 != nullptr;
    if (per_seq_tables) *per_seq_tables = on ? 1 : 0;
    if (table_bytes) *table_bytes = on ? (int64_t)e->cfg.max_batch_size * e->rope_max_pos * e->D * (int64_t)sizeof(half_t) : 0;
    return 0;
}

int tm_engine_kv_info(tm_engine* e, int* ring_blocks, int64_t* free_blocks)
{
    TM_REQUIRE(e && e->started, "null pointer / engine not started");
    if (e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    if (ring_blocks) *ring_blocks = e->ring_blocks;
    if (free_blocks) *free_blocks = e->sched ? (int64_t)e->sched->n_free_blocks() : (int64_t)e->free_blocks.size();
    return 0;
}

tm_stream_t tm_engine_stream(tm_engine* e)
{
    return e ? (tm_stream_t)e->stream : nullptr;
}

int tm_engine_stats(tm_engine* e, int64_t* weight_bytes, int64_t* kv_bytes_per_token, int64_t* num_blocks,
                    int* decode_splits)
{
    TM_REQUIRE(e, "null pointer");
    int64_t wb = 0;
    for (auto& L : e->layers) {
        for (const LinearSlots* l : {&L.qkv, &L.wo, &L.w13, &L.w2}) {
            wb += (int64_t)linear_weight_bytes(l->w);
        }
        if (L.is_moe) {
            for (int x = 0; x < L.moe.experts; ++x) {
                wb += (int64_t)linear_weight_bytes(L.moe.w13[x]) + (int64_t)linear_weight_bytes(L.moe.w2[x]);
            }
        }
    }
    wb += (int64_t)linear_weight_bytes(e->output.w);
    if (weight_bytes) *weight_bytes = wb;
    if (kv_bytes_per_token) *kv_bytes_per_token = e->started ? e->block_bytes / 64 : 0;
    if (num_blocks) *num_blocks = e->num_blocks;
    if (decode_splits) *decode_splits = e->decode_splits;
    return 0;
}

int tm_engine_destroy(tm_engine* e)
{
    if (!e) {
        return 0;
    }
    (void)tm_engine_serve_stop(e);
    (void)hipSetDevice(e->cfg.device);
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
    }
    if (e->graph) {
        (void)hipGraphExecDestroy(e->graph);
    }
    if (e->graph_spec) {
        (void)hipGraphExecDestroy(e->graph_spec);
    }
    if (e->graph_cb) {
        (void)hipGraphExecDestroy(e->graph_cb);
    }
    if (e->aux_stream) {
        (void)hipStreamDestroy(e->aux_stream);
        (void)hipEventDestroy(e->ev_aux_fork);
        (void)hipEventDestroy(e->ev_aux_join);
    }
    for (int i = 0; i < 2; ++i) {
        for (void* q : {(void*)e->h_cb_lp_vals[i], (void*)e->h_cb_lp_idx[i], (void*)e->h_cb_lp_num[i], (void*)e->h_cb_lp_sel[i]}) {
            if (q) {
                (void)hipHostFree(q);
            }
        }
        if (e->h_step_pin[i]) {
            (void)hipHostFree(e->h_step_pin[i]);
            (void)hipEventDestroy(e->ev_step[i]);
        }
    }
    for (void* q : {(void*)e->d_active, (void*)e->d_pf_k_len, (void*)e->d_pf_cu_q, (void*)e->d_pf_block_ptrs, (void*)e->d_first_ids, (void*)e->d_temp, (void*)e->d_topp, (void*)e->d_minp,
                    (void*)e->d_u, (void*)e->d_topk, (void*)e->d_seed, e->d_sample_ws, (void*)e->d_logits_gather, (void*)e->d_logits_full,
                    (void*)e->d_seen, (void*)e->d_lp_rep,
                    (void*)e->d_lp_minlen, (void*)e->d_lp_ban, (void*)e->d_lp_end, (void*)e->d_lpr_vals, (void*)e->d_lpr_idx, (void*)e->d_lpr_num,
                    (void*)e->d_lpr_sel, (void*)e->d_kept, (void*)e->d_cb_lp_vals, (void*)e->d_cb_lp_idx, (void*)e->d_cb_lp_num, (void*)e->d_cb_lp_sel,
                    (void*)e->d_score_logits, (void*)e->d_score_nll, (void*)e->d_score_tgt}) {
        if (q) {
            (void)hipFree(q);
        }
    }
    for (auto& L : e->layers) {
        for (LinearSlots* l : {&L.qkv, &L.wo, &L.w13, &L.w2}) {
            linear_weight_free(l->w);
        }
        for (auto& l : L.ex13) {
            linear_weight_free(l.w);
        }
        for (auto& l : L.ex2) {
            linear_weight_free(l.w);
        }
        if (L.is_moe) {
            moe_free(L.moe);
        }
    }
    for (void* q : {e->d_moe_ws, (void*)e->d_shared}) {
        if (q) {
            (void)hipFree(q);
        }
    }
    linear_weight_free(e->output.w);
    for (auto& kv : e->slots) {
        if (kv.second.dev) {
            (void)hipFree(kv.second.dev);
        }
    }
    void* bufs[] = {e->pool, e->d_block_ptrs, e->d_cu_block_nums, e->d_resid, e->d_x, e->d_qkv, e->d_attn, e->d_act,
                    e->d_tmp, e->d_logits, e->d_last, e->d_gemm_ws, e->scratch.xq, e->scratch.sx, e->d_attn_ws, e->d_kflat, e->d_vflat, e->d_rope,
                    e->d_ids, e->d_k_len, e->d_cu_q, e->d_cu_q_b, e->d_cu_koff, e->d_rows, e->d_generated, e->d_step,
                    e->d_prefill_ids, e->d_argmax_val, e->d_cand, e->d_cand_all, e->d_next_ids, e->d_ss, e->d_tickets,
                    e->d_rope_row0, e->d_pos_delta, e->d_emb_rows, e->d_emb_index, e->d_mrope_pos, e->d_spec_hist, e->d_spec_len,
                    e->d_spec_emitted, e->d_spec_drafts, e->d_spec_ndraft, e->d_spec_ids, e->d_spec_out, e->d_spec_cu_q, e->d_spec_k_len,
                    e->d_spec_step, e->d_spec_totals, e->d_spec_logits, e->d_spec_attn_ws};
    for (void* p : bufs) {
        if (p) {
            (void)hipFree(p);
        }
    }
    for (int r = 0; r < 8; ++r) {
        (void)tm_p2p_segment_close(e->p2p_peer[r], 1);
    }
    (void)tm_p2p_segment_close(e->p2p_seg, 0);
    if (e->p2p_state) {
        (void)hipFree(e->p2p_state);
    }
    if (e->comm) {
        (void)ncclCommDestroy(e->comm);
    }
    if (e->comm_stream) {
        (void)hipStreamDestroy(e->comm_stream);
    }
    for (hipEvent_t ev : e->pipe_events) {
        (void)hipEventDestroy(ev);
    }
    if (e->stream) {
        (void)hipStreamDestroy(e->stream);
    }
    delete e;
    return 0;
}

}  // extern "C"
