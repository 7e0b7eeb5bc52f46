// The forward pass of the engine (LanguageModel::Forward / UnifiedDecoder::Forward, src/turbomind/models/language_model.cc:493-542,
// models/llama/unified_decoder.cc:163-380): one forward over M tokens (decode, prefill, mixed), the static-batch prefill / decode entry
// points and the hipGraph capture of the decode step.  See engine.hip for the overview.
#include "engine_internal.h"

namespace tmk {

__global__ void advance_kernel(int* k_len, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) {
        k_len[b] += 1;
    }
}

// continuous batching: only slots that hold a running sequence advance
__global__ void advance_active_kernel(int* k_len, const int* active, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch && active[b]) {
        k_len[b] += 1;
    }
}

// continuous batching: a finished / cancelled slot goes back to the scratch block (no host memory involved: the launch needs
// no synchronisation, so it can queue up behind a decode step that is still running)
int launch_advance_active(int* k_len, const int* active, int n, hipStream_t st)
{
    advance_active_kernel<<<(n + 63) / 64, 64, 0, st>>>(k_len, active, n);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ids -> generated[b][step]; step++ (single thread does the counter after everybody read it)
__global__ void record_kernel(const int* ids, int* generated, int* step_counter, int batch, int max_new)
{
    const int b    = blockIdx.x * blockDim.x + threadIdx.x;
    const int step = *step_counter;
    if (b < batch && step < max_new) {
        generated[(size_t)b * max_new + step] = ids[b];
    }
    __syncthreads();
    if (b == 0) {
        *step_counter = step + 1;
    }
}

// pick the global arg-max out of tp (value, index) candidates per sequence
__global__ void pick_kernel(int* out_ids, const float* cand /*[tp][B][2]*/, int tp, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) {
        return;
    }
    float best = -INFINITY;
    int   bi   = 0;
    for (int r = 0; r < tp; ++r) {
        const float v = cand[((size_t)r * batch + b) * 2];
        const int   i = __float_as_int(cand[((size_t)r * batch + b) * 2 + 1]);
        if (v > best || (v == best && i < bi)) {
            best = v;
            bi   = i;
        }
    }
    out_ids[b] = bi;
}

// all-gathered vocabulary shards [tp][n][vl] -> full rows [n][tp * vl] (16-byte vectors; vl % 8 == 0)
__global__ void gather_vocab_kernel(half_t* __restrict__ full, const half_t* __restrict__ shards, int n, int vl, int tp)
{
    const size_t nvec = (size_t)n * tp * (vl / 8);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
        const int    v = (int)(i % (vl / 8));
        const int    r = (int)((i / (vl / 8)) % tp);
        const size_t b = i / ((size_t)(vl / 8) * tp);
        *(u32x4*)(full + (b * tp + r) * vl + (size_t)v * 8) = *(const u32x4*)(shards + ((size_t)r * n + b) * vl + (size_t)v * 8);
    }
}

__global__ void pack_candidates_kernel(float* cand, const int* ids, const half_t* vals, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < batch) {
        cand[b * 2]     = (float)vals[b];
        cand[b * 2 + 1] = __int_as_float(ids[b]);
    }
}

// A range of a forward's rows and the sequences that own them: the whole forward, the prefill rows or the decode rows of a mixed
// forward, a micro-batch.  A row half has rows only (the row-wise operators read r0 / rows and nothing else).
struct Rows {
    int        r0, rows;  // first row, row count
    int        s0, nseq;  // first sequence in the forward's per-sequence arrays (block table, d_cu_koff, rope_row0), sequence count
    const int* cu_q;      // [nseq + 1], counted from the range's first row
    const int* k_len;     // [nseq] context lengths
};

static KvCacheView cache_view(const tm_engine* e, int layer, int s0 = 0)
{
    KvCacheView v{};
    v.block_ptrs    = e->d_block_ptrs + (size_t)s0 * e->max_blocks_per_seq;  // cu_block_nums[b] = b * max_blocks_per_seq (create())
    v.cu_block_nums = e->d_cu_block_nums;
    static const bool rect = !getenv("TM_ATTN_RECT") || atoi(getenv("TM_ATTN_RECT")) != 0;  // A/B switch
    v.block_stride  = rect ? e->max_blocks_per_seq : 0;
    v.layer_offset  = (int64_t)layer * e->layout.layer_size();
    v.layout        = e->layout;
    return v;
}

size_t prof_event(tm_engine* e)
{
    if (e->prof_used == e->prof_pool.size()) {
        hipEvent_t ev;
        (void)hipEventCreate(&ev);
        e->prof_pool.push_back(ev);
    }
    (void)hipEventRecord(e->prof_pool[e->prof_used], e->stream);
    return e->prof_used++;
}

// A dense linear of the model's format (linear_forward, linear.hip), reduced into y.  It alone hands the arrival counters on, so only
// it may run a measured in-launch merge shape.
static int linear_plain(tm_engine* e, LinearSlots& l, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated)
{
    LinearScratch s = e->scratch;
    s.tickets       = e->d_tickets;
    return linear_forward(l.w, x, ldx, y, ldy, M, gated, s, false, nullptr, e->stream);
}

// A linear whose consumer can sum the split-K slices itself (the residual-norm launch, the decode attention's fused prologue):
// `defer` and a split launch leave the fp32 slabs in d_gemm_ws, *slabs > 1; otherwise y holds the result and *slabs = 1.
// (No arrival counters here, unlike linear_plain, even when nothing is deferred: launch_linear then runs a merge shape as the plain form
// of the same tile.)
static int linear_deferrable(tm_engine* e, LinearSlots& l, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated, bool defer,
                             int* slabs)
{
    return linear_forward(l.w, x, ldx, y, ldy, M, gated, e->scratch, defer, slabs, e->stream);
}

// row-parallel linear followed by (all-reduce +) residual + RMSNorm; without a communicator the norm launch sums the slabs
// (bias: the o_proj bias, r = h(h(r + out) + bias) -- the HAS_BIAS arm of the norm kernel; nullptr for every other linear)
static int linear_residual_norm(tm_engine* e, LinearSlots& l, const half_t* x, int ldx, int M, const half_t* norm_w,
                                int gemm_cat, const half_t* bias = nullptr)
{
    int slabs = 1;
    TM_PROF(gemm_cat, TM_TRY(linear_deferrable(e, l, x, ldx, e->d_tmp, e->hidden, M, false, !e->use_comm, &slabs)));
    if (slabs > 1) {
        TM_PROF(P_RES_NORM, TM_TRY(launch_residual_rmsnorm(e->d_x, e->d_resid, nullptr, e->d_gemm_ws, slabs, bias, norm_w,
                                                           e->cfg.model.rms_eps, M, e->hidden, e->stream, e->hidden_valid)));
        return 0;
    }
    return reduce_residual_norm(e, M, norm_w, bias);
}

// ---- RMSNorm folded into the decode GEMMs (tp = 1, dense u4 layers, M <= 64; NormFold in tm_kernels.h) ----------------------------
// the tiling of a folded launch: dec32_pick_fold's, its split-K fitted to the engine's workspace
static void fold_tiling(tm_engine* e, const LinearWeight& w, int M, int* shape, int* splits, bool producer)
{
    dec32_pick_fold(w, M, producer, shape, splits);
    *splits = fit_splits(e, M, w.N, *splits);
}

static bool fold_ok(const tm_engine* e, const Layer& L, int M)
{
    return e->fold_norm != 0 && !L.is_moe && M <= e->fold_max_rows && dec32_supported(L.qkv.w, M) && dec32_supported(L.wo.w, M) && dec32_supported(L.w13.w, M)
           && dec32_supported(L.w2.w, M);
}

// consumer: y = (x . W) * inv[m] (x = r . g of the producing GEMM); ss_tiles == 0: x is already normalised (plain GEMM)
static int linear_fold_consume(tm_engine* e, LinearSlots& l, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated, int ss_tiles,
                               bool slabs_ok, int* slabs)
{
    int shape, splits;
    fold_tiling(e, l.w, M, &shape, &splits, false);
    const bool mrg = dec32_is_merge_shape(shape);  // split-K merged in the launch: no slab leaves it, whoever consumes
    // a split-K consumer nobody takes slabs from (w1w3; w_qkv without the fused attention prologue): the slices' slabs already carry the row
    // factor (it is applied to the accumulators before ANY epilogue, and a sum of scaled slices is the scaled sum), so the plain reduce launch
    // finishes them -- what the 128-row tile needs at batch 128, where one slice per column tile leaves half the CUs idle (round 6)
    const bool reduce_after = !slabs_ok && !mrg && splits > 1 && M > 64;
    if (!slabs_ok && !mrg && !reduce_after) {
        splits = 1;
    }
    NormFold nf{};
    nf.ss_in    = ss_tiles > 0 ? e->d_ss : nullptr;
    nf.ss_tiles = ss_tiles;
    nf.inv_h    = 1.0f / (float)e->hidden;
    nf.eps      = e->cfg.model.rms_eps;
    nf.tickets  = e->d_tickets;
    int nslab   = 1;
    TM_TRY(launch_linear_dec32(l.w, x, ldx, y, ldy, M, gated, shape, splits, e->d_gemm_ws, &nslab, e->stream, (ss_tiles > 0 || mrg) ? &nf : nullptr));
    if (reduce_after && nslab > 1) {
        TM_TRY(launch_splitk_reduce(y, ldy, e->d_gemm_ws, nslab, M, l.w.N, gated, e->stream));
        nslab = 1;
    }
    if (slabs) {
        *slabs = nslab;
    }
    return 0;
}

// producer: d_resid += x . W ; d_x = d_resid . norm_w (not normalised) ; d_ss = per-tile sums of squares -> *ss_tiles
static int linear_fold_produce(tm_engine* e, LinearSlots& l, const half_t* x, int ldx, int M, const half_t* norm_w, int* ss_tiles)
{
    int shape, splits;
    fold_tiling(e, l.w, M, &shape, &splits, true);
    NormFold nf{};
    nf.resid   = e->d_resid;
    nf.norm_w  = norm_w;
    nf.ss_out  = e->d_ss;
    nf.tickets = e->d_tickets;
    TM_TRY(launch_linear_dec32(l.w, x, ldx, e->d_x, e->hidden, M, false, shape, splits, e->d_gemm_ws, nullptr, e->stream, &nf));
    *ss_tiles = nf.tiles_out;
    return 0;
}

// ---- layer blocks: written once for every schedule; the only places where a Layer's attention features reach a kernel --------------
// w_qkv over R's rows of d_x -> d_qkv.  fold: the consumer of a folded norm (ss_tiles).  fused (decode + int8 KV): the attention kernel
// consumes the GEMM's raw output (fp32 split-K slabs, *slabs > 1, or fp16), applies RoPE and quantises / stores the new K/V itself -> no
// splitk_reduce, no kv_rope_store launch; it defers whenever the launch splits, communicator or not
static int qkv_project(tm_engine* e, Layer& L, const Rows& R, bool fold, bool fused, int ss_tiles, int* slabs)
{
    const half_t* const x = e->d_x + (size_t)R.r0 * e->hidden;
    half_t* const       y = e->d_qkv + (size_t)R.r0 * e->qkv_n;
    TM_PROF(P_GEMM_QKV, TM_TRY(fold  ? linear_fold_consume(e, L.qkv, x, e->hidden, y, e->qkv_n, R.rows, false, ss_tiles, fused, slabs) :
                               fused ? linear_deferrable(e, L.qkv, x, e->hidden, y, e->qkv_n, R.rows, false, true, slabs) :
                                       linear_plain(e, L.qkv, x, e->hidden, y, e->qkv_n, R.rows, false)));
    return 0;
}

// RoPE + K/V quantise-store of R's rows of d_qkv (rope_row0: the forward's per-sequence table rows, nullptr: one table)
// (M-RoPE: a multimodal prefill forward carries coordinates per row, e->fw_mrope_pos; a static decode step of a model with sections the
// slots' position deltas, e->fw_pos_delta -- either one selects the sectioned store, neither: the plain kernel as before)
static int kv_store(tm_engine* e, const Layer& L, const KvCacheView& cv, const Rows& R, hipStream_t st, const int* rope_row0)
{
    if (e->fw_mrope_pos || e->fw_pos_delta) {
        TM_REQUIRE(!rope_row0, "internal: M-RoPE sections with per-sequence RoPE tables");  // tm_engine_set_mrope_section refuses rope_type 4
        const int* sec = e->mrope_section;
        return launch_kv_rope_store_mrope(e->d_qkv + (size_t)R.r0 * e->qkv_n, e->q_heads, R.cu_q, R.k_len, R.nseq, R.rows, e->d_rope,
                                          e->rope_max_pos, e->fw_mrope_pos ? e->fw_mrope_pos + (size_t)R.r0 * 3 : nullptr,
                                          e->fw_pos_delta ? e->fw_pos_delta + R.s0 : nullptr, sec[0], sec[1], sec[2], cv, st, L.qkv_bias,
                                          L.q_norm, L.k_norm, e->cfg.model.rms_eps);
    }
    return launch_kv_rope_store(e->d_qkv + (size_t)R.r0 * e->qkv_n, e->q_heads, R.cu_q, R.k_len, R.nseq, R.rows, e->d_rope, e->rope_max_pos, cv,
                                st, L.qkv_bias, L.q_norm, L.k_norm, e->cfg.model.rms_eps, rope_row0 ? rope_row0 + R.s0 : nullptr);
}

// prefill attention of R's sequences: their K/V (stored before: kv_store) flattened into the scratch, attention over it
static int prefill_attention_block(tm_engine* e, const Layer& L, const KvCacheView& cv, const Rows& R, int max_q_len, int max_k_len,
                                   int kflat_stride, float scale_log2)
{
    // (a windowed layer flattens from the first 64-key stage of its window on: launch_flatten_kv_window; window 0 = the whole context)
    TM_PROF(P_KV_STORE, TM_TRY(launch_flatten_kv_window(e->d_kflat, e->d_vflat, 1, e->d_cu_koff + R.s0, R.k_len, R.cu_q, L.window, R.nseq,
                                                       max_k_len, kflat_stride, cv, e->stream)));
    PrefillAttnParams p{};
    p.q          = e->d_qkv + (size_t)R.r0 * e->qkv_n;
    p.q_stride   = e->qkv_n;
    p.out        = e->d_attn + (size_t)R.r0 * e->q_heads * e->D;
    p.k          = e->d_kflat;
    p.vt         = e->d_vflat;
    p.k_stride   = kflat_stride;
    p.cu_q_len   = R.cu_q;
    p.cu_k_off   = e->d_cu_koff + R.s0;  // offsets into the flat K / V^T scratch of the WHOLE forward
    p.k_len      = R.k_len;
    p.batch      = R.nseq;
    p.max_q_len  = max_q_len;
    p.q_heads    = e->q_heads;
    p.kv_heads   = e->kv_heads;
    p.scale_log2 = scale_log2;
    p.head_dim   = e->D;
    p.window     = L.window;
    p.sinks      = L.sinks;
    TM_PROF(P_ATTN, TM_TRY(launch_prefill_attention(p, e->stream)));
    return 0;
}

// verify attention of R's sequences (speculative decoding: max_q_len = k + 1 rows each; their K/V stored before: kv_store) straight over
// the paged cache -- int8 / int4 KV at head_dim 128, no window, no sinks (tm_engine_set_speculative refuses those models)
static int verify_attention_block(tm_engine* e, const KvCacheView& cv, const Rows& R, int max_q_len, float scale_log2)
{
    VerifyAttnParams p{};
    p.q          = e->d_qkv + (size_t)R.r0 * e->qkv_n;
    p.q_stride   = e->qkv_n;
    p.out        = e->d_attn + (size_t)R.r0 * e->q_heads * e->D;
    p.cu_q_len   = R.cu_q;
    p.k_len      = R.k_len;
    p.batch      = R.nseq;
    p.q_heads    = e->q_heads;
    p.scale_log2 = scale_log2;
    p.splits     = e->decode_splits;
    p.partial_o  = e->d_spec_attn_ws;
    p.partial_ml = e->d_spec_attn_ws + (size_t)R.rows * e->q_heads * e->decode_splits * e->D;
    p.cache      = cv;
    p.max_q_len  = max_q_len;
    TM_PROF(P_ATTN, TM_TRY(launch_verify_attention(p, e->stream)));
    return 0;
}

// decode attention of R's one-token sequences on stream `st`: a pure decode step, or the leading decode rows of a mixed forward.
// prologue_slabs >= 1: the kernel's fused prologue (bias, q/k norm, RoPE, K/V quantise-store) reads the raw projection -- 1: the fp16 rows
// of d_qkv, > 1: that many fp32 split-K slabs in d_gemm_ws; 0 (fp16 KV, head_dim 64, windows, per-sequence RoPE): kv_store first
static int decode_attention_block(tm_engine* e, const Layer& L, const KvCacheView& cv, const Rows& R, int prologue_slabs, float scale_log2,
                                  hipStream_t st, const int* rope_row0)
{
    DecodeAttnParams p{};
    if (prologue_slabs == 0) {
        TM_PROF(P_KV_STORE, TM_TRY(kv_store(e, L, cv, R, st, rope_row0)));
    }
    else {
        p.qkv_slabs  = prologue_slabs > 1 ? e->d_gemm_ws : nullptr;
        p.qkv_f16    = prologue_slabs > 1 ? nullptr : e->d_qkv;
        p.qkv_splits = prologue_slabs > 1 ? prologue_slabs : 0;
        p.qkv_n      = e->qkv_n;
        p.cos_sin    = e->d_rope;
        p.max_pos    = e->rope_max_pos;
        p.qkv_bias   = L.qkv_bias;
        p.q_norm     = L.q_norm;
        p.k_norm     = L.k_norm;
        p.qk_eps     = e->cfg.model.rms_eps;
        p.pos_delta  = e->fw_pos_delta ? e->fw_pos_delta + R.s0 : nullptr;
    }
    p.q          = e->d_qkv;
    p.q_stride   = e->qkv_n;
    p.out        = e->d_attn;
    p.k_len      = R.k_len;
    p.batch      = R.nseq;
    p.q_heads    = e->q_heads;
    p.scale_log2 = scale_log2;
    p.splits     = e->decode_splits;
    p.partial_o  = e->d_attn_ws;
    p.partial_ml = e->d_attn_ws + (size_t)R.nseq * e->q_heads * e->decode_splits * e->D;
    p.cache      = cv;
    p.window     = L.window;
    p.sinks      = L.sinks;
    TM_PROF(P_ATTN, TM_TRY(launch_decode_attention(p, st)));
    return 0;
}

// tp > 1 prefill on the pipe, R's rows: wo -> d_tmp, the exchange of the partial sums started on the side stream (*done)
static int pipe_wo(tm_engine* e, Layer& L, const Rows& R, hipEvent_t* done)
{
    const int kq = e->q_heads * e->D;
    TM_PROF(P_GEMM_O, TM_TRY(linear_plain(e, L.wo, e->d_attn + (size_t)R.r0 * kq, kq, e->d_tmp + (size_t)R.r0 * e->hidden, e->hidden, R.rows, false)));
    return allreduce_rows_side(e, R.r0, R.rows, done);
}

// closes an exchange: R's rows of d_tmp are summed by now (or the stream waits here); residual (+ bias) + RMSNorm of them
static int pipe_close(tm_engine* e, const Rows& R, hipEvent_t done, const half_t* bias, const half_t* norm_w)
{
    const size_t off = (size_t)R.r0 * e->hidden;
    TM_TRY(pipe_wait(e, done));
    TM_PROF(P_RES_NORM, TM_TRY(launch_residual_rmsnorm(e->d_x + off, e->d_resid + off, e->d_tmp + off, nullptr, 0, bias, norm_w,
                                                       e->cfg.model.rms_eps, R.rows, e->hidden, e->stream, e->hidden_valid)));
    return 0;
}

// row-wise dense FFN of R's rows: closes their wo exchange (*done), w1w3 + gated SiLU, w2 -> d_tmp, exchange started (*done)
static int pipe_ffn(tm_engine* e, Layer& L, const Rows& R, hipEvent_t* done)
{
    half_t* const act = e->d_act + (size_t)R.r0 * e->inter;
    const size_t  off = (size_t)R.r0 * e->hidden;
    TM_TRY(pipe_close(e, R, *done, L.wo_bias, L.ffn_norm));
    TM_PROF(P_GEMM_GATE_UP, TM_TRY(linear_plain(e, L.w13, e->d_x + off, e->hidden, act, e->inter, R.rows, true)));
    TM_PROF(P_GEMM_DOWN, TM_TRY(linear_plain(e, L.w2, act, e->inter, e->d_tmp + off, e->hidden, R.rows, false)));
    return allreduce_rows_side(e, R.r0, R.rows, done);
}

// -- the unsplit tail of a layer over all M rows: from the attention output to the next layer's normalised input
static int tail_dense(tm_engine* e, Layer& L, int M, const half_t* next_norm)
{
    TM_TRY(linear_residual_norm(e, L.wo, e->d_attn, e->q_heads * e->D, M, L.ffn_norm, P_GEMM_O, L.wo_bias));
    TM_PROF(P_GEMM_GATE_UP, TM_TRY(linear_plain(e, L.w13, e->d_x, e->hidden, e->d_act, e->inter, M, true)));
    return linear_residual_norm(e, L.w2, e->d_act, e->inter, M, next_norm, P_GEMM_DOWN);
}

// wo's epilogue updates the residual stream and hands r . g + sums of squares to w1w3, whose accumulators take the row factor before
// the gated SiLU; w2 does the same for the next layer's w_qkv when that layer folds too (next_folds; the last layer's w2 feeds the final
// norm and the fp16 lm_head: reduce-norm launch as before).  5 launches per layer instead of 7.  *ss_tiles: what w2 leaves for w_qkv.
static int tail_folded(tm_engine* e, Layer& L, int M, const half_t* next_norm, bool next_folds, int* ss_tiles)
{
    if (e->fold_norm & 1) {
        TM_PROF(P_GEMM_O, TM_TRY(linear_fold_produce(e, L.wo, e->d_attn, e->q_heads * e->D, M, L.ffn_norm, ss_tiles)));
    }
    else {
        TM_TRY(linear_residual_norm(e, L.wo, e->d_attn, e->q_heads * e->D, M, L.ffn_norm, P_GEMM_O, L.wo_bias));
    }
    TM_PROF(P_GEMM_GATE_UP, TM_TRY(linear_fold_consume(e, L.w13, e->d_x, e->hidden, e->d_act, e->inter, M, true, *ss_tiles, false, nullptr)));
    *ss_tiles = 0;
    if ((e->fold_norm & 2) && next_folds) {
        TM_PROF(P_GEMM_DOWN, TM_TRY(linear_fold_produce(e, L.w2, e->d_act, e->inter, M, next_norm, ss_tiles)));
        return 0;
    }
    return linear_residual_norm(e, L.w2, e->d_act, e->inter, M, next_norm, P_GEMM_DOWN);
}

// router + grouped expert FFNs + combine -> d_tmp, then (all-reduce +) residual + RMSNorm as for the dense FFN
static int tail_moe(tm_engine* e, Layer& L, int M, const half_t* next_norm)
{
    TM_TRY(linear_residual_norm(e, L.wo, e->d_attn, e->q_heads * e->D, M, L.ffn_norm, P_GEMM_O, L.wo_bias));
    const half_t* shared = nullptr;
    if (L.has_shared) {
        // Qwen2-MoE: the shared expert is the layer's dense FFN (unified_decoder.cc:295-318); its output waits in d_shared for
        // the combine, which scales it by sigmoid(x . shared_gate) and adds the routed experts (moe_combine_shared_kernel)
        TM_PROF(P_GEMM_GATE_UP, TM_TRY(linear_plain(e, L.w13, e->d_x, e->hidden, e->d_act, e->shared_inter, M, true)));
        TM_PROF(P_GEMM_DOWN, TM_TRY(linear_plain(e, L.w2, e->d_act, e->shared_inter, e->d_shared, e->hidden, M, false)));
        shared = e->d_shared;
    }
    TM_PROF(P_GEMM_GATE_UP, TM_TRY(moe_forward(L.moe, e->d_tmp, e->hidden, e->d_x, e->hidden, M, e->d_moe_ws, nullptr, nullptr, e->stream,
                                               kMoeAll, shared)));
    return reduce_residual_norm(e, M, next_norm);
}

// Tensor-parallel prefill forward, dense layer, from the attention output to the next layer's QKV projection, as two row halves
// A = [0, Ma), B = [Ma, M): every operator here is row-wise, so a half's all-reduce (RCCL on the side stream, engine_comm.hip) runs
// under the other half's GEMMs on the engine stream --
//   engine stream:  wo A | wo B | norm A  w1w3 A  w2 A | norm B  w1w3 B  w2 B | norm A  qkv' A | norm B  qkv' B
//   side stream:         | AR A        | AR B                 | AR A                   | AR B
// (qkv' = the NEXT layer's w_qkv: it hides the last exchange; absent behind the last layer).  Same kernels, same per-row arithmetic
// as the unsplit sequence (reduce_residual_norm's RCCL branch): a row's result does not depend on which rows share its launch, as
// long as both forms pick the same tiling -- they pick per launch size, so equality with the unsplit forward is to rounding, and the
// parity gate is the engine's usual one against the oracle.  Reference role: the overlap the reference gets from its fused
// all-reduce + norm kernel (unified_decoder.cc:278,328; comm/cuda_ipc/fused_allreduce.cu:406-500).
static int forward_tail_two_halves(tm_engine* e, Layer& L, int M, int Ma, const half_t* next_norm, Layer* next)
{
    const Rows half[2] = {{0, Ma}, {Ma, M - Ma}};
    hipEvent_t done[2];
    for (int h = 0; h < 2; ++h) {
        TM_TRY(pipe_wo(e, L, half[h], &done[h]));
    }
    for (int h = 0; h < 2; ++h) {
        TM_TRY(pipe_ffn(e, L, half[h], &done[h]));
    }
    for (int h = 0; h < 2; ++h) {
        TM_TRY(pipe_close(e, half[h], done[h], nullptr, next_norm));
        if (next) {
            TM_TRY(qkv_project(e, *next, half[h], false, false, 0, nullptr));
        }
    }
    return 0;
}

// Tensor-parallel prefill forward whose sequences split into two micro-batches A = sequences [0, seqs_a) = rows [0, rows_a) and B = the
// rest (prefill_slots decides; e->mb): between the embedding and the lm_head the two share nothing -- not even the attention -- so they
// leapfrog through ALL layers, every all-reduce of one running on the side stream under a whole block of the other:
//   engine stream:  attn-block A | attn-block B | ffn A | ffn B | attn-block' A | attn-block' B | ...
//   side stream:                 | AR(wo A)     | AR(wo B)  | AR(w2 A) | AR(w2 B)       | ...
// attn-block = (residual + RMSNorm of the previous layer's w2 sum,) w_qkv, RoPE + K/V quantise-store, flatten, attention, wo;
// ffn = residual + RMSNorm of the wo sum, w1w3 + gated SiLU, w2.  The row-half schedule inside a layer (forward_tail_two_halves) can
// hide AR(wo A) only under wo B and AR(w2 B) only under the next w_qkv A; here every exchange has a third to a half of the other
// micro-batch's layer to hide under (measured with the 1-rank exchange stand-in: profiles/r05_prefill_overlap_emulated_exchange.txt).
// Same kernels and per-row arithmetic as the unsplit forward; dense layers only.
static int forward_layers_two_microbatches(tm_engine* e, int M, int nseq, int max_q_len, int max_k_len, int kflat_stride, float scale_log2,
                                           const int* rope_row0)
{
    const tm_model_config& m       = e->cfg.model;
    const int              sa      = e->mb.seqs_a;
    const Rows             part[2] = {{0, e->mb.rows_a, 0, sa, e->d_cu_q, e->d_k_len},
                                      {e->mb.rows_a, M - e->mb.rows_a, sa, nseq - sa, e->d_cu_q_b, e->d_k_len + sa}};
    hipEvent_t             done[2] = {nullptr, nullptr};
    for (int li = 0; li < m.layers; ++li) {
        Layer& L = e->layers[li];
        TM_REQUIRE(!L.is_moe, "internal: micro-batch schedule on a MoE layer");
        for (int h = 0; h < 2; ++h) {
            const Rows&       P  = part[h];
            const KvCacheView cv = cache_view(e, li, P.s0);
            if (li > 0) {  // this micro-batch's w2 partial sums of the previous layer
                TM_TRY(pipe_close(e, P, done[h], nullptr, L.attn_norm));
            }
            TM_TRY(qkv_project(e, L, P, false, false, 0, nullptr));
            TM_PROF(P_KV_STORE, TM_TRY(kv_store(e, L, cv, P, e->stream, rope_row0)));
            TM_TRY(prefill_attention_block(e, L, cv, P, max_q_len, max_k_len, kflat_stride, scale_log2));
            TM_TRY(pipe_wo(e, L, P, &done[h]));
        }
        for (int h = 0; h < 2; ++h) {
            TM_TRY(pipe_ffn(e, L, part[h], &done[h]));
        }
    }
    for (int h = 0; h < 2; ++h) {
        TM_TRY(pipe_close(e, part[h], done[h], nullptr, e->final_norm));
    }
    return 0;
}

// tm_engine_score: every row's final-normed hidden state through the lm_head, then its NLL against the next token (the
// reference's ComputeAndOutputLogits + ComputeCeLoss, output_processor.cc:236-300); no arg-max, sampling or processors
static int score_rows(tm_engine* e, int M)
{
    for (int r0 = 0; r0 < M; r0 += e->score_rows) {
        const int n = std::min(e->score_rows, M - r0);
        TM_PROF(P_LM_HEAD, TM_TRY(linear_plain(e, e->output, e->d_x + (size_t)r0 * e->hidden, e->hidden, e->d_score_logits, e->score_ld,
                                               n, false)));
        TM_PROF(P_SAMPLE, TM_TRY(launch_cross_entropy(e->d_score_nll + e->score_base + r0, e->d_score_logits,
                                                      e->d_score_tgt + e->score_base + r0, n, e->vocab_local, e->score_ld, e->stream)));
    }
    return 0;
}

// tp > 1 sampling: the vocabulary shards of `n` logits rows are all-gathered into full rows, d_logits_full (the reference gathers the
// logits too, models/language_model.cc:304-333); EVERY rank then draws from the same distribution with the same Philox number -> the
// same token everywhere, no further exchange
static int gather_logits_tp(tm_engine* e, const half_t* logits, int n)
{
    hipStream_t  st  = e->stream;
    const size_t cnt = (size_t)n * e->vocab_local;
    if (!e->comm) {
        // native communicator alone: the shards travel through the P2P segments, as many whole rows per exchange as
        // one segment buffer holds; rank q's rows land in its [n][vocab / tp] plane of d_logits_gather
        half_t*   data[8];
        uint32_t* flags[8];
        p2p_tables(e, data, flags);
        const size_t tile = (size_t)e->p2p_rows * e->hidden;  // fp16 elements of one segment buffer
        const int    per  = (int)std::min<size_t>(n, tile / e->vocab_local);
        TM_REQUIRE(per >= 1, "native communicator: one logits row does not fit a segment buffer (export more rows)");
        for (int r0 = 0; r0 < n; r0 += per) {
            const int rows = std::min(per, n - r0);
            TM_TRY(launch_p2p_allgather(data, flags, e->cfg.tp, e->cfg.rank, e->p2p_state, tile, logits + (size_t)r0 * e->vocab_local,
                                        e->d_logits_gather + (size_t)r0 * e->vocab_local, rows * e->vocab_local / 2, st,
                                        cnt / 2));
        }
    }
    else {
        TM_NCCL_CHECK(ncclAllGather(logits, e->d_logits_gather, cnt, ncclHalf, e->comm, st));
    }
    gather_vocab_kernel<<<std::min<size_t>(1024, (cnt * e->cfg.tp / 8 + 255) / 256), 256, 0, st>>>(
        e->d_logits_full, e->d_logits_gather, n, e->vocab_local, e->cfg.tp);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// tp > 1 greedy: every rank's (best value, global index) per row is exchanged, the best of them picked -> ids
static int argmax_tp(tm_engine* e, int* ids, const half_t* logits, int n)
{
    hipStream_t st = e->stream;
    TM_TRY(launch_argmax(ids, e->d_argmax_val, logits, n, e->vocab_local, e->vocab_local, e->cfg.rank * e->vocab_local, st));
    pack_candidates_kernel<<<(n + 63) / 64, 64, 0, st>>>(e->d_cand, ids, e->d_argmax_val, n);
    TM_HIP_CHECK(hipGetLastError());
    if (e->p2p_ready) {
        half_t*   data[8];
        uint32_t* flags[8];
        p2p_tables(e, data, flags);
        TM_TRY(launch_p2p_allgather(data, flags, e->cfg.tp, e->cfg.rank, e->p2p_state, (size_t)e->p2p_rows * e->hidden, e->d_cand,
                                    e->d_cand_all, n * 2, st));
    }
    else {
        TM_NCCL_CHECK(ncclAllGather(e->d_cand, e->d_cand_all, (size_t)n * 2, ncclFloat, e->comm, st));
    }
    pick_kernel<<<(n + 63) / 64, 64, 0, st>>>(ids, e->d_cand_all, e->cfg.tp, n);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// last-token hidden states -> logits -> next ids, for `n` sequences whose logits / next ids land in the batch slots
// [slot, slot + n): hx = their hidden rows, ids_in / cu_q (nullptr: one token per sequence) / ntok = the tokens this forward
// consumed for them, k_len = their context lengths
static int head(tm_engine* e, const half_t* hx, int n, int slot, const int* ids_in, const int* cu_q, int ntok, const int* k_len,
                const int* active = nullptr)
{
    hipStream_t st     = e->stream;
    half_t*     logits = e->d_logits + (size_t)slot * e->vocab_local;
    int*        ids    = e->d_next_ids + slot;
    TM_PROF(P_LM_HEAD, TM_TRY(linear_plain(e, e->output, hx, e->hidden, logits, e->vocab_local, n, false)));
    if (e->logits_on) {
        // the tokens this forward consumed join the slots' seen masks, then penalty / bans on the (local) logits
        uint32_t* seen = e->d_seen + (size_t)slot * e->seen_words;
        TM_PROF(P_SAMPLE, TM_TRY(launch_seen_update(seen, e->seen_words, ids_in, cu_q, n, ntok, e->cfg.model.vocab, st, active)));
        TM_PROF(P_SAMPLE, TM_TRY(launch_logits_process(logits, n, e->vocab_local, e->vocab_local,
                                                       e->vocab_local < e->cfg.model.vocab ? e->cfg.rank * e->vocab_local : 0, seen,
                                                       e->seen_words, e->d_lp_rep + slot, e->d_lp_ban + slot * kMaxBadIds,
                                                       e->d_lp_end + slot * kMaxEndIds, k_len, e->d_lp_minlen + slot, st)));
    }
    if (e->sampling_on && (!e->use_comm || ((e->comm || e->p2p_ready) && e->d_logits_full))) {
        // parameters are indexed by batch slot, the counter (context length) by the row of this forward
        const half_t* lg = logits;
        int           V  = e->vocab_local;
        if (e->use_comm) {
            TM_TRY(gather_logits_tp(e, logits, n));
            V  = e->vocab_local * e->cfg.tp;
            lg = e->d_logits_full;
        }
        TM_PROF(P_SAMPLE, TM_TRY(launch_sample_uniform(e->d_u + slot, e->d_seed + slot, k_len, n, st)));
        // static batch with tm_engine_set_logprobs: the kept candidates' logprobs of this step join the record of (slot, step)
        // continuous batching with tm_engine_request_logprobs: the record of (slot, this step), handed to the host behind the step
        const bool           lpr_cb = e->sched && e->cb_logprobs_on;
        const bool           lpr    = (e->logprobs_on && !e->sched) || lpr_cb;
        const SampleLogprobs lp = lpr_cb ? SampleLogprobs{e->d_cb_lp_vals, e->d_cb_lp_idx, e->d_cb_lp_num, e->d_cb_lp_sel, kMaxLogProb, nullptr, 0, 1, slot, 1}
                                         : SampleLogprobs{e->d_lpr_vals, e->d_lpr_idx, e->d_lpr_num, e->d_lpr_sel, e->logprobs_n, e->d_step, 1, e->max_new,
                                                          slot, e->max_new};
        TM_PROF(P_SAMPLE, TM_TRY(launch_sample(ids, lpr ? e->d_kept + slot : nullptr, lg, n, V, V, e->d_temp + slot, e->d_topk + slot,
                                               e->d_topp + slot, e->d_minp + slot, e->d_u + slot, e->d_sample_ws, st, lpr ? &lp : nullptr)));
    }
    else if (!e->use_comm) {
        TM_PROF(P_SAMPLE, TM_TRY(launch_argmax(ids, nullptr, logits, n, e->vocab_local, e->vocab_local, 0, st)));
    }
    else {
        TM_TRY(argmax_tp(e, ids, logits, n));
    }
    return 0;
}

// One forward over M tokens.  decode: one token per sequence (cu_q = 0..B); prefill: nseq sequences.
// Mixed forward (continuous batching, the reference's unified batch: unified_attention_layer.cc:310-311 puts the decode rows
// first): `md` != nullptr and !decode -> rows [0, md->rows) are the decode tokens of batch slots 0 .. md->rows-1 (their KV
// through the fused decode attention on the engine's own, UNSHIFTED block table and md->k_len), rows [md->rows, M) are the
// prefill tokens of `nseq` sequences described by e->d_cu_q / d_k_len / d_rows (d_rows already counts from row 0 of the
// forward).  Every linear, norm and (MoE) FFN runs ONCE over all M rows -- one weight stream serves both.
int forward(tm_engine* e, const int* d_ids, int M, int nseq, bool decode, int max_q_len, int max_k_len,
                   int kflat_stride, int slot0, const MixedDecode* md)
{
    const tm_model_config& m = e->cfg.model;
    hipStream_t            st = e->stream;
    const int              nd = md ? md->rows : 0;  // leading decode rows of a mixed forward
    TM_REQUIRE(!md || (!decode && nd > 0 && nd < M), "internal: mixed forward");
    // per-sequence RoPE tables: the row offsets are indexed by batch slot, this forward's sequence 0 sits in slot0
    const int* const rope_row0 = e->d_rope_row0 ? e->d_rope_row0 + slot0 : nullptr;
    TM_REQUIRE(!rope_row0 || !e->fuse_qkv, "internal: fused decode prologue with per-sequence RoPE tables");
    const float scale_log2 = (1.0f / std::sqrt((float)e->D)) * 1.4426950408889634f;
    const Rows  own{nd, M - nd, 0, nseq, e->d_cu_q, e->d_k_len};  // the forward's own sequences: every row unless it is mixed
    const Rows  dec{0, nd, 0, nd, md ? md->cu_q : nullptr, md ? md->k_len : nullptr};  // mixed: decode rows = batch slots 0 .. nd-1
    // a static decode step of a model with M-RoPE sections: the slots' position deltas (zeros for text) shift the new token's RoPE row
    e->fw_pos_delta = decode && !e->sched && e->d_pos_delta ? e->d_pos_delta + slot0 : nullptr;
    TM_REQUIRE(!(e->fw_emb_index || e->fw_mrope_pos) || (!decode && !md && !e->scoring && !e->use_comm), "internal: multimodal forward");
    if (e->fw_emb_index) {  // a multimodal prefill forward: rows inside an embedding range come from the request's buffer
        TM_PROF(P_EMBED, TM_TRY(launch_embedding_mixed(e->d_resid, e->tok_embeddings, d_ids, e->d_emb_rows, e->fw_emb_index, M, e->hidden,
                                                       m.vocab, st)));
    }
    else {
        TM_PROF(P_EMBED, TM_TRY(launch_embedding(e->d_resid, e->tok_embeddings, d_ids, M, e->hidden, m.vocab, st)));
    }
    TM_PROF(P_RES_NORM, TM_TRY(launch_rmsnorm(e->d_x, e->d_resid, e->layers[0].attn_norm, m.rms_eps, M, e->hidden, st, e->hidden_valid)));
    // tp > 1 prefill through RCCL: whole dense layers as two micro-batches, or their row-wise part as two row halves (side-stream all-reduces)
    e->pipe_events_used = 0;
    const bool  pipe     = !decode && !md && prefill_pipe_ok(e, M);
    const int   Ma       = pipe ? (M / 2 + 63) / 64 * 64 : 0;
    e->pipe_forwards += pipe ? 1 : 0;
    bool two_mb = pipe && e->mb.seqs_a > 0 && e->mb.seqs_a < nseq && e->mb.rows_a > 0 && e->mb.rows_a < M;
    for (int li = 0; two_mb && li < m.layers; ++li) {
        two_mb = !e->layers[li].is_moe;
    }
    if (two_mb) {
        e->pipe_mb_forwards += 1;
        TM_TRY(forward_layers_two_microbatches(e, M, nseq, max_q_len, max_k_len, kflat_stride, scale_log2, rope_row0));
    }
    const bool aux      = md && e->mixed_two_streams && e->aux_stream;  // mixed: the decode rows' attention beside the prefill rows'
    const bool fuse_qkv = decode && e->fuse_qkv;
    bool       qkv_done = false;  // the previous layer's two-halves tail already projected this layer's QKV
    int        ss_tiles = 0;  // > 0: d_x holds r . g of a folded producer, d_ss its sums of squares (the next GEMM applies the row factor)
    for (int li = 0; li < (two_mb ? 0 : m.layers); ++li) {
        Layer&            L    = e->layers[li];
        Layer* const      nxt  = li + 1 < m.layers ? &e->layers[li + 1] : nullptr;
        const half_t*     next_norm = nxt ? nxt->attn_norm : e->final_norm;
        const KvCacheView cv   = cache_view(e, li);
        const bool        fold = decode && fold_ok(e, L, M);
        TM_REQUIRE(ss_tiles == 0 || fold, "internal: folded norm without a folded consumer");
        int qkv_slabs = 1;
        if (!qkv_done) {
            TM_TRY(qkv_project(e, L, Rows{0, M}, fold, fuse_qkv, ss_tiles, &qkv_slabs));
        }
        ss_tiles = 0;
        qkv_done = false;
        if (decode) {
            TM_TRY(decode_attention_block(e, L, cv, own, fuse_qkv ? qkv_slabs : 0, scale_log2, st, rope_row0));
        }
        else {
            TM_PROF(P_KV_STORE, TM_TRY(kv_store(e, L, cv, own, st, rope_row0)));
            if (md) {
                // decode rows: (fused prologue: RoPE + K/V quantise-store) + attention on the fp16 projection rows; they share
                // nothing with the prefill rows' path below, so they run beside it on the aux stream (fork here, join behind the
                // prefill attention) -- the reference's decode / prefill split of a unified batch
                if (aux) {
                    TM_HIP_CHECK(hipEventRecord(e->ev_aux_fork, st));
                    TM_HIP_CHECK(hipStreamWaitEvent(e->aux_stream, e->ev_aux_fork, 0));
                }
                KvCacheView cvd = cv;
                cvd.block_ptrs  = md->block_ptrs;
                TM_TRY(decode_attention_block(e, L, cvd, dec, e->fuse_qkv ? 1 : 0, scale_log2, aux ? e->aux_stream : st, e->d_rope_row0));
                if (aux) {
                    TM_HIP_CHECK(hipEventRecord(e->ev_aux_join, e->aux_stream));
                }
            }
            if (e->fw_verify && e->spec_mfma) {
                TM_TRY(verify_attention_block(e, cv, own, max_q_len, scale_log2));
            }
            else {
                TM_TRY(prefill_attention_block(e, L, cv, own, max_q_len, max_k_len, kflat_stride, scale_log2));
            }
            if (aux) {
                TM_HIP_CHECK(hipStreamWaitEvent(st, e->ev_aux_join, 0));  // join: wo reads the decode rows' attention output too
            }
        }
        if (pipe && !L.is_moe) {
            TM_TRY(forward_tail_two_halves(e, L, M, Ma, next_norm, nxt));
            qkv_done = nxt != nullptr;
        }
        else if (fold) {
            TM_TRY(tail_folded(e, L, M, next_norm, nxt && fold_ok(e, *nxt, M), &ss_tiles));
        }
        else if (L.is_moe) {
            TM_TRY(tail_moe(e, L, M, next_norm));
        }
        else {
            TM_TRY(tail_dense(e, L, M, next_norm));
        }
    }
    if (e->scoring) {
        TM_REQUIRE(!decode && !md && !e->use_comm, "internal: scoring forward");
        return score_rows(e, M);
    }
    if (e->fw_verify) {  // speculative decoding: the greedy token behind EVERY row
        TM_REQUIRE(!decode && !md && !e->use_comm, "internal: verify forward");
        TM_PROF(P_LM_HEAD, TM_TRY(linear_plain(e, e->output, e->d_x, e->hidden, e->d_spec_logits, e->vocab_local, M, false)));
        TM_PROF(P_SAMPLE, TM_TRY(launch_argmax(e->d_spec_out, nullptr, e->d_spec_logits, M, e->vocab_local, e->vocab_local, 0, st)));
        return 0;
    }
    if (decode) {
        return head(e, e->d_x, nseq, slot0, d_ids, nullptr, M, e->d_k_len);
    }
    if (md) {  // the decode rows first: their slots are 0 .. nd-1; the prefilled slots' entries are overwritten right after
        TM_TRY(head(e, e->d_x, nd, 0, d_ids, nullptr, nd, md->k_len, md->active));
    }
    TM_TRY(launch_gather_rows(e->d_last, e->d_x, e->d_rows, nseq, e->hidden, st));
    return head(e, e->d_last, nseq, slot0, d_ids + nd, e->d_cu_q, M - nd, e->d_k_len);
}

// next ids become the current ids and are appended to generated[b][step]
static int commit_tokens(tm_engine* e)
{
    TM_HIP_CHECK(hipMemcpyAsync(e->d_ids, e->d_next_ids, (size_t)e->batch * 4, hipMemcpyDeviceToDevice, e->stream));
    record_kernel<<<1, std::max(64, ((e->batch + 63) / 64) * 64), 0, e->stream>>>(e->d_ids, e->d_generated, e->d_step,
                                                                                  e->batch, e->max_new);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

static int decode_step(tm_engine* e)
{
    advance_kernel<<<(e->batch + 63) / 64, 64, 0, e->stream>>>(e->d_k_len, e->batch);
    TM_HIP_CHECK(hipGetLastError());
    TM_TRY(forward(e, e->d_ids, e->batch, e->batch, true, 1, 0, 0, 0));
    return commit_tokens(e);
}

// ---- speculative decoding by prompt lookup (speculative.hip) -----------------------------------------------------------
// The batch state the device-side proposer / acceptance work on: the decode arrays (d_k_len = tokens in the cache, d_ids = the last
// emitted token = row 0 of the next forward, d_generated [batch][max_new]) + the token history and per-sequence counters.
static SpecState spec_state(const tm_engine* e)
{
    SpecState s{};
    s.hist        = e->d_spec_hist;
    s.hist_stride = e->cfg.session_len;
    s.hist_len    = e->d_spec_len;
    s.emitted     = e->d_spec_emitted;
    s.generated   = e->d_generated;
    s.max_new     = e->max_new;
    s.k_len       = e->d_k_len;
    s.next_id     = e->d_ids;
    s.totals      = e->d_spec_totals;
    return s;
}

// The flatten + prefill-attention path of the verify forward (fp16 KV, head_dim 64) needs what no kernel can tell the host: the longest
// context and the sequences' offsets in the flat scratch.  Reads d_k_len back (a synchronisation per step: this path is never captured).
static int spec_host_lengths(tm_engine* e, int* max_k_len)
{
    std::vector<int> kl(e->batch), koff(e->batch + 1, 0);
    TM_HIP_CHECK(hipMemcpyAsync(kl.data(), e->d_k_len, (size_t)e->batch * 4, hipMemcpyDeviceToHost, e->stream));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    *max_k_len = 0;
    for (int b = 0; b < e->batch; ++b) {
        const int n = kl[b] + e->spec_k + 1;
        *max_k_len  = std::max(*max_k_len, n);
        koff[b + 1] = koff[b] + (n + 63) / 64 * 64;
    }
    TM_REQUIRE(koff.back() <= e->kflat_stride,
               "speculative decoding on the flatten + prefill-attention path (fp16 KV / head_dim 64): the batch's contexts do not fit the "
               "flatten scratch -- lower the batch or the context, or use int8 / int4 KV at head_dim 128");
    TM_HIP_CHECK(hipMemcpyAsync(e->d_cu_koff, koff.data(), koff.size() * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));  // koff is pageable
    return 0;
}

// rows (last token + drafts) -> verify forward over batch * (k + 1) rows -> acceptance.  The forward is the prefill-shaped one over the
// step's own per-sequence arrays (cu_q = (k + 1) b, k_len = tokens in the cache + k + 1): plain w_qkv, K/V store, attention, lm_head
// over every row, arg-max -- no fused prologue, no folded norm.
static int spec_verify_accept(tm_engine* e)
{
    const SpecState s  = spec_state(e);
    const int       k1 = e->spec_k + 1;
    int             max_k_len = 0;
    if (!e->spec_mfma) {
        TM_TRY(spec_host_lengths(e, &max_k_len));
    }
    TM_TRY(launch_spec_rows(e->d_spec_ids, e->d_spec_k_len, e->d_spec_drafts, s, e->batch, e->spec_k, e->stream));
    int* const cu_q  = e->d_cu_q;
    int* const k_len = e->d_k_len;
    e->d_cu_q        = e->d_spec_cu_q;
    e->d_k_len       = e->d_spec_k_len;
    e->fw_verify     = true;
    const int rc     = forward(e, e->d_spec_ids, e->batch * k1, e->batch, false, k1, max_k_len, e->kflat_stride, 0);
    e->fw_verify     = false;
    e->d_cu_q        = cu_q;
    e->d_k_len       = k_len;
    TM_TRY(rc);
    return launch_spec_accept(e->d_spec_out, e->d_spec_drafts, e->d_spec_ndraft, s, e->batch, e->spec_k, e->d_spec_step, e->stream);
}

static int spec_step(tm_engine* e)
{
    TM_TRY(launch_spec_propose(e->d_spec_drafts, e->d_spec_ndraft, spec_state(e), e->batch, e->spec_k, e->spec_ngram_max, e->spec_ngram_min,
                               e->stream));
    return spec_verify_accept(e);
}

}  // namespace tmk

extern "C" {

// sampling state: device arrays for all slots (allocated on first use), upload of `n` slots starting at slot0
int sampling_upload(tm_engine* e, const tm_sampling* p, int slot0, int n)
{
    const int B = e->cfg.max_batch_size;
    if (!e->d_temp) {
        TM_REQUIRE(e->vocab_local % 8 == 0, "sampling needs vocab % 8 == 0");
        TM_TRY(dmalloc(&e->d_temp, (size_t)B));
        TM_TRY(dmalloc(&e->d_topp, (size_t)B));
        TM_TRY(dmalloc(&e->d_minp, (size_t)B));
        TM_TRY(dmalloc(&e->d_u, (size_t)B));
        TM_TRY(dmalloc(&e->d_topk, (size_t)B));
        TM_TRY(dmalloc(&e->d_seed, (size_t)B));
        TM_HIP_CHECK(hipMalloc(&e->d_sample_ws, sample_workspace_bytes(B)));
        TM_HIP_CHECK(hipMemsetAsync(e->d_sample_ws, 0, sample_workspace_bytes(B), e->stream));
        if (e->use_comm) {
            TM_TRY(dmalloc(&e->d_logits_gather, (size_t)B * e->vocab_local * e->cfg.tp));
            TM_TRY(dmalloc(&e->d_logits_full, (size_t)B * e->vocab_local * e->cfg.tp));
        }
        std::vector<float>    one(B, 1.f), zero(B, 0.f);
        std::vector<int>      k1(B, 1);
        std::vector<uint64_t> s0(B, 0);
        TM_HIP_CHECK(hipMemcpyAsync(e->d_temp, one.data(), B * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_topp, one.data(), B * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_minp, zero.data(), B * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_topk, k1.data(), B * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_seed, s0.data(), B * 8, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    std::vector<float>    t(n), pp(n), mp(n);
    std::vector<int>      k(n);
    std::vector<uint64_t> sd(n);
    for (int i = 0; i < n; ++i) {
        TM_REQUIRE(p[i].temperature > 0.f, "sampling: temperature must be > 0");
        t[i]  = p[i].temperature;
        k[i]  = p[i].top_k;
        pp[i] = p[i].top_p;
        mp[i] = p[i].min_p;
        sd[i] = p[i].seed;
    }
    TM_HIP_CHECK(hipMemcpyAsync(e->d_temp + slot0, t.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_topk + slot0, k.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_topp + slot0, pp.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_minp + slot0, mp.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_seed + slot0, sd.data(), n * 8, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    return 0;
}

// logits-processor state of `n` slots starting at slot0: parameters + cleared seen masks.  eos[i] (may be < 0) joins the
// stop ids as an end id; prompt_len[i] turns min_new_tokens into the context-length threshold of the kernel.
extern const tm_logits_param kNoLogitsParam = {1.f, 0, 0, {0}, 0, {0}};

int logits_param_check(const tm_logits_param& p)
{
    TM_REQUIRE(p.repetition_penalty > 0.f, "repetition_penalty must be > 0");
    TM_REQUIRE(p.min_new_tokens >= 0, "min_new_tokens must be >= 0");
    TM_REQUIRE(p.n_bad_ids >= 0 && p.n_bad_ids <= TM_MAX_BAD_IDS, "0 <= n_bad_ids <= TM_MAX_BAD_IDS");
    TM_REQUIRE(p.n_stop_ids >= 0 && p.n_stop_ids <= TM_MAX_STOP_IDS, "0 <= n_stop_ids <= TM_MAX_STOP_IDS");
    return 0;
}

int logits_upload(tm_engine* e, const tm_logits_param* p, const int* prompt_len, const int* eos, int slot0, int n)
{
    const int B = e->cfg.max_batch_size;
    if (!e->d_seen) {
        TM_REQUIRE(e->vocab_local % 8 == 0, "logits processors need (local) vocab % 8 == 0");
        e->seen_words = (e->cfg.model.vocab + 31) / 32;
        TM_TRY(dmalloc(&e->d_seen, (size_t)B * e->seen_words));
        TM_TRY(dmalloc(&e->d_lp_rep, (size_t)B));
        TM_TRY(dmalloc(&e->d_lp_minlen, (size_t)B));
        TM_TRY(dmalloc(&e->d_lp_ban, (size_t)B * kMaxBadIds));
        TM_TRY(dmalloc(&e->d_lp_end, (size_t)B * kMaxEndIds));
        std::vector<float> one(B, 1.f);
        TM_HIP_CHECK(hipMemcpyAsync(e->d_lp_rep, one.data(), B * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemsetAsync(e->d_lp_minlen, 0, (size_t)B * 4, e->stream));
        TM_HIP_CHECK(hipMemsetAsync(e->d_lp_ban, 0xff, (size_t)B * kMaxBadIds * 4, e->stream));
        TM_HIP_CHECK(hipMemsetAsync(e->d_lp_end, 0xff, (size_t)B * kMaxEndIds * 4, e->stream));
        TM_HIP_CHECK(hipMemsetAsync(e->d_seen, 0, (size_t)B * e->seen_words * 4, e->stream));
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    std::vector<float> r(n);
    std::vector<int>   ml(n), ban((size_t)n * kMaxBadIds, -1), end((size_t)n * kMaxEndIds, -1);
    for (int i = 0; i < n; ++i) {
        TM_TRY(logits_param_check(p[i]));
        r[i]  = p[i].repetition_penalty;
        ml[i] = p[i].min_new_tokens > 0 ? prompt_len[i] + p[i].min_new_tokens : 0;
        for (int k = 0; k < p[i].n_bad_ids; ++k) {
            ban[(size_t)i * kMaxBadIds + k] = p[i].bad_ids[k];
        }
        end[(size_t)i * kMaxEndIds] = eos ? eos[i] : -1;
        for (int k = 0; k < p[i].n_stop_ids; ++k) {
            end[(size_t)i * kMaxEndIds + 1 + k] = p[i].stop_ids[k];
        }
    }
    TM_HIP_CHECK(hipMemcpyAsync(e->d_lp_rep + slot0, r.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_lp_minlen + slot0, ml.data(), n * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_lp_ban + (size_t)slot0 * kMaxBadIds, ban.data(), ban.size() * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_lp_end + (size_t)slot0 * kMaxEndIds, end.data(), end.size() * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemsetAsync(e->d_seen + (size_t)slot0 * e->seen_words, 0, (size_t)n * e->seen_words * 4, e->stream));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    return 0;
}

// decode split heuristic: fill >= 2 workgroups per CU (GetSplitCount, kernels/attention/utils.cc:11-46); fused prologue
void setup_decode(tm_engine* e, int batch)
{
    const tm_engine_config& c = e->cfg;
    int splits = c.decode_splits;
    if (splits <= 0) {
        // int8 / int4 KV run the MFMA kernel: up to 16 query heads of a kv head per workgroup (launch_decode_attention_i8_mfma),
        // four waves = four cache blocks in flight per workgroup -- one workgroup per CU is enough: measured at one rank's head
        // count of TP = 8 (profiles/r04_gemm_experiments_session2.txt, call25): 64 x 4 workgroups 1.485 ms per step against
        // 1.547 .. 1.587 with 64 x 8 (Llama-3-8B shard), 5.06 against 5.26 (Llama-3-70B shard).  fp16 KV (VALU kernel, <= 4
        // heads per workgroup): two workgroups per CU as before.
        // head_dim 64 decodes on the VALU kernel for every KV width: its head-per-workgroup rule
        // quant_policy 42 (TurboQuant KV): a VALU kernel of the same workgroup shape (attention_decode_tq.hip), never the fused prologue
        const bool mfma = (e->cfg.quant_policy == 8 || e->cfg.quant_policy == 4) && e->D == 128 && !e->windowed;
        const int  group = e->q_heads / e->kv_heads;
        int        hpw   = 1;
        if (mfma) {
            hpw = group;
            while (hpw > 16) {
                int d = 2;
                while (hpw % d) {
                    ++d;
                }
                hpw /= d;
            }
        }
        else {
            for (int cand = 4; cand >= 1; --cand) {
                if (group % cand == 0) {
                    hpw = cand;
                    break;
                }
            }
        }
        const int wgs = e->kv_heads * (group / hpw) * batch;
        splits        = 1;
        // (the 256-workgroup target is what was measured: full decode batches; small batches -- typically long contexts per sequence --
        // keep the deeper split)
        while (wgs * splits < (mfma && batch >= 32 ? 256 : 512) && splits < 16) {
            splits *= 2;
        }
    }
    e->decode_splits = std::min(std::max(splits, 1), 16);
    const char* valu = getenv("TM_ATTN_VALU");
    const char* fuse = getenv("TM_FUSE_QKV");
    // per-sequence RoPE tables (dynamic NTK active): the fused prologue reads the one shared table, so such an engine runs the unfused
    // decode path -- kv_rope_store with the row offsets, then plain decode attention
    // head_dim 64: no MFMA kernel, so no fused prologue either -- the same unfused path
    // a sliding window or attention sinks (e->windowed): the VALU kernel's variant serves them, the same unfused path for every layer
    // u4 weights in groups of 32 (gemm_u4_g32.hip): the linear always finishes its own fp16 rows, no slab reaches the attention kernel -- such
    // a model runs kv_rope_store, then plain decode attention, the same unfused path
    const bool g32   = e->cfg.model.weight_type == TM_WEIGHT_U4 && e->cfg.model.group_size == 32;
    e->fuse_qkv      = (e->cfg.quant_policy == 8 || e->cfg.quant_policy == 4) && !(valu && atoi(valu)) && !(fuse && !atoi(fuse))
                  && !e->d_rope_row0 && e->D == 128 && !e->windowed && !g32;
}

// Chunked prefill of `batch` sequences into the batch slots [slot0, slot0 + batch): whole sequences,
// <= max_prefill_token_num tokens per iteration (a sequence longer than the budget is split into history + new tokens).
// Logits / first tokens land in d_logits / d_next_ids at slot0 + i.  Uses e->d_k_len / d_cu_q as iteration-local arrays.
// `mix` (continuous batching): the LAST iteration also carries the decode step of all batch slots as leading rows of the
// same forward (MixedDecode); every iteration then leaves room for those rows.  *mix->done reports that it happened.
int prefill_slots(tm_engine* e, const int* const* seq_ids, const int* host_lens, int batch, int slot0, float* ttft_ms,
                         const MixedStep* mix)
{
    // The decode rows ride on the LAST iteration of the admission (any number of iterations, chunked prompts included -- the
    // reference mixes unconditionally, unified_attention_layer.cc:310-311).  The decode head of that iteration writes the
    // next-id entry of every batch slot, so the first tokens that EARLIER iterations left in d_next_ids are moved to
    // d_first_ids right after each iteration and handed back when the admission is done.
    const int  budget  = e->max_tokens - (mix ? mix->rows : 0);
    const auto t_start = std::chrono::steady_clock::now();
    // Because the batch tables (block_ptrs, cu_block_nums) are indexed by the batch slot, every prefill
    // iteration covers a contiguous range of slots [b0, b1]; the block table is offset accordingly and the
    // logits / first tokens of the iteration land in d_logits / d_next_ids at slot b0 + i.
    int b0 = 0;
    int done_in_b0 = 0;  // tokens of sequence b0 already prefilled (chunked long prompt)
    int consumed   = 0;  // tokens of the concatenated sequences prefilled by earlier iterations (the scoring rows' positions)
    while (b0 < batch) {
        std::vector<int> cu_q{0}, klen, koff{0}, rows, ids;
        std::vector<int> emb_index, coords;  // multimodal batch: per row, next to ids (a chunked sequence continues at `start`)
        const bool       mm = !e->mm_coords.empty() && !mix && !e->scoring;
        int b1 = b0, tokens = 0, max_q = 0, max_k = 0;
        bool partial_last = false;
        while (b1 < batch) {
            const int start  = (b1 == b0) ? done_in_b0 : 0;
            const int remain = host_lens[b1] - start;
            const int take   = std::min(remain, budget - tokens);
            if (take <= 0) {
                break;
            }
            ids.insert(ids.end(), seq_ids[b1] + start, seq_ids[b1] + start + take);
            if (mm) {
                const std::vector<int>& ei = e->mm_emb_index[b1];
                const std::vector<int>& co = e->mm_coords[b1];
                emb_index.insert(emb_index.end(), ei.begin() + start, ei.begin() + start + take);
                coords.insert(coords.end(), co.begin() + (size_t)start * 3, co.begin() + (size_t)(start + take) * 3);
            }
            tokens += take;
            cu_q.push_back(tokens);
            klen.push_back(start + take);
            koff.push_back(koff.back() + ((start + take + 63) / 64) * 64);
            rows.push_back(tokens - 1);
            max_q = std::max(max_q, take);
            max_k = std::max(max_k, start + take);
            if (take < remain) {  // budget exhausted inside this sequence: it continues in the next iteration
                done_in_b0   = start + take;
                partial_last = true;
                break;
            }
            ++b1;
        }
        const int nseq = (int)klen.size();
        TM_REQUIRE(nseq >= 1, "internal: empty prefill iteration");
        TM_REQUIRE(koff.back() <= e->kflat_stride, "internal: flatten scratch too small");
        // the last iteration of a continuous-batching admission: decode rows of every slot in front of the prefill rows
        const bool merge = mix && b1 == batch && !partial_last;
        const int  nd    = merge ? mix->rows : 0;
        if (merge) {
            TM_TRY(launch_advance_active(mix->k_len, mix->active, nd, e->stream));
            TM_HIP_CHECK(hipMemcpyAsync(e->d_prefill_ids, mix->ids, (size_t)nd * 4, hipMemcpyDeviceToDevice, e->stream));
            for (int& r : rows) {
                r += nd;
            }
        }
        TM_HIP_CHECK(hipMemcpyAsync(e->d_prefill_ids + nd, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_cu_q, cu_q.data(), cu_q.size() * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_k_len, klen.data(), klen.size() * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_cu_koff, koff.data(), koff.size() * 4, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, e->stream));
        if (mm) {
            // an iteration without a single embedding row keeps the plain lookup; coordinates reach the store only on a model with sections
            const bool any_emb = std::any_of(emb_index.begin(), emb_index.end(), [](int v) { return v >= 0; });
            if (any_emb) {
                TM_HIP_CHECK(hipMemcpyAsync(e->d_emb_index, emb_index.data(), emb_index.size() * 4, hipMemcpyHostToDevice, e->stream));
                e->fw_emb_index = e->d_emb_index;
            }
            if (e->d_pos_delta) {
                TM_HIP_CHECK(hipMemcpyAsync(e->d_mrope_pos, coords.data(), coords.size() * 4, hipMemcpyHostToDevice, e->stream));
                e->fw_mrope_pos = e->d_mrope_pos;
            }
        }
        // tensor-parallel forward through RCCL: the sequence boundary nearest to half the rows makes two micro-batches that leapfrog
        // through the layers (forward_layers_two_microbatches); none with both sides >= pipe_min_rows / 2 -> the row-half schedule
        e->mb = {};
        std::vector<int> cu_q_b;  // lives until the synchronisation at the end of this iteration, like the vectors above
        static const bool mb_on = !getenv("TM_PIPE_MICROBATCH") || atoi(getenv("TM_PIPE_MICROBATCH")) != 0;  // A/B switch: 0 = row halves only
        if (mb_on && !merge && nseq >= 2 && prefill_pipe_ok(e, tokens)) {
            const int best = prefill_microbatch_split(cu_q.data(), nseq, e->pipe_min_rows);  // scheduler.h
            if (best > 0) {
                cu_q_b.assign(cu_q.begin() + best, cu_q.end());
                for (int& v : cu_q_b) {
                    v -= cu_q[best];
                }
                TM_HIP_CHECK(hipMemcpyAsync(e->d_cu_q_b, cu_q_b.data(), cu_q_b.size() * 4, hipMemcpyHostToDevice, e->stream));
                e->mb.seqs_a = best;
                e->mb.rows_a = cu_q[best];
            }
        }
        // shift the block tables so that slot 0 of this iteration is sequence b0
        uint64_t* saved_ptrs = e->d_block_ptrs;
        e->d_block_ptrs += (size_t)(slot0 + b0) * e->max_blocks_per_seq;
        const MixedDecode md{nd, merge ? mix->k_len : nullptr, merge ? mix->block_ptrs : nullptr, merge ? mix->cu_q : nullptr,
                             merge ? mix->active : nullptr};
        e->score_base   = consumed;
        consumed       += tokens;
        const int rc    = forward(e, e->d_prefill_ids, nd + tokens, nseq, false, max_q, max_k, e->kflat_stride, slot0 + b0,
                                  merge ? &md : nullptr);
        e->d_block_ptrs = saved_ptrs;
        e->mb           = {};
        e->fw_emb_index = nullptr;
        e->fw_mrope_pos = nullptr;
        if (rc) {
            (void)hipStreamSynchronize(e->stream);  // the pageable vectors above must outlive every copy queued from them
            return rc;
        }
        if (mix) {
            const int n_done = b1 - b0;  // sequences b0 .. b1-1 got their first token in this iteration
            if (n_done > 0 && !merge) {
                TM_HIP_CHECK(hipMemcpyAsync(e->d_first_ids + slot0 + b0, e->d_next_ids + slot0 + b0, (size_t)n_done * 4,
                                            hipMemcpyDeviceToDevice, e->stream));
            }
        }
        if (merge) {  // as decode_step_cb: the next ids of every slot become its current token ...
            TM_HIP_CHECK(hipMemcpyAsync(mix->ids, e->d_next_ids, (size_t)nd * 4, hipMemcpyDeviceToDevice, e->stream));
            // ... and the first tokens of the admission's earlier iterations return to their d_next_ids entries (the caller
            // reads first tokens from there); the sequences of THIS iteration wrote theirs after the decode head
            if (b0 > 0) {
                TM_HIP_CHECK(hipMemcpyAsync(e->d_next_ids + slot0, e->d_first_ids + slot0, (size_t)b0 * 4, hipMemcpyDeviceToDevice,
                                            e->stream));
            }
            *mix->done = true;
        }
        // the host vectors above are pageable: make sure the async copies are done before they die
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        if (ttft_ms) {
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_start).count();
            for (int b = b0; b < b1; ++b) {
                ttft_ms[b] = ms;  // first token of sequence b exists once its last chunk has been processed
            }
        }
        b0 = b1;  // a partially prefilled sequence (b1) is revisited with done_in_b0 tokens of history
        if (!partial_last) {
            done_in_b0 = 0;
        }
    }
    return 0;
}

// multimodal state back to "text": nothing armed, nothing admitted, every slot's position delta 0
static int multimodal_reset(tm_engine* e)
{
    e->h_mm.clear();
    e->mm_emb_index.clear();
    e->mm_coords.clear();
    if (e->d_pos_delta) {
        TM_HIP_CHECK(hipMemsetAsync(e->d_pos_delta, 0, (size_t)e->cfg.max_batch_size * sizeof(int), e->stream));
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    return 0;
}

// tm_engine_prefill: the armed multimodal inputs (`mm`: tm_engine_prefill took them out of e->h_mm on entry, so a prefill that fails
// anywhere leaves nothing armed) become what prefill_slots slices per iteration -- per sequence
// the row of d_emb_rows behind every prompt position (-1: token table) and three coordinates per position (the given ones, then linear
// position + delta) -- the rows go to the device in one buffer, the deltas into the batch slots.  Without armed inputs: deltas 0.
static int multimodal_admit(tm_engine* e, const std::vector<tmk::MmSeqT>& mm, const int* host_lens, int batch)
{
    e->mm_emb_index.clear();
    e->mm_coords.clear();
    if (mm.empty()) {
        if (e->d_pos_delta) {
            TM_HIP_CHECK(hipMemsetAsync(e->d_pos_delta, 0, (size_t)e->cfg.max_batch_size * sizeof(int), e->stream));
        }
        return 0;
    }
    TM_REQUIRE((int)mm.size() == batch, "tm_engine_set_multimodal: batch size differs from the prefill's");
    const int           H = e->hidden;
    std::vector<half_t> rows;
    std::vector<int>    delta(batch, 0);
    e->mm_emb_index.resize(batch);
    e->mm_coords.resize(batch);
    for (int b = 0; b < batch; ++b) {
        const auto& s = mm[b];
        if (s.prompt_len != host_lens[b]) {
            e->mm_emb_index.clear();
            e->mm_coords.clear();
            TM_REQUIRE(false, "tm_engine_set_multimodal: prompt_len differs from the prefill's prompt length");
        }
        const int n = host_lens[b];
        auto&     ei = e->mm_emb_index[b];
        auto&     co = e->mm_coords[b];
        ei.assign(n, -1);
        int row = (int)(rows.size() / H);
        for (size_t r = 0; r < s.ranges.size() / 2; ++r) {
            for (int p = s.ranges[2 * r]; p < s.ranges[2 * r + 1]; ++p) {
                ei[p] = row++;
            }
        }
        rows.insert(rows.end(), s.rows.begin(), s.rows.end());
        co.resize((size_t)n * 3);
        std::copy(s.pos.begin(), s.pos.end(), co.begin());
        for (int p = s.n_pos; p < n; ++p) {
            co[3 * p] = co[3 * p + 1] = co[3 * p + 2] = p + s.delta;  // the store clamps to [0, max_pos - 1]
        }
        delta[b] = s.delta;
    }
    if (!e->d_emb_index) {
        TM_TRY(dmalloc(&e->d_emb_index, (size_t)e->max_tokens));
        TM_TRY(dmalloc(&e->d_mrope_pos, (size_t)e->max_tokens * 3));
    }
    if (rows.size() > e->emb_rows_cap) {
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        (void)hipFree(e->d_emb_rows);
        e->d_emb_rows   = nullptr;
        e->emb_rows_cap = 0;
        TM_TRY(dmalloc(&e->d_emb_rows, rows.size()));
        e->emb_rows_cap = rows.size();
    }
    if (!rows.empty()) {
        TM_HIP_CHECK(hipMemcpyAsync(e->d_emb_rows, rows.data(), rows.size() * sizeof(half_t), hipMemcpyHostToDevice, e->stream));
    }
    if (e->d_pos_delta) {
        TM_HIP_CHECK(hipMemsetAsync(e->d_pos_delta, 0, (size_t)e->cfg.max_batch_size * sizeof(int), e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_pos_delta, delta.data(), (size_t)batch * 4, hipMemcpyHostToDevice, e->stream));
    }
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));  // rows / delta are pageable locals
    return 0;
}

int tm_engine_set_multimodal(tm_engine* e, const tm_mm_input* host, int batch)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(e->batch == 0 && !e->sched, "set the multimodal inputs before tm_engine_prefill");
    e->h_mm.clear();
    if (!host) {
        return 0;
    }
    TM_REQUIRE(e->cfg.tp == 1 && !e->use_comm, "multimodal input with tp > 1 is not built");
    TM_REQUIRE(e->cfg.quant_policy != 42, "multimodal input with quant_policy 42 (TurboQuant KV) is not built");
    TM_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch_size, "1 <= batch <= max_batch_size");
    const bool sections = e->mrope_section[0] + e->mrope_section[1] + e->mrope_section[2] > 0;
    std::vector<tmk::MmSeqT> mm(batch);
    for (int b = 0; b < batch; ++b) {
        const tm_mm_input& in = host[b];
        TM_REQUIRE(in.prompt_len >= 1, "multimodal input: prompt_len >= 1");
        TM_REQUIRE(in.n_rows >= 0 && in.n_ranges >= 0 && in.n_pos >= 0, "multimodal input: negative count");
        TM_REQUIRE(in.n_rows == 0 || in.emb_rows, "multimodal input: n_rows > 0 without emb_rows");
        TM_REQUIRE(in.n_ranges == 0 || in.ranges, "multimodal input: n_ranges > 0 without ranges");
        TM_REQUIRE(in.n_pos == 0 || in.mrope_pos, "multimodal input: n_pos > 0 without mrope_pos");
        int prev_end = 0, total = 0;
        for (int r = 0; r < in.n_ranges; ++r) {
            const int b0 = in.ranges[2 * r], b1 = in.ranges[2 * r + 1];
            TM_REQUIRE(b0 >= 0 && b1 <= in.prompt_len, "multimodal input: embedding range outside the prompt");
            TM_REQUIRE(b0 < b1, "multimodal input: empty or reversed embedding range");
            TM_REQUIRE(b0 >= prev_end, "multimodal input: embedding ranges unsorted or overlapping");
            prev_end = b1;
            total += b1 - b0;
        }
        TM_REQUIRE(total == in.n_rows, "multimodal input: embedding ranges do not add up to the row count");
        TM_REQUIRE(in.n_pos <= in.prompt_len, "multimodal input: n_pos larger than the prompt length");
        for (int i = 0; i < in.n_pos * 3; ++i) {
            TM_REQUIRE(in.mrope_pos[i] >= 0, "multimodal input: negative M-RoPE coordinate");
        }
        TM_REQUIRE(in.position_delta >= -in.prompt_len, "multimodal input: position_delta < -prompt_len");
        TM_REQUIRE(sections || (in.n_pos == 0 && in.position_delta == 0),
                   "multimodal input: M-RoPE coordinates or a position delta on a model without mrope_section (tm_engine_set_mrope_section)");
        auto& s      = mm[b];
        s.prompt_len = in.prompt_len;
        s.n_pos      = in.n_pos;
        s.delta      = in.position_delta;
        s.rows.assign((const half_t*)in.emb_rows, (const half_t*)in.emb_rows + (size_t)in.n_rows * e->hidden);
        s.ranges.assign(in.ranges, in.ranges + (size_t)in.n_ranges * 2);
        s.pos.assign(in.mrope_pos, in.mrope_pos + (size_t)in.n_pos * 3);
    }
    e->h_mm.swap(mm);
    return 0;
}

int tm_engine_release(tm_engine* e)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e, "null pointer");
    if (e->stream) {
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    }
    e->pending.valid = false;  // a look-ahead decode step of the session that ends here: its tokens belong to nobody
    TM_TRY(rope_reset(e, 0, e->cfg.max_batch_size));
    TM_TRY(multimodal_reset(e));
    for (auto& blks : e->h_blocks) {
        for (int b : blks) {
            e->free_blocks.push_back(b);
        }
    }
    e->h_blocks.clear();
    e->h_len.clear();
    e->batch      = 0;
    e->spec_batch = false;
    e->steps_done = 0;
    e->steps_fetched = 0;
    e->h_sampling.clear();
    e->cb_sampling.clear();
    e->sampling_on = false;
    e->logprobs_next = 0;
    e->logprobs_on   = false;
    e->cb_logprobs_on = false;
    e->cb_lp_used     = 0;
    e->h_logits.clear();
    e->cb_logits.clear();
    e->logits_on = false;
    if (e->sched) {  // leave continuous-batching mode: every block goes back to the static free list
        e->sched.reset();
        e->free_blocks.resize(e->num_blocks);
        for (int64_t i = 0; i < e->num_blocks; ++i) {
            e->free_blocks[i] = (int)(e->num_blocks - 1 - i);
        }
    }
    return 0;
}

int tm_engine_prefill(tm_engine* e, const int* host_ids, const int* host_lens, int batch, int max_new_tokens)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e && host_ids && host_lens, "null pointer");
    std::vector<tmk::MmSeqT> mm;
    mm.swap(e->h_mm);  // tm_engine_set_multimodal's input belongs to THIS call: consumed, whatever happens below
    TM_REQUIRE(e->started, "engine not started");
    TM_REQUIRE(e->batch == 0 && !e->sched, "a batch is already admitted (release it first)");
    TM_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch_size, "1 <= batch <= max_batch_size");
    TM_REQUIRE(max_new_tokens >= 1, "max_new_tokens >= 1");
    // speculation armed (tm_engine_set_speculative, k > 0): a greedy text batch only, and k tokens of KV slack behind every sequence --
    // the rows of a verify forward behind the accepted ones are stored, never read, and overwritten by the next step
    const int spec_slack = e->spec_k;
    if (spec_slack > 0) {
        TM_REQUIRE(mm.empty(), "speculative decoding does not take multimodal input (tm_engine_set_speculative with k = 0 first)");
        TM_REQUIRE(e->h_sampling.empty(), "speculative decoding is greedy: sampling parameters are armed (tm_engine_set_sampling)");
        TM_REQUIRE(e->h_logits.empty(), "speculative decoding is greedy: logits processors are armed (tm_engine_set_logits_params)");
        TM_REQUIRE(e->logprobs_next == 0, "speculative decoding does not record logprobs (tm_engine_set_logprobs)");
    }
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    const tm_engine_config& c = e->cfg;

    // ---- admit: reserve blocks for prompt + generation ------------------------------------------
    int64_t need = 0;
    for (int b = 0; b < batch; ++b) {
        TM_REQUIRE(host_lens[b] >= 1, "empty prompt");
        if (host_lens[b] + max_new_tokens + spec_slack > c.session_len) {
            set_last_error(spec_slack ? "prompt + max_new_tokens + speculative tokens exceeds session_len" :
                                        "prompt + max_new_tokens exceeds session_len");
            return TM_TOO_LONG;
        }
        need += kv_blocks_owned((host_lens[b] + max_new_tokens + spec_slack + 63) / 64, e->ring_blocks);
    }
    if (need > (int64_t)e->free_blocks.size()) {
        set_last_error("out of KV cache blocks");
        return TM_OOM;
    }
    std::vector<uint64_t> ptrs((size_t)batch * e->max_blocks_per_seq, 0);
    e->h_blocks.assign(batch, {});
    for (int b = 0; b < batch; ++b) {
        const int nb = (host_lens[b] + max_new_tokens + spec_slack + 63) / 64;
        for (int i = 0; i < kv_blocks_owned(nb, e->ring_blocks); ++i) {
            e->h_blocks[b].push_back(e->free_blocks.back());
            e->free_blocks.pop_back();
        }
        kv_table_row(e, ptrs.data() + (size_t)b * e->max_blocks_per_seq, e->h_blocks[b], nb);
    }
    TM_HIP_CHECK(hipMemcpyAsync(e->d_block_ptrs, ptrs.data(), ptrs.size() * 8, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemsetAsync(e->d_step, 0, 4, e->stream));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    e->batch   = batch;
    e->max_new = max_new_tokens;
    e->h_len.assign(host_lens, host_lens + batch);
    e->steps_done = 0;
    e->steps_fetched = 0;

    e->sampling_on = false;
    if (!e->h_sampling.empty()) {
        TM_REQUIRE((int)e->h_sampling.size() == batch, "tm_engine_set_sampling: batch size differs from the prefill's");
        TM_TRY(sampling_upload(e, e->h_sampling.data(), 0, batch));
        e->sampling_on = true;
    }
    e->logprobs_on = false;
    if (e->logprobs_next > 0) {
        // the logprobs come out of the sampling kernels: greedy rows are their top_k = 1 rows (kept = 1: the token with logprob 0,
        // what the reference reports for top_k = 1 as well)
        if (!e->sampling_on) {
            std::vector<tm_sampling> greedy(batch, tm_sampling{1.f, 1, 1.f, 0.f, 0});
            TM_TRY(sampling_upload(e, greedy.data(), 0, batch));
            e->sampling_on = true;
        }
        const size_t records = (size_t)batch * max_new_tokens, entries = records * e->logprobs_next;
        if (records > e->lpr_records || entries > e->lpr_entries || !e->d_kept) {
            TM_HIP_CHECK(hipStreamSynchronize(e->stream));
            (void)hipFree(e->d_lpr_vals), (void)hipFree(e->d_lpr_idx), (void)hipFree(e->d_lpr_num), (void)hipFree(e->d_lpr_sel);
            e->d_lpr_vals = nullptr, e->d_lpr_idx = nullptr, e->d_lpr_num = nullptr, e->d_lpr_sel = nullptr;
            e->lpr_records = e->lpr_entries = 0;
            TM_TRY(dmalloc(&e->d_lpr_vals, entries));
            TM_TRY(dmalloc(&e->d_lpr_idx, entries));
            TM_TRY(dmalloc(&e->d_lpr_num, records));
            TM_TRY(dmalloc(&e->d_lpr_sel, records));
            if (!e->d_kept) {
                TM_TRY(dmalloc(&e->d_kept, (size_t)e->cfg.max_batch_size));
            }
            e->lpr_records = records;
            e->lpr_entries = entries;
        }
        TM_HIP_CHECK(hipMemsetAsync(e->d_lpr_num, 0, records * 4, e->stream));
        e->logprobs_n  = e->logprobs_next;
        e->logprobs_on = true;
    }
    e->logits_on = false;
    if (!e->h_logits.empty()) {
        TM_REQUIRE((int)e->h_logits.size() == batch, "tm_engine_set_logits_params: batch size differs from the prefill's");
        TM_TRY(logits_upload(e, e->h_logits.data(), host_lens, nullptr, 0, batch));
        e->logits_on = true;
    }
    e->h_ttft_ms.assign(batch, 0.f);
    for (int b = 0; b < batch; ++b) {
        TM_TRY(rope_admit(e, b, host_lens[b]));
    }
    TM_TRY(multimodal_admit(e, mm, host_lens, batch));
    {
        std::vector<const int*> seq_ids(batch);
        int                     off = 0;
        for (int b = 0; b < batch; ++b) {
            seq_ids[b] = host_ids + off;
            off += host_lens[b];
        }
        const int rc = prefill_slots(e, seq_ids.data(), host_lens, batch, 0, e->h_ttft_ms.data());
        e->mm_emb_index.clear();  // the prompt is in the cache: decode needs the slots' deltas only
        e->mm_coords.clear();
        TM_TRY(rc);
    }

    // ---- steady-state decode layout: one token per sequence ------------------------------------------
    std::vector<int> cu_q(batch + 1);
    for (int b = 0; b <= batch; ++b) {
        cu_q[b] = b;
    }
    TM_HIP_CHECK(hipMemcpyAsync(e->d_cu_q, cu_q.data(), cu_q.size() * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_k_len, host_lens, batch * 4, hipMemcpyHostToDevice, e->stream));
    // generated[b][0] = first token; step counter = 1
    TM_HIP_CHECK(hipMemsetAsync(e->d_step, 0, 4, e->stream));
    TM_TRY(commit_tokens(e));
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    e->steps_done = 1;
    e->spec_batch = spec_slack > 0;
    if (e->spec_batch) {  // the device token history: the prompts, then the first token
        std::vector<int> hist((size_t)batch * c.session_len, 0);
        for (int b = 0, off = 0; b < batch; off += host_lens[b], ++b) {
            std::copy(host_ids + off, host_ids + off + host_lens[b], hist.begin() + (size_t)b * c.session_len);
        }
        TM_HIP_CHECK(hipMemcpyAsync(e->d_spec_hist, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, e->stream));
        TM_TRY(launch_spec_begin(spec_state(e), batch, e->stream));
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));  // hist is pageable
        if (e->graph_spec && (e->graph_spec_batch != batch || e->graph_spec_max_new != max_new_tokens || e->graph_spec_k != e->spec_k)) {
            (void)hipGraphExecDestroy(e->graph_spec);  // batch, max_new and k are captured kernel arguments
            e->graph_spec = nullptr;
        }
    }

    setup_decode(e, batch);
    if (e->graph && (e->graph_batch != batch || e->graph_max_new != max_new_tokens || e->graph_sampling != e->sampling_on
                     || e->graph_logits != e->logits_on || e->graph_logprobs != e->logprobs_on || e->logprobs_on)) {
        // (with logprobs on the record pointers and the cap are captured kernel arguments: always re-capture)
        (void)hipGraphExecDestroy(e->graph);
        e->graph = nullptr;
    }
    return 0;
}

// Prompt scoring: chunked prefill of `batch` sequences whose forwards end in the scoring head (forward(), e->scoring) instead of
// the last-token lm_head.  Each sequence holds ceil(len / 64) blocks for the call only (no room for generation); the batch slots,
// d_next_ids, d_logits and the decode graph are not touched, so a later prefill / decode runs as on a fresh engine.
int tm_engine_score(tm_engine* e, const int* host_ids, const int* host_lens, int batch, float* host_nll)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e && host_ids && host_lens && host_nll, "null pointer");
    TM_REQUIRE(e->started, "engine not started");
    TM_REQUIRE(e->batch == 0 && !e->sched, "a batch is already admitted (release it first)");
    TM_REQUIRE(e->cfg.tp == 1 && !e->use_comm, "scoring at tp > 1 is not supported (the vocabulary is sharded across the ranks)");
    TM_REQUIRE(e->h_mm.empty(), "tm_engine_score does not take multimodal input (tm_engine_set_multimodal(e, NULL, 0) clears it)");
    TM_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch_size, "1 <= batch <= max_batch_size");
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    const tm_engine_config& c = e->cfg;
    const int               V = c.model.vocab;

    int64_t need = 0, total = 0;
    for (int b = 0; b < batch; ++b) {
        TM_REQUIRE(host_lens[b] >= 2, "scoring needs at least 2 tokens per sequence");
        if (host_lens[b] >= c.session_len) {
            set_last_error("input length >= session_len");
            return TM_TOO_LONG;
        }
        need += kv_blocks_owned((host_lens[b] + 63) / 64, e->ring_blocks);
        total += host_lens[b];
    }
    for (int64_t i = 0; i < total; ++i) {
        TM_REQUIRE(host_ids[i] >= 0 && host_ids[i] < V, "token id outside [0, vocab)");
    }
    if (need > (int64_t)e->free_blocks.size()) {
        set_last_error("out of KV cache blocks");
        return TM_OOM;
    }
    if (!e->d_score_logits) {
        e->score_rows        = std::min(1024, e->max_tokens);
        e->score_ld          = (e->vocab_local + 7) / 8 * 8;
        const size_t per_seq = (size_t)c.max_batch_size * c.session_len;
        if (hipMalloc((void**)&e->d_score_logits, (size_t)e->score_rows * e->score_ld * sizeof(half_t)) != hipSuccess
            || hipMalloc((void**)&e->d_score_nll, per_seq * sizeof(float)) != hipSuccess
            || hipMalloc((void**)&e->d_score_tgt, per_seq * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(e->d_score_logits), (void)hipFree(e->d_score_nll), (void)hipFree(e->d_score_tgt);
            e->d_score_logits = nullptr, e->d_score_nll = nullptr, e->d_score_tgt = nullptr;
            set_last_error("scoring scratch allocation failed");
            return TM_OOM;
        }
    }
    // targets of every position of the concatenated sequences: the next token, -1 at a sequence's last position (no target)
    std::vector<int>         tgt(total);
    std::vector<const int*>  seq_ids(batch);
    std::vector<int>         blocks;
    std::vector<uint64_t>    ptrs((size_t)batch * e->max_blocks_per_seq, 0);
    for (int b = 0, off = 0; b < batch; off += host_lens[b], ++b) {
        seq_ids[b] = host_ids + off;
        for (int p = 0; p < host_lens[b]; ++p) {
            tgt[off + p] = p + 1 < host_lens[b] ? host_ids[off + p + 1] : -1;
        }
        const int        nb = (host_lens[b] + 63) / 64;
        std::vector<int> own;
        for (int i = 0; i < kv_blocks_owned(nb, e->ring_blocks); ++i) {
            own.push_back(e->free_blocks.back());
            e->free_blocks.pop_back();
        }
        blocks.insert(blocks.end(), own.begin(), own.end());
        kv_table_row(e, ptrs.data() + (size_t)b * e->max_blocks_per_seq, own, nb);
    }
    std::vector<float> nll(total);
    auto run = [&]() -> int {
        TM_HIP_CHECK(hipMemcpyAsync(e->d_block_ptrs, ptrs.data(), ptrs.size() * 8, hipMemcpyHostToDevice, e->stream));
        TM_HIP_CHECK(hipMemcpyAsync(e->d_score_tgt, tgt.data(), tgt.size() * 4, hipMemcpyHostToDevice, e->stream));
        for (int b = 0; b < batch; ++b) {
            TM_TRY(rope_admit(e, b, host_lens[b]));
        }
        e->scoring  = true;
        const int r = prefill_slots(e, seq_ids.data(), host_lens, batch, 0, nullptr);
        e->scoring  = false;
        const int rr = rope_reset(e, 0, batch);  // also behind a failed forward: the slots go back to the shared table
        TM_TRY(r);
        TM_TRY(rr);
        TM_HIP_CHECK(hipMemcpyAsync(nll.data(), e->d_score_nll, nll.size() * 4, hipMemcpyDeviceToHost, e->stream));
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        return 0;
    };
    const int rc = run();
    if (rc) {
        (void)hipStreamSynchronize(e->stream);  // the pageable vectors above must outlive every copy queued from them
    }
    // the blocks go back in reverse order of their removal: the free list is exactly what it was
    for (auto it = blocks.rbegin(); it != blocks.rend(); ++it) {
        e->free_blocks.push_back(*it);
    }
    if (rc) {
        return rc;
    }
    for (int b = 0, off = 0, out = 0; b < batch; off += host_lens[b], ++b) {
        memcpy(host_nll + out, nll.data() + off, (size_t)(host_lens[b] - 1) * sizeof(float));
        out += host_lens[b] - 1;
    }
    return 0;
}

// hipGraph capture of one decode step.  Steps that contain RCCL calls (tp > 1) are captured too -- a TP = 8 step is
// ~290 launches + 65 collectives, far too many for eager launches -- but defensively: if the capture or the instantiation
// fails (RCCL build without graph support, ...) the engine falls back to eager steps for good instead of failing.
bool graph_enabled(const tm_engine* e)
{
    if (!e->cfg.use_graph) {
        return false;
    }
    if (!e->use_comm) {
        return true;
    }
    return e->graph_comm && !e->graph_comm_failed;  // TM_GRAPH_COMM=0 (read at create) keeps collectives out of graphs
}

int capture_step(tm_engine* e, int (*step)(tm_engine*), hipGraphExec_t* exec)
{
    *exec        = nullptr;
    hipGraph_t g = nullptr;
    hipError_t be = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    int        rc = be == hipSuccess ? step(e) : 0;
    hipError_t ce = be == hipSuccess ? hipStreamEndCapture(e->stream, &g) : be;
    hipError_t ie = hipSuccess;
    if (rc == 0 && ce == hipSuccess) {
        ie = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    }
    if (g) {
        (void)hipGraphDestroy(g);
    }
    if (rc == 0 && ce == hipSuccess && ie == hipSuccess) {
        return 0;
    }
    *exec = nullptr;
    if (e->use_comm) {  // collectives inside: give up on graphs, keep running
        (void)hipGetLastError();
        e->graph_comm_failed = true;
        fprintf(stderr, "[tm] hipGraph capture of the tensor-parallel decode step failed (rc %d, capture %s, instantiate %s): "
                        "falling back to eager launches\n", rc, hipGetErrorString(ce), hipGetErrorString(ie));
        return 0;
    }
    if (rc) {
        return rc;
    }
    TM_HIP_CHECK(ce);
    TM_HIP_CHECK(ie);
    return 0;
}

int tm_engine_decode(tm_engine* e, int steps)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e && e->batch > 0, "no admitted batch");
    TM_REQUIRE(!e->sched, "continuous-batching session active: use tm_engine_step");
    TM_REQUIRE(!e->spec_batch, "the batch was admitted with speculation armed: use tm_engine_decode_spec / tm_engine_verify");
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    if (e->steps_done + steps > e->max_new) {
        set_last_error("decode past max_new_tokens");
        return TM_TOO_LONG;
    }
    if (graph_enabled(e) && !e->graph) {
        // run one eager step first (lazy module loading etc. must not happen inside a capture)
        if (steps == 0) {
            return 0;
        }
        TM_TRY(decode_step(e));
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        e->steps_done += 1;
        steps -= 1;
        TM_TRY(capture_step(e, decode_step, &e->graph));
        e->graph_batch    = e->batch;
        e->graph_max_new  = e->max_new;
        e->graph_sampling = e->sampling_on;
        e->graph_logits   = e->logits_on;
        e->graph_logprobs = e->logprobs_on;
    }
    for (int i = 0; i < steps; ++i) {
        if (graph_enabled(e) && e->graph) {
            TM_HIP_CHECK(hipGraphLaunch(e->graph, e->stream));
        }
        else {
            TM_TRY(decode_step(e));
        }
    }
    e->steps_done += steps;
    return 0;
}

int tm_engine_set_speculative(tm_engine* e, int k, int ngram_max, int ngram_min)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(e->batch == 0, "set the speculative configuration before tm_engine_prefill (a batch is admitted)");
    if (k == 0) {
        e->spec_k = 0;
        return 0;
    }
    TM_REQUIRE(!e->sched, "speculative decoding: a continuous-batching session is open (continuous batching does not speculate)");
    TM_REQUIRE(e->started, "engine not started");
    TM_REQUIRE(k >= 1 && k <= kSpecMaxDraft, "speculative decoding: 1 <= k <= 7 (k + 1 rows per sequence in the verify attention)");
    TM_REQUIRE(1 <= ngram_min && ngram_min <= ngram_max && ngram_max <= kSpecMaxNgram,
               "speculative decoding: 1 <= ngram_min <= ngram_max <= 8");
    const tm_engine_config& c = e->cfg;
    TM_REQUIRE(c.tp == 1 && !e->use_comm, "speculative decoding with tp > 1 is not built");
    TM_REQUIRE(c.quant_policy != 42, "speculative decoding with quant_policy 42 (TurboQuant KV) is not built");
    TM_REQUIRE(!e->windowed, "speculative decoding with a sliding window or attention sinks is not built");
    TM_REQUIRE(e->mrope_section[0] + e->mrope_section[1] + e->mrope_section[2] == 0,
               "speculative decoding with M-RoPE sections (multimodal models) is not built");
    const int B = c.max_batch_size;
    TM_REQUIRE((int64_t)B * (k + 1) <= e->max_tokens,
               "speculative decoding: max_batch_size * (k + 1) rows exceed one forward (raise max_prefill_token_num)");
    TM_HIP_CHECK(hipSetDevice(c.device));
    if (!e->d_spec_hist) {
        TM_TRY(dmalloc(&e->d_spec_hist, (size_t)B * c.session_len));
        TM_TRY(dmalloc(&e->d_spec_len, (size_t)B));
        TM_TRY(dmalloc(&e->d_spec_emitted, (size_t)B));
        TM_TRY(dmalloc(&e->d_spec_ndraft, (size_t)B));
        TM_TRY(dmalloc(&e->d_spec_k_len, (size_t)B));
        TM_TRY(dmalloc(&e->d_spec_step, (size_t)B));
        TM_TRY(dmalloc(&e->d_spec_cu_q, (size_t)B + 1));
        TM_TRY(dmalloc(&e->d_spec_totals, (size_t)4));
        TM_HIP_CHECK(hipMemset(e->d_spec_totals, 0, 4 * sizeof(long long)));
    }
    if (k > e->spec_cap_k) {  // the buffers that scale with k
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        for (void* q : {(void*)e->d_spec_drafts, (void*)e->d_spec_ids, (void*)e->d_spec_out, (void*)e->d_spec_logits, (void*)e->d_spec_attn_ws}) {
            if (q) {
                (void)hipFree(q);
            }
        }
        e->d_spec_drafts = e->d_spec_ids = e->d_spec_out = nullptr;
        e->d_spec_logits = nullptr, e->d_spec_attn_ws = nullptr, e->spec_cap_k = 0;
        const size_t rows = (size_t)B * (k + 1);
        TM_TRY(dmalloc(&e->d_spec_drafts, (size_t)B * k));
        TM_TRY(dmalloc(&e->d_spec_ids, rows));
        TM_TRY(dmalloc(&e->d_spec_out, rows));
        TM_TRY(dmalloc(&e->d_spec_logits, rows * e->vocab_local));
        TM_HIP_CHECK(hipMalloc((void**)&e->d_spec_attn_ws, decode_attention_workspace_bytes((int)rows, e->q_heads, 128, 16)));
        e->spec_cap_k = k;
    }
    std::vector<int> cu(B + 1);
    for (int b = 0; b <= B; ++b) {
        cu[b] = b * (k + 1);
    }
    TM_HIP_CHECK(hipMemcpy(e->d_spec_cu_q, cu.data(), cu.size() * 4, hipMemcpyHostToDevice));
    e->spec_k         = k;
    e->spec_ngram_max = ngram_max;
    e->spec_ngram_min = ngram_min;
    e->spec_mfma      = (c.quant_policy == 8 || c.quant_policy == 4) && e->D == 128;
    return 0;
}

static int spec_entry(tm_engine* e)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e && e->batch > 0, "no admitted batch");
    TM_REQUIRE(e->spec_batch && e->spec_k > 0, "the batch was admitted without speculation (tm_engine_set_speculative before tm_engine_prefill)");
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    return 0;
}

int tm_engine_decode_spec(tm_engine* e, int steps)
{
    TM_TRY(spec_entry(e));
    TM_REQUIRE(steps >= 0, "steps >= 0");
    // the flatten + prefill-attention path needs host-side lengths per step: it stays eager
    const bool graphs = graph_enabled(e) && e->spec_mfma;
    if (graphs && !e->graph_spec) {
        if (steps == 0) {
            return 0;
        }
        TM_TRY(spec_step(e));  // one eager step first, as tm_engine_decode
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        steps -= 1;
        TM_TRY(capture_step(e, spec_step, &e->graph_spec));
        e->graph_spec_batch   = e->batch;
        e->graph_spec_max_new = e->max_new;
        e->graph_spec_k       = e->spec_k;
    }
    for (int i = 0; i < steps; ++i) {
        if (graphs && e->graph_spec) {
            TM_HIP_CHECK(hipGraphLaunch(e->graph_spec, e->stream));
        }
        else {
            TM_TRY(spec_step(e));
        }
    }
    return 0;
}

int tm_engine_verify(tm_engine* e, const int* host_drafts, const int* host_n_draft)
{
    TM_TRY(spec_entry(e));
    TM_REQUIRE(host_drafts && host_n_draft, "null pointer");
    const int k = e->spec_k;
    for (int b = 0; b < e->batch; ++b) {
        TM_REQUIRE(host_n_draft[b] >= 0 && host_n_draft[b] <= k, "tm_engine_verify: 0 <= n_draft[b] <= k");
        for (int j = 0; j < k; ++j) {
            TM_REQUIRE(host_drafts[b * k + j] >= 0 && host_drafts[b * k + j] < e->cfg.model.vocab, "tm_engine_verify: a draft id outside [0, vocab)");
        }
    }
    TM_HIP_CHECK(hipMemcpyAsync(e->d_spec_drafts, host_drafts, (size_t)e->batch * k * 4, hipMemcpyHostToDevice, e->stream));
    TM_HIP_CHECK(hipMemcpyAsync(e->d_spec_ndraft, host_n_draft, (size_t)e->batch * 4, hipMemcpyHostToDevice, e->stream));
    const int rc = spec_verify_accept(e);
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));  // the caller's arrays may be pageable
    return rc;
}

int tm_engine_fetch_spec(tm_engine* e, int* host_tokens, int* host_counts)
{
    TM_REQUIRE(e && host_tokens && host_counts, "null pointer");
    TM_REQUIRE(e->batch > 0 && e->spec_batch, "no batch admitted with speculation armed");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    TM_HIP_CHECK(hipMemcpy(host_tokens, e->d_generated, (size_t)e->batch * e->max_new * 4, hipMemcpyDeviceToHost));
    TM_HIP_CHECK(hipMemcpy(host_counts, e->d_spec_emitted, (size_t)e->batch * 4, hipMemcpyDeviceToHost));
    return 0;
}

int tm_engine_fetch_spec_logits(tm_engine* e, void* host_out)
{
    TM_REQUIRE(e && host_out, "null pointer");
    TM_REQUIRE(e->batch > 0 && e->spec_batch, "no batch admitted with speculation armed");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    TM_HIP_CHECK(hipMemcpy(host_out, e->d_spec_logits, (size_t)e->batch * (e->spec_k + 1) * e->vocab_local * 2, hipMemcpyDeviceToHost));
    return 0;
}

int tm_engine_spec_stats(tm_engine* e, int64_t* host_stats)
{
    TM_REQUIRE(e && host_stats, "null pointer");
    if (!e->d_spec_totals) {  // never armed
        host_stats[0] = host_stats[1] = host_stats[2] = host_stats[3] = 0;
        return 0;
    }
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    TM_HIP_CHECK(hipMemcpy(host_stats, e->d_spec_totals, 4 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int tm_engine_set_sampling(tm_engine* e, const tm_sampling* host_params, int batch)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(e->batch == 0 && !e->sched, "set the sampling parameters before tm_engine_prefill");
    e->h_sampling.clear();
    if (!host_params) {
        return 0;
    }
    TM_REQUIRE(!e->use_comm || e->comm || e->p2p_ready,
               "stochastic sampling with tp > 1 gathers the logits: tm_engine_comm_init or the native communicator first");
    TM_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch_size, "1 <= batch <= max_batch_size");
    for (int i = 0; i < batch; ++i) {
        TM_REQUIRE(host_params[i].temperature > 0.f, "sampling: temperature must be > 0");
    }
    e->h_sampling.assign(host_params, host_params + batch);
    return 0;
}

int tm_engine_set_logprobs(tm_engine* e, int n)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(e->batch == 0 && !e->sched, "set the logprobs count before tm_engine_prefill");
    TM_REQUIRE(n >= 0 && n <= kMaxLogProb, "0 <= logprobs <= TM_MAX_LOGPROBS");
    TM_REQUIRE(n == 0 || !e->use_comm || e->comm || e->p2p_ready,
               "logprobs with tp > 1 gather the logits like stochastic sampling: tm_engine_comm_init or the native communicator first");
    e->logprobs_next = n;
    return 0;
}

int tm_engine_fetch_logprobs(tm_engine* e, float* host_vals, int* host_idx, int* host_num, float* host_sel)
{
    TM_REQUIRE(e && host_vals && host_idx && host_num && host_sel, "null pointer");
    TM_REQUIRE(e->batch > 0 && !e->sched && e->logprobs_on, "no admitted static batch with logprobs (tm_engine_set_logprobs before the prefill)");
    TM_HIP_CHECK(hipStreamSynchronize(e->stream));
    const size_t records = (size_t)e->batch * e->max_new;
    TM_HIP_CHECK(hipMemcpy(host_vals, e->d_lpr_vals, records * e->logprobs_n * 4, hipMemcpyDeviceToHost));
    TM_HIP_CHECK(hipMemcpy(host_idx, e->d_lpr_idx, records * e->logprobs_n * 4, hipMemcpyDeviceToHost));
    TM_HIP_CHECK(hipMemcpy(host_num, e->d_lpr_num, records * 4, hipMemcpyDeviceToHost));
    TM_HIP_CHECK(hipMemcpy(host_sel, e->d_lpr_sel, records * 4, hipMemcpyDeviceToHost));
    return 0;
}

int tm_engine_set_logits_params(tm_engine* e, const tm_logits_param* host_params, int batch)
{
    TM_REQUIRE(e, "null pointer");
    TM_REQUIRE(e->batch == 0 && !e->sched, "set the logits-processor parameters before tm_engine_prefill");
    e->h_logits.clear();
    if (!host_params) {
        return 0;
    }
    TM_REQUIRE(batch >= 1 && batch <= e->cfg.max_batch_size, "1 <= batch <= max_batch_size");
    for (int i = 0; i < batch; ++i) {
        TM_TRY(logits_param_check(host_params[i]));
    }
    e->h_logits.assign(host_params, host_params + batch);
    return 0;
}

int tm_engine_prefill_times(tm_engine* e, float* host_ms)
{
    TM_REQUIRE(e && host_ms, "null pointer");
    TM_REQUIRE((int)e->h_ttft_ms.size() == e->batch, "no admitted batch");
    memcpy(host_ms, e->h_ttft_ms.data(), sizeof(float) * e->batch);
    return 0;
}

int tm_engine_profile_decode(tm_engine* e, int steps, float* host_ms_per_step, int* host_launches_per_step)
{
    if (e && e->loop_on.load()) {
        set_last_error("the engine thread is running (tm_engine_serve_stop first)");
        return TM_CONFLICT;
    }
    TM_REQUIRE(e && host_ms_per_step && e->batch > 0 && steps >= 1, "arguments");
    TM_HIP_CHECK(hipSetDevice(e->cfg.device));
    if (e->steps_done + steps > e->max_new) {
        set_last_error("decode past max_new_tokens");
        return TM_TOO_LONG;
    }
    std::vector<double> acc(P_NUM, 0.0);
    std::vector<int>    cnt(P_NUM, 0);
    for (int i = 0; i < steps; ++i) {
        e->prof_on   = true;
        e->prof_used = 0;
        e->prof_spans.clear();
        int rc     = decode_step(e);
        e->prof_on = false;
        if (rc) {
            return rc;
        }
        TM_HIP_CHECK(hipStreamSynchronize(e->stream));
        for (auto& sp : e->prof_spans) {
            float ms = 0.f;
            TM_HIP_CHECK(hipEventElapsedTime(&ms, e->prof_pool[std::get<1>(sp)], e->prof_pool[std::get<2>(sp)]));
            acc[std::get<0>(sp)] += ms;
            cnt[std::get<0>(sp)] += 1;
        }
        e->steps_done += 1;
    }
    for (int c = 0; c < P_NUM; ++c) {
        host_ms_per_step[c] = (float)(acc[c] / steps);
        if (host_launches_per_step) {
            host_launches_per_step[c] = cnt[c] / steps;
        }
    }
    return 0;
}

}  // extern "C"
