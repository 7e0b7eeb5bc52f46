/*
 * tm_mi355x.h -- C ABI of libtm_mi355x.so: the MI355X-native (gfx950, hand-written HIP) replacement for the
 * TurboMind quantized decode hot path of InternLM/lmdeploy.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes (device pointers unless noted "host"),
 * never throws and never aborts on the request path: it returns a tm_status code, and tm_last_error()
 * describes the last failure on the calling thread.  Streams are hipStream_t passed as void*.
 *
 * What each group replaces in the reference (paths relative to the lmdeploy checkout, v0.16.0):
 *   engine  : pybind11 module `_turbomind` -- TurboMind.create / create_context / create_root / process_weight /
 *             create_engine / ModelRequest.forward  (src/turbomind/python/bind.cpp:743-793,938-999;
 *             src/turbomind/turbomind.cc:159-361), weight slots = Module/Param protocol
 *             (lmdeploy/turbomind/builders/_base.py:72-99).
 *   linear  : `_tm.LinearWeight` + `_tm.LlamaLinear.forward_dense` + `tm.QuantizeGroupwise`
 *             (src/turbomind/python/linear_bind.cpp:111-137,265-294), the operator-level surface the
 *             reference's tests/turbomind/linear fixtures drive.
 *   kernels : invokeRMSNorm / invokeResidualBiasRMSNorm (kernels/norm/rms_norm.cu), invokeProcessKV_v2_ /
 *             invokeFlattenKV_v2_ (kernels/attention/kv_cache_utils_v2.h:36-112), dispatchDecoding /
 *             dispatchAttention (kernels/attention/decoding.cu, attention.cu), embedding + greedy sampling.
 */
#ifndef TM_MI355X_H
#define TM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Request status codes == src/turbomind/engine/request.h:120-131 */
enum tm_status {
    TM_OK        = 0,
    TM_INVALID   = 1,
    TM_CONFLICT  = 2,
    TM_FAIL      = 5,
    TM_TOO_LONG  = 6,
    TM_FINISH    = 7,
    TM_CANCEL    = 8,
    TM_NO_QUEUE  = 10,
    TM_OOM       = 11
};

typedef void* tm_stream_t; /* hipStream_t; NULL = default stream */

int         tm_version(void);
const char* tm_last_error(void);
/* number of visible gfx950 devices (0 without a GPU); never fails */
int         tm_device_count(void);

/* ----------------------------------------------------------------------------------------------
 * Paged KV cache view (kernels/attention/block.h:126-219, block_iterator.h:9-100)
 * --------------------------------------------------------------------------------------------*/
typedef struct tm_kv_cache {
    const uint64_t* block_ptrs;    /* device: base address of every cache block (char**)           */
    const int*      cu_block_nums; /* device [batch+1]: first block of each sequence in block_ptrs */
    int64_t         layer_offset;  /* bytes: layer * tm_kv_layer_size()                            */
    int             kv_heads;      /* local kv heads                                               */
    int             head_dim;      /* 64 | 128                                                     */
    int             block_len;     /* 64 tokens (lmdeploy/messages.py:323)                         */
    int             bits;          /* quant_policy: 16 (none) | 8 | 4 | 42 (lmdeploy/messages.py:20-27) */
} tm_kv_cache;

/* bytes of one layer inside a block: kv_heads*2*block_len*(head_dim*bits/8) + kv_heads*2*block_len*4*[bits<16].
 * bits 42 (TurboQuant, head_dim 128 only): K rows of head_dim/2 bytes (3-bit Lloyd-Max code of the Hadamard-rotated row + the sign of
 * the residual per element), V rows of head_dim/4 bytes (2-bit code), one fp16 pair per row each (K: norm, residual norm; V: norm, 0):
 * kv_heads*block_len*(head_dim/2 + head_dim/4 + 8).  Per kv head K data [block_len][head_dim/2], then V data [block_len][head_dim/4];
 * behind the data of all heads, per head, K params then V params.  tm_kv_rope_store*, tm_flatten_kv and tm_decode_attention serve it;
 * head_dim 64, the fused decode prologue, a window > 0 and sinks return TM_INVALID with bits 42. */
int64_t tm_kv_layer_size(int kv_heads, int head_dim, int block_len, int bits);

/* ----------------------------------------------------------------------------------------------
 * Operator level
 * --------------------------------------------------------------------------------------------*/
/* y = rmsnorm(x) * w          x,y fp16 [M,H], w fp16 [H]                     (rms_norm.cu:21-138) */
int tm_rmsnorm(void* y, const void* x, const void* w, float eps, int M, int H, tm_stream_t st);
/* r <- r + hidden (+ bias), y <- rmsnorm(r) * w ; residual stream accumulates in fp16 (rms_norm.cu:286-362).
 * If `partial` != NULL, hidden is given as `splits` fp32 split-K slabs [splits][M][H] (hidden must be NULL). */
int tm_residual_rmsnorm(void* y, void* resid, const void* hidden, const float* partial, int splits,
                        const void* bias, const void* w, float eps, int M, int H, tm_stream_t st);
/* The same two operators over zero-padded rows (a model whose hidden size is served padded to a multiple of 128): only the columns
 * [0, Hv) are the row, Hv % 8 == 0, 0 < Hv <= H.  The sum of squares runs over them and is divided by Hv; the columns [Hv, H) of x /
 * resid / hidden / partial are never read -- a NaN there reaches no output -- and y (and resid) receive +0 there.  bias and w are
 * read on [0, Hv) only.  Hv == H forwards to tm_rmsnorm / tm_residual_rmsnorm. */
int tm_rmsnorm_valid(void* y, const void* x, const void* w, float eps, int M, int H, int Hv, tm_stream_t st);
int tm_residual_rmsnorm_valid(void* y, void* resid, const void* hidden, const float* partial, int splits,
                              const void* bias, const void* w, float eps, int M, int H, int Hv, tm_stream_t st);

/* (cos,sin) fp16 table [max_pos][rope_dim/2][2] on the HOST (rotary_embedding.h:11-52, attention_weight.cc:37-93).
 * rope_type: 0 default, 1 linear, 2 llama3.  The caller uploads it. */
int tm_rope_table(void* host_out, int max_pos, int rope_dim, float base, int rope_type, float factor,
                  float low_freq_factor, float high_freq_factor, int original_max_position);

/* The same recipe for every RoPE type (RopeConfig, init_rope_kernel_param: attention_weight.cc:37-93; rotary_embedding.h:11-110):
 * type 0 default, 1 linear, 2 llama3, 3 yarn, 4 dynamic.  yarn: inv_freq = freq - freq * alpha * (1 - 1 / factor) with alpha the ramp
 * between the correction dimensions of yarn_beta_fast / yarn_beta_slow rotations over max_position_embeddings, and cos / sin scaled by
 * yarn_attention_factor in fp32 before the cast to fp16.  dynamic: the default recipe of `base` (the caller passes the SEQUENCE's
 * base, tm_rope_dynamic_base); factor and max_position_embeddings only feed that function.
 * yarn_truncate (yarn only): 1 = the correction dimensions are rounded outwards (floor / ceil: the reference, and transformers'
 * default); 0 = they stay fractional (transformers' `truncate: false`, gpt-oss).  The clamps to [0, dim - 1] and the low == high guard
 * apply to both. */
typedef struct tm_rope_param {
    int   dim;
    float base;
    int   type;
    float factor, low_freq_factor, high_freq_factor;
    int   original_max_position;
    int   max_position_embeddings;
    float yarn_beta_fast, yarn_beta_slow, yarn_attention_factor;
    int   yarn_truncate;
} tm_rope_param;
/* tm_rope_table for every type: fp32 products, exp2 / sin / cos in double on those fp32 values, rounded fp32 -> fp16 */
int tm_rope_table_ex(void* host_out, int max_pos, const tm_rope_param* p);
/* the recipe's per-pair inverse frequencies themselves (host): inv_freq fp32 [dim / 2], *attention_factor (may be NULL) the factor
 * the table scales cos / sin by */
int tm_rope_inv_freq(float* inv_freq, float* attention_factor, const tm_rope_param* p);
/* the same table built on the DEVICE (asynchronous on `st`; inverse frequencies from the host recipe, angles / cos / sin per entry
 * as on the host) */
int tm_rope_table_device(void* dev_out, int max_pos, const tm_rope_param* p, tm_stream_t st);
/* dynamic NTK (init_dynamic_ntk, unified_attention_layer.cc:228-243): factor > 1 and prompt_len > max_position_embeddings
 * -> base * s ^ (dim / (dim - 2)) with s = factor * prompt_len / max_position_embeddings - (factor - 1) in float as the reference has
 * it, the power in double and rounded to float once (the reference's powf with a float exponent lies up to ~5 fp32 ulps from the
 * formula's value); else base.  The engine fixes a sequence's base with exactly this function when the sequence is admitted. */
float tm_rope_dynamic_base(float base, float factor, int dim, int max_position_embeddings, int prompt_len);

/* RoPE(q,k) + quantise-and-store K/V of the new tokens into the paged cache (ProcessKV_v2 / decode prologue).
 * qkv fp16 [total_tokens][(q_heads + 2 kv_heads)*head_dim]; q is rotated in place.  cache->head_dim is 64 or 128 (cos_sin rows
 * of head_dim / 2 pairs).
 * cu_q_len [batch+1], k_len [batch] = context length of each sequence AFTER adding its new tokens (device).
 * cos_sin may be NULL (no rotation). */
int tm_kv_rope_store(void* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                     const void* cos_sin, int max_pos, const tm_kv_cache* cache, tm_stream_t st);
/* The same with the Qwen attention prologue in front of RoPE, each part optional (NULL = off): q_norm / k_norm fp16 [128]
 * (both or neither) -> per-head RMSNorm of every q / k head, y = h(h(f32(x) * inv) * w), inv = 1 / sqrt(sum f32(x)^2 / 128 + eps)
 * (Qwen3; head_dim 128 only: with head_dim 64 the norm returns TM_INVALID); then qkv_bias fp16 [(q_heads + 2 kv_heads)*head_dim]
 * added to q, k and v in fp16 (Qwen2; head_dim 64 or 128).  With all three NULL this is tm_kv_rope_store. */
int tm_kv_rope_store_qk(void* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                        const void* cos_sin, int max_pos, const void* qkv_bias, const void* q_norm, const void* k_norm, float qk_eps,
                        const tm_kv_cache* cache, tm_stream_t st);
/* tm_kv_rope_store_qk with per-sequence tables: rope_row0 device int [batch] (NULL = tm_kv_rope_store_qk), sequence b reads table row
 * rope_row0[b] + min(pos, max_pos - 1) -- cos_sin holds several regions of max_pos rows, an offset of 0 is the first (shared) one. */
int tm_kv_rope_store_seq(void* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                         const void* cos_sin, int max_pos, const int* rope_row0, const void* qkv_bias, const void* q_norm,
                         const void* k_norm, float qk_eps, const tm_kv_cache* cache, tm_stream_t st);
/* tm_kv_rope_store_qk with multimodal RoPE in sections (Qwen2-VL; the reference's RopeType::kMrope / FastRoPE mode kChunked,
 * src/turbomind/kernels/attention/rotary_embedding.h:112-193).  Frequency pair j = (x[2j], x[2j+1]) of every q / k head takes table
 * row clamp(c, 0, max_pos - 1) of ONE of three coordinates -- t for j < sec_t, h for j < sec_t + sec_h, w behind -- and entry j of
 * that row; the rotation is tm_kv_rope_store's.  mrope_pos: device int [total_tokens][3] (t, h, w) for the rows of this call, or
 * NULL: all three are the row's linear position + pos_delta[b] (pos_delta device int [batch], NULL = 0).  K / V land at the linear
 * position either way.  Equal coordinates = the linear position and no delta give tm_kv_rope_store_qk's bits.  head_dim 128, kv bits
 * 16 / 8 / 4, one table: kv bits 42, head_dim 64, a NULL table and sections that do not sum to 64 return TM_INVALID by name. */
int tm_kv_rope_store_mrope(void* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                           const void* cos_sin, int max_pos, const int* mrope_pos, const int* pos_delta, int sec_t, int sec_h,
                           int sec_w, const void* qkv_bias, const void* q_norm, const void* k_norm, float qk_eps,
                           const tm_kv_cache* cache, tm_stream_t st);
/* FlattenKV_v2: dequantise the whole context into linear fp16 scratch.  k_out [kv_heads][k_stride][head_dim];
 * v_out the same, or transposed [kv_heads][head_dim][k_stride] when transpose_v != 0 (head_dim 64 or 128; the transposed rows are
 * zero-filled from k_len up to the next multiple of 64).  Sequence b starts at
 * cu_k_off[b] (device; must be 64-aligned when transposing). */
int tm_flatten_kv(void* k_out, void* v_out, int transpose_v, const int* cu_k_off, const int* k_len, int batch,
                  int max_k_len, int k_stride, const tm_kv_cache* cache, tm_stream_t st);
/* tm_flatten_kv in front of tm_prefill_attention_window: cu_q_len (device, [batch + 1]) are the query rows of the forward, so
 * sequence b has hist = k_len[b] - q_len[b] cached tokens in front of them.  Every 64-token tile with
 * t0 + 64 <= max(hist - window + 1, 0) is skipped: its cache block is not read and its part of k_out / v_out is left UNWRITTEN
 * (nothing is zero-filled) -- the windowed prefill kernel starts its key loop at floor64(max(hist - window + 1, 0)) and never
 * stages those keys.  Every other tile holds tm_flatten_kv's bytes.  window == 0 is tm_flatten_kv, bit for bit (cu_q_len may
 * be NULL then); window < 0: TM_INVALID. */
int tm_flatten_kv_window(void* k_out, void* v_out, int transpose_v, const int* cu_k_off, const int* k_len, int batch,
                         int max_k_len, int k_stride, const tm_kv_cache* cache, const int* cu_q_len, int window, tm_stream_t st);

/* Paged flash-decode, one query token per sequence (dispatchDecoding).  q fp16 [batch][q_stride] already
 * rotated (head h at h*head_dim), out fp16 [batch][q_heads*head_dim], head_dim = cache->head_dim (64 or 128).  splits >= 1;
 * workspace of tm_decode_attention_workspace() bytes needed when splits > 1 (sized for head_dim 128, which is enough for 64).
 * softmax_scale <= 0 -> 1/sqrt(head_dim).  head_dim 64 runs the VALU kernel for every KV width.
 * Every k_len[b] >= 1 and the first block-table entry of every sequence is a mapped block (the engine parks free batch slots on a
 * dummy block with k_len = 1); a k_len = 0 entry reads that first block and produces no meaningful row. */
size_t tm_decode_attention_workspace(int batch, int q_heads, int splits);
int    tm_decode_attention(void* out, const void* q, int q_stride, const int* k_len, int batch, int q_heads,
                           float softmax_scale, int splits, void* workspace, const tm_kv_cache* cache,
                           tm_stream_t st);
/* Decode attention with the reference decode kernel's fused prologue (attention_universal.h:168-330: the decode
 * kernel itself applies RoPE to q/k and quantises + stores the new K/V).  int8 / int4 KV.  Input is the raw QKV
 * projection of the new token of every sequence: qkv_splits == 0 -> `qkv` is fp16 [batch][qkv_n]; qkv_splits >= 1
 * -> `qkv` is fp32 split-K slabs [qkv_splits][batch][qkv_n] which are summed in order and rounded to fp16 first.
 * Row layout [Q heads | K heads | V heads] x 128: head_dim 128 only, a cache of head_dim 64 returns TM_INVALID (run
 * tm_kv_rope_store + tm_decode_attention).  k_len INCLUDES the new token.  Cache bytes/params written are
 * bit-identical to tm_kv_rope_store; `out` equals tm_decode_attention on that cache. */
int tm_decode_attention_fused(void* out, const void* qkv, int qkv_splits, int qkv_n, const void* cos_sin, int max_pos,
                              const int* k_len, int batch, int q_heads, float softmax_scale, int splits,
                              void* workspace, const tm_kv_cache* cache, tm_stream_t st);
/* The same with the Qwen prologue of tm_kv_rope_store_qk (norm -> bias -> RoPE) applied to the new token's q / k / v; cache
 * bytes / params bit-identical to tm_kv_rope_store_qk with the same arguments. */
int tm_decode_attention_fused_qk(void* out, const void* qkv, int qkv_splits, int qkv_n, const void* cos_sin, int max_pos,
                                 const void* qkv_bias, const void* q_norm, const void* k_norm, float qk_eps, const int* k_len,
                                 int batch, int q_heads, float softmax_scale, int splits, void* workspace, const tm_kv_cache* cache,
                                 tm_stream_t st);
/* tm_decode_attention_fused_qk with a per-sequence position delta (M-RoPE models: a decode token sits at linear position + delta on
 * all three axes): the new token's RoPE row is clamp(k_len[b] - 1 + pos_delta[b], 0, max_pos - 1); pos_delta device int [batch].
 * NULL is tm_decode_attention_fused_qk (the same kernel instantiation); a delta array of zeros gives its bits.  Needs cos_sin. */
int tm_decode_attention_fused_delta(void* out, const void* qkv, int qkv_splits, int qkv_n, const void* cos_sin, int max_pos,
                                    const int* pos_delta, const void* qkv_bias, const void* q_norm, const void* k_norm, float qk_eps,
                                    const int* k_len, int batch, int q_heads, float softmax_scale, int splits, void* workspace,
                                    const tm_kv_cache* cache, tm_stream_t st);
/* tm_decode_attention with a sliding window and attention sinks (AttentionParams::window_size / ::sinks,
 * src/turbomind/kernels/attention/attention_params.h:55-72; the tile skip of decoding_template.h:29 and
 * attention_universal.h:411,474-480; the sink term L += expf(sink - M * scale) of attention_universal.h:529-535).
 * window > 0: the query at k_len - 1 sees the keys j with k_len - 1 - j < window, i.e. the last min(k_len, window) tokens; cache
 * tiles wholly before them are not read.  sinks (device fp16 [q_heads], may be NULL): one natural-log logit per head that joins
 * the softmax denominator and contributes no value.  Runs the VALU kernel for every KV width and head_dim (never the MFMA
 * kernel or its fused prologue).  window == 0 && sinks == NULL is tm_decode_attention, bit for bit; window < 0: TM_INVALID. */
int tm_decode_attention_window(void* out, const void* q, int q_stride, const int* k_len, int batch, int q_heads,
                               float softmax_scale, int splits, void* workspace, const tm_kv_cache* cache, int window,
                               const void* sinks, tm_stream_t st);
/* Verify attention (speculative decoding): paged split-K flash-decode for q_len[b] = cu_q_len[b + 1] - cu_q_len[b] query rows per
 * sequence, 1 <= q_len[b] <= 8, over int8 / int4 KV at head_dim 128 on the matrix cores.  The rows' K / V are in the cache already
 * (tm_kv_rope_store first, the prefill convention): k_len[b] counts EVERY row of this forward, hist = k_len[b] - q_len[b], and query
 * row j of sequence b sees the tokens t < hist + j + 1.  q fp16 [rows][q_stride] rotated, out fp16 [rows][q_heads * 128] in forward
 * row order; cu_q_len, k_len: device.  A score column of the kernel is a (row, query head) pair of one kv head -- q_len * group columns
 * in chunks of 16, so q_len * group <= 16 costs the cache bytes and the MFMA count of one decode token.  splits >= 1; the workspace
 * (tm_verify_attention_workspace bytes for rows = cu_q_len[batch]) is needed when splits > 1.  The call reads cu_q_len and k_len
 * back to check them (it synchronises the stream); the engine's own verify forward does not.  TM_INVALID by name: a q_len outside
 * 1 .. 8, k_len[b] < q_len[b], fp16 KV, kv bits 42, head_dim 64 (those run tm_flatten_kv + tm_prefill_attention).  No window, no
 * sinks, no fused prologue. */
size_t tm_verify_attention_workspace(int rows, int q_heads, int splits);
int    tm_verify_attention(void* out, const void* q, int q_stride, const int* cu_q_len, const int* k_len, int batch, int q_heads,
                           float softmax_scale, int splits, void* workspace, const tm_kv_cache* cache, tm_stream_t st);
/* The device side of speculative decoding by prompt lookup, one sequence batch at a time (operator level; the engine runs the same
 * kernels).  State, all device int arrays: hist [batch][hist_stride] token history (prompt + emitted tokens) and hist_len [batch];
 * emitted [batch] tokens emitted so far; generated [batch][max_new]; k_len [batch]; next_id [batch]; totals int64 [4] = (sequence-steps
 * that emitted, drafted, accepted, emitted), added to.
 * tm_spec_propose: per sequence, for n = ngram_max .. ngram_min the suffix hist[L - n : L] is looked up among the starts i with
 * hist[i : i + n] == suffix and i + n <= L - 1; the largest i of the first n that matches gives drafts[b] = hist[i + n : min(i + n + k, L)],
 * n_draft[b] its length capped at max_new - emitted[b] - 1 (0: no match).  drafts [batch][k] (unused entries 0).
 * tm_spec_accept: out_ids [batch][k + 1] = the greedy token behind every row of the verify forward (row 0 = next_id, rows 1 .. k the
 * drafts); a = the longest prefix of the n_draft drafts with out_ids[j] == drafts[j]; out_ids[0 .. a] are emitted, cut at max_new -
 * emitted[b], appended to generated and hist; k_len += emitted, next_id = the last one; step_emitted [batch] (may be NULL) receives the
 * count.  A sequence with emitted == max_new is left alone.  1 <= k <= 7, 1 <= ngram_min <= ngram_max <= 8. */
int tm_spec_propose(int* drafts, int* n_draft, const int* hist, int hist_stride, const int* hist_len, const int* emitted, int max_new,
                    int batch, int k, int ngram_max, int ngram_min, tm_stream_t st);
int tm_spec_accept(const int* out_ids, const int* drafts, const int* n_draft, int* hist, int hist_stride, int* hist_len, int* emitted,
                   int* generated, int max_new, int* k_len, int* next_id, int64_t* totals, int* step_emitted, int batch, int k,
                   tm_stream_t st);
/* Causal prefill attention over flattened KV (dispatchAttention).  vt is the transposed V of tm_flatten_kv.  head_dim 128;
 * softmax_scale <= 0 -> 1/sqrt(128). */
int tm_prefill_attention(void* out, const void* q, int q_stride, const void* k, const void* vt, int k_stride,
                         const int* cu_q_len, const int* cu_k_off, const int* k_len, int batch, int max_q_len,
                         int q_heads, int kv_heads, float softmax_scale, tm_stream_t st);
/* The same for head_dim 64 or 128 (q heads at h*head_dim, k [kv_heads][k_stride][head_dim], vt [kv_heads][head_dim][k_stride]);
 * softmax_scale <= 0 -> 1/sqrt(head_dim).  tm_prefill_attention is the head_dim = 128 case. */
int tm_prefill_attention_hd(void* out, const void* q, int q_stride, const void* k, const void* vt, int k_stride,
                            const int* cu_q_len, const int* cu_k_off, const int* k_len, int batch, int max_q_len,
                            int q_heads, int kv_heads, int head_dim, float softmax_scale, tm_stream_t st);
/* tm_prefill_attention_hd with a sliding window and attention sinks (attention_params.h:55-72; the per-row mask
 * 0 <= q_pos - k_pos < window_size of mainloop_sm80.h:558-566; tile skip attention_universal.h:411,474-480; sink term :529-535):
 * the row at absolute position q sees the keys t with 0 <= q - t < window; key steps no row of a workgroup sees are skipped.
 * sinks as in tm_decode_attention_window.  window == 0 && sinks == NULL is tm_prefill_attention_hd, bit for bit; window < 0:
 * TM_INVALID. */
int tm_prefill_attention_window(void* out, const void* q, int q_stride, const void* k, const void* vt, int k_stride,
                                const int* cu_q_len, const int* cu_k_off, const int* k_len, int batch, int max_q_len,
                                int q_heads, int kv_heads, int head_dim, float softmax_scale, int window, const void* sinks,
                                tm_stream_t st);

int tm_embedding(void* out, const void* table, const int* ids, int tokens, int hidden, int vocab, tm_stream_t st);
/* tm_embedding for multimodal prompts (the reference's input_embeddings / input_embedding_ranges, lmdeploy/turbomind/turbomind.py:632-674):
 * emb_index device int [tokens]; row t is row emb_index[t] of emb_rows (device fp16 [n][hidden], copied bit for bit, ids[t] is not
 * read) when emb_index[t] >= 0, the table row of ids[t] when it is -1.  All -1 is tm_embedding. */
int tm_embedding_mixed(void* out, const void* table, const int* ids, const void* emb_rows, const int* emb_index, int tokens, int hidden,
                       int vocab, tm_stream_t st);
/* greedy top-1 on fp32-cast logits (generation/sampling.cc:92-183); out_val (fp16 [batch]) may be NULL */
int tm_argmax(int* out_ids, void* out_val, const void* logits, int batch, int vocab, int ld, tm_stream_t st);
/* Per-row cross-entropy (kernels/cross_entropy_kernels.cu:31-73): nll fp32 [rows] = logf(sum_v exp(x_v - max) + 1e-9f) + max
 * - x[targets[r]] over fp16 logits [rows][ld] of `vocab` columns, in fp32 from the raw logits (max starts at -FLT_MAX: a row of
 * -inf gives +inf).  targets (device int32 [rows]) < 0: nll = 0 and the row is not read; >= vocab: NaN.  One pass, fixed
 * reduction order, no atomics: bitwise reproducible.  rows == 0 is a no-op. */
int tm_cross_entropy(float* nll, const void* logits, const int* targets, int rows, int vocab, int ld, tm_stream_t st);
/* Stochastic sampling (generation/sampling.cc:92-183, logits_processor.cc:105-112, kernels/sampling_*.cu): per row
 * logits / temperature -> keep the top_k most probable (top_k <= 0: all) -> softmax -> keep the shortest prefix whose
 * cumulative probability exceeds top_p (>= 1: all) -> drop p < min_p * p_max -> renormalise -> first candidate whose
 * inclusive prefix sum exceeds uniform[b] (in [0,1)).  Candidates are ordered by descending probability, ties by
 * ascending token id.  Per-row device arrays temperature / top_k / top_p / min_p may be NULL (1, all, 1, 0).
 * kept_out (device int[batch], may be NULL) receives the number of surviving candidates.  workspace:
 * tm_sample_workspace(batch) bytes, ZERO on first use (every call leaves it zero again). */
size_t tm_sample_workspace(int batch);
int    tm_sample(int* out_ids, int* kept_out, const void* logits, int batch, int vocab, int ld, const float* temperature,
                 const int* top_k, const float* top_p, const float* min_p, const float* uniform, void* workspace,
                 tm_stream_t st);
/* tm_sample + the logprobs of the kept candidates (the `sampled_logprobs / sampled_indexes / sampled_nums` outputs of
 * invokeSampling, kernels/sampling_kernels.cu:67-90, which generation/sampling.cc:173-178 arms when a request asks for
 * output_logprobs): per row the first min(kept, cap) candidates in sampling order -- idx [batch][cap] token ids, vals [batch][cap]
 * logf of their renormalised probability (-inf for zero-probability candidates), num [batch] their count -- and sel [batch], the
 * drawn token's own logprob.  cap = TM_MAX_LOGPROBS reproduces the reference's layout: a drawn token beyond the first 1024
 * candidates replaces entry 1023.  Smaller caps keep the first cap candidates untouched (the drawn token's logprob is in sel).
 * All arrays are device memory; kept_out is required. */
#define TM_MAX_LOGPROBS 1024
int    tm_sample_logprobs(int* out_ids, int* kept_out, float* vals, int* idx, int* num, float* sel, int cap, const void* logits,
                          int batch, int vocab, int ld, const float* temperature, const int* top_k, const float* top_p,
                          const float* min_p, const float* uniform, void* workspace, tm_stream_t st);
/* the engine's uniform draw: Philox4x32-10, key = request seed, counter = context length -> [0, 1) (host function) */
float  tm_philox_uniform(uint64_t seed, uint32_t counter);

/* Logits processors ahead of arg-max / sampling: repetition penalty -> bad ids -> min-length ban of the end ids
 * (LogitsProcessor::Forward, generation/logits_processor.cc:66-115; kernels/sampling_penalty_kernels.cu:137-215,
 * kernels/ban_bad_words.cu:51-95 single-token case).  In place on fp16 logits [batch][ld] (columns vocab_offset ..
 * vocab_offset + vocab of the global vocabulary; ld and vocab_offset multiples of 8):
 *   seen     device u32 [batch][seen_words]: bit id%32 of word id/32 set = token id occurs in the sequence (prompt +
 *            generated); maintained with tm_seen_update (the reference rebuilds it from token_ids_ptrs every step)
 *   rep      device float [batch]  repetition penalty (1 = off): seen ids get l < 0 ? l*p : l/p
 *   ban      device int [batch][TM_MAX_BAD_IDS]  ids that get -65504 (-1 = unused; ids <= 0 are skipped, as upstream)
 *   end      device int [batch][1 + TM_MAX_STOP_IDS]  eos / stop ids, banned while k_len + 1 < min_len (ids <= 0 skipped)
 *   k_len    device int [batch]  context length of this forward; min_len = prompt length + min_new_tokens
 * The fp32 result is rounded to fp16 once (the reference keeps fp32 logits from here on).
 * tm_seen_update: OR the tokens ids[0..n_tokens) into the masks; cu_q NULL: token t belongs to row t (decode),
 * else rows are the packed prefill sequences cu_q[r] .. cu_q[r+1]. */
#define TM_MAX_BAD_IDS 32
#define TM_MAX_STOP_IDS 8
int tm_seen_update(void* seen, int seen_words, const int* ids, const int* cu_q, int nseq, int n_tokens, int vocab,
                   tm_stream_t st);
int tm_logits_process(void* logits, int batch, int vocab, int ld, int vocab_offset, const void* seen, int seen_words,
                      const float* rep, const int* ban, const int* end, const int* k_len, const int* min_len,
                      tm_stream_t st);
/* unfused activation on [M][2*inter] laid out [gate | up]            (kernels/activation.cu:27-130) */
int tm_silu_mul(void* out, const void* gate_up, int M, int inter, tm_stream_t st);

/* ---- Linear (mirrors _tm.LinearWeight / LlamaLinear.forward_dense / QuantizeGroupwise) -------- */
typedef struct tm_linear tm_linear;
enum { TM_WEIGHT_U4 = 0, TM_WEIGHT_F16 = 1, TM_WEIGHT_FP8 = 2, TM_WEIGHT_MXFP4 = 3 /* experts weight-only (tm_moe); dense linears W4A4 (tm_linear_prepare_mxfp4) */,
       TM_WEIGHT_I8 = 4 /* dense linears W8A8 (tm_linear_prepare_int8); never experts */ };
int tm_linear_create(tm_linear** out, int in_features, int out_features, int weight_type, int group_size);
/* TM_WEIGHT_U4 comes in two group sizes.  group_size 128: the AWQ / GPTQ / compressed-tensors g128 form on the decode, prefill and
 * general kernels.  group_size 32 (compressed-tensors pack-quantized g32): a format of its own on gemm_u4_g32.hip
 * (v_mfma_f32_32x32x16_f16; K % 128 == 0, N % 32 == 0, image K N / 2 + K N / 8 bytes below 2^31) -- the same three parts with scales /
 * zeros [K/32][N], the same arithmetic w = h(fma(h(q), s, h(-z*s))), fp32 accumulation, one rounding.  Its tm_linear_forward picks its
 * own tile (nt = waves = 0; M <= 32 / <= 64 / 128-row tiles) and takes `splits` (0 = its heuristic, evened out over the k-blocks);
 * a split launch is reduced before the call returns, so y always holds the finished fp16 result, and tm_linear_residual_norm / the
 * folded-norm entries refuse such a handle.  tm_linear_dequant_f16 reads its image back.  Any other u4 group_size is refused here by
 * name (before: accepted here, refused by tm_linear_prepare); tm_moe_create has no group parameter (experts: 128), and an engine with
 * group_size 32 and moe_experts > 0 is refused at creation. */
/* Boundary ("TM") layout, device pointers: qweight int32 [K][N/8] (nibble j of word c = column 8c+j,
 * lmdeploy/turbomind/weight_format.py:63-74), scales / zeros fp16 [K/g][N].  For TM_WEIGHT_F16: weight fp16
 * [K][N], scales = zeros = NULL.  For TM_WEIGHT_FP8 (lmdeploy/turbomind/weight_format.py:349-393): weight = e4m3 bytes
 * [K][N], scales = fp32 128x128 block scales [K/128][ceil(N/128)] (`weight_scale_inv`, transposed like the weight),
 * zeros = NULL; w = fp16(e4m3) * fp16(scale), one rounding (the pre-sm90 weight-only path, linear_weight.cc:138-150).
 * Performs LinearWeight::prepare (repack to MFMA-fragment order, fuse (s,-z*s)). */
int tm_linear_prepare(tm_linear* w, const void* weight, const void* scales, const void* zeros, tm_stream_t st);
/* y fp16 [M][N] (or [M][N/2] when gated_silu: columns interleaved (gate_j, up_j), epilogue.h:159-176).
 * nt / splits / waves: 0 = heuristic.  waves per workgroup: 4 or 8; waves | 0x100 additionally splits K two ways
 * inside the workgroup (8 waves).  workspace >= tm_linear_workspace() bytes when split-K may be used. */
size_t tm_linear_workspace(const tm_linear* w, int M);
int    tm_linear_forward(const tm_linear* w, const void* x, int ldx, void* y, int ldy, int M, int gated_silu,
                         int nt, int splits, int waves, void* workspace, tm_stream_t st);
/* tm_linear_dequant_f16: the fp16 image [N][K] of the weights, bit for bit the operand the W4A16 kernels build on chip
 * (w = h(fma(h(q), s, h(-z*s))), kernels/gemm/transform.h:34-74) -- what the reference's own tests call quant_vs_dequant
 * (tests/turbomind/linear/fixture.py:404-507).  (Round 3 also exported tm_f16_library_available / tm_linear_build_f16_image:
 * prefill-sized forwards through a vendor fp16 GEMM on that image -- removed in round 4, every GEMM of this library is its own.) */
int    tm_linear_dequant_f16(const tm_linear* w, void* out_nk, tm_stream_t st);
/* Row-parallel linear closed by residual + RMSNorm -- wo / w2 of a decoder layer at the decode batch: LlamaLinear::Forward
 * followed by invokeResidualBiasRMSNorm (src/turbomind/models/llama/unified_decoder.cc:149,226; kernels/norm/rms_norm.cu:286-362):
 *   resid += fp16(x . W);  y = RMSNorm(resid) * norm_w.
 * The GEMM (fp32 split-K slabs when it splits), then the reduce-norm kernel.
 * shape: decode tile 0..3 / 6..9 / 11, -1 = dispatch; splits: 0 = dispatch.  workspace >= tm_linear_workspace(w, M) + M * N * 2 bytes.
 * (Round 3's in-launch consumer behind a `fused` flag was removed in round 4; its two dead parameters left the signature in round 5.) */
int    tm_linear_residual_norm(const tm_linear* w, const void* x, int ldx, void* y, void* resid, const void* norm_w, float eps, int M,
                               int shape, int splits, void* workspace, tm_stream_t st);
/* The same pair of operators with the RMSNorm FOLDED into the two GEMMs around it (round 5; the engine's decode step at tp = 1):
 *   RMSNorm(r) . W2 = inv[m] * sum_k (r[m,k] g[k]) W2[k,n],   inv[m] = 1 / sqrt(sum_k r[m,k]^2 / H + eps)
 * tm_linear_fold_produce -- the row-parallel linear (wo / w2): resid += fp16(x . W) in the GEMM's own epilogue (bit-identical to
 *   tm_linear_residual_norm's residual stream, split-K included: the last-arriving slice of a column tile sums the slices' fp32 slabs in
 *   slice order), xg = fp16(f32(resid) * f32(norm_w)) (saturating), ss[tile][m] = sum of f32(resid)^2 over the tile's columns;
 *   *ss_tiles = tiles written (<= N / 64).  ss holds (N / 64) * M floats; workspace >= tm_linear_fold_workspace(w, M).
 * tm_linear_fold_consume -- the linear fed with xg: y = [gated SiLU](inv[m] * (xg . W)); norm_h = H of the folded norm.
 * Replaces invokeResidualBiasRMSNorm + the following LlamaLinear::Forward (unified_decoder.cc:226,278,328; rms_norm.cu:286-362;
 * epilogue.h:159-176): two launches instead of three; the normalised activations carry ONE fp16 rounding (r * g) instead of two and
 * the row factor is applied to fp32 accumulators -- tests/test_gpu_ops.py::test_w4a16_folded_norm states the bound next to the
 * unfused sequence's.  shape: decode tile 0..3 / 6..9, -1 = dispatch; splits: 0 = dispatch. */
size_t tm_linear_fold_workspace(const tm_linear* w, int M);
int    tm_linear_fold_produce(const tm_linear* w, const void* x, int ldx, void* xg, void* resid, const void* norm_w, float* ss,
                              int* ss_tiles, int M, int shape, int splits, void* workspace, tm_stream_t st);
int    tm_linear_fold_consume(const tm_linear* w, const void* xg, int ldx, void* y, int ldy, int M, int gated_silu, const float* ss,
                              int ss_tiles, int norm_h, float eps, int shape, int splits, void* workspace, tm_stream_t st);
/* FP8 x FP8 linear on the fp8 matrix cores -- the reference's path for e4m3 weights on fp8 tensor cores:
 * LlamaLinear::Forward quantises the activations per row and 128-channel group (QuantizeSymm,
 * src/turbomind/kernels/quantization.cu:28-125, called at models/llama/LlamaLinear.cu:67-93) and runs the fp8 GEMM with
 * both scale sets.  tm_quant_fp8_rows = QuantizeSymm (codes [M][K] e4m3, scales fp32 [K/128][ldsx]);
 * tm_linear_forward_fp8 = quantise + GEMM (+ split-K reduce); workspace >= tm_linear_fp8_workspace(w, M) bytes. */
/* the fused w1w3 linear of an fp8 checkpoint: (gate_j, up_j)-interleaved e4m3 columns whose block-scale row is
 * [w1's inter/128 blocks | w3's inter/128 blocks] (w1 / w3 are quantised separately; lmdeploy/turbomind/builders/ffn.py:31-34) */
int    tm_linear_prepare_fp8_gated(tm_linear* w, const void* weight, const void* scales, tm_stream_t st);
/* Channel-scaled e4m3 weights (per-tensor and per-channel FP8 checkpoints): codes [K][N] with ONE fp32 scale per output column,
 * scales = device fp32 [N] (a per-tensor scale is that scalar repeated; fused linears concatenate / interleave their parts' scales
 * like their columns); N % 32 == 0.  Activations are quantised per token over the whole row (tm_quant_fp8_token: codes [M][K],
 * sx fp32 [M]; absmax clamped to 1e-8, sx = absmax / 448, q = e4m3_rne_sat(x * (448 / absmax)); K % 128 == 0, K <= 32768), and
 *   y[m, n] = h( (sx[m] * sw[n]) * sum_k xq[m, k] * wq[k, n] )
 * with the sum chained in fp32 on the matrix core over all of K and the scale product applied once, in the epilogue (split-K slabs
 * are written scaled).  tm_linear_forward_fp8 / tm_linear_fp8_workspace serve a weight prepared this way; tm_linear_forward does not
 * (there is no weight-only image: its fp16 (s, 0) scales would push small per-tensor scales into fp16 subnormals), and
 * TM_FP8_MFMA=0 makes the preparation return TM_INVALID. */
int    tm_linear_prepare_fp8_channel(tm_linear* w, const void* weight, const void* scales_f32_N, tm_stream_t st);
int    tm_quant_fp8_token(void* xq, float* sx, const void* x, int ldx, int M, int K, tm_stream_t st);
/* The grouped (mixture-of-experts) form of tm_linear_forward_fp8 on its own: `experts` = host array of E handles of one shape and
 * one scale mode; flat output rows seg[e] .. seg[e + 1] (device int32 [E + 1]) belong to expert e and read row row_idx[f] of x
 * (device int32, NULL: f itself); x fp16 [x_rows][K] is quantised first (per token for channel-scaled experts); m_cap = upper bound
 * of an expert's rows.  workspace >= tm_linear_fp8_grouped_workspace(E, x_rows, K) bytes.  Synchronises the stream once. */
size_t tm_linear_fp8_grouped_workspace(int experts, int x_rows, int K);
int    tm_linear_forward_fp8_grouped(const tm_linear* const* experts, int E, const void* x, int ldx, int x_rows, void* y, int ldy,
                                     int m_cap, int gated_silu, const int* seg, const int* row_idx, void* workspace, tm_stream_t st);
/* MXFP4 dense linears, FP4 weights and FP4 activations ("W4A4") on the block-scaled FP4 matrix cores
 * (v_mfma_scale_f32_32x32x64_f8f6f4).  tm_linear_create(..., TM_WEIGHT_MXFP4, 32); limits: K % 128 == 0, N % 32 == 0, K * N / 2 < 2^31.
 * Weights arrive in the checkpoint layout of the gpt-oss experts: blocks uint8 [N][K/2] (byte j of row n = k 2j in the low nibble, 2j + 1
 * in the high nibble; e2m1 code c & 7 -> {0, .5, 1, 1.5, 2, 3, 4, 6}, bit 3 = sign) and scales uint8 [N][K/32] (e8m0: 2^(b - 127), 255 is
 * never accepted).  Activations are quantised on the fly per row and group of 32 k (tm_quant_mxfp4_rows: codes [M][K/2] in the same
 * nibble order, scale bytes [M][K/32]): e = floor(log2(amax)) - 2 (-127 for a zero group), byte e + 127, code = e2m1_rne_sat(x / 2^e)
 * with ties to the even mantissa, saturation to 6 and the sign of zero kept (the OCP MX v1.0 rule), and
 *   y[m, n] = h( sum_g 2^(sx[m,g] - 127) 2^(sw[n,g] - 127) sum_{k in g} xq[m,k] wq[n,k] )
 * with the whole sum chained in fp32 on the matrix core, both scale bytes operands of the instruction.  gated_silu as tm_linear_forward
 * ((gate_j, up_j)-interleaved columns, y [M][N/2]); splits = 0: heuristic, else 1..16 split-K slices through fp32 slabs.
 * tm_linear_forward_mxfp4 quantises, runs the GEMM and reduces; workspace >= tm_linear_mxfp4_workspace(w, M) bytes.
 * tm_linear_dequant_f16 on such a weight writes the fp16 [N][K] image lut[code] * 2^(s - 127) rebuilt from the repacked units;
 * tm_linear_forward returns TM_INVALID: there is no weight-only arm. */
int    tm_linear_prepare_mxfp4(tm_linear* w, const void* blocks, const void* scales, tm_stream_t st);
int    tm_quant_mxfp4_rows(void* xq, void* sx, const void* x, int ldx, int M, int K, tm_stream_t st);
size_t tm_linear_mxfp4_workspace(const tm_linear* w, int M);
int    tm_linear_forward_mxfp4(const tm_linear* w, const void* x, int ldx, void* y, int ldy, int M, int gated_silu, int splits,
                               void* workspace, tm_stream_t st);
/* INT8 dense linears, int8 weights and int8 activations ("W8A8") on the int8 matrix cores (v_mfma_i32_32x32x32_i8): the form
 * `lmdeploy lite smooth_quant` writes and compressed-tensors publishes as "int-quantized".  tm_linear_create(..., TM_WEIGHT_I8, 128);
 * limits: K % 128 == 0, K <= 32768, N % 32 == 0.  weight = int8 codes [K][N], scales = device fp32 [N], one per output column (a
 * per-tensor scale is that scalar repeated; fused linears concatenate / interleave their parts' scales like their columns).
 * Activations are quantised per token over the whole row (tm_quant_int8_token: codes int8 [M][K], sx fp32 [M]; K % 128 == 0,
 * K <= 32768), per fp16 row in fp32: absmax = max(max|x|, 1e-7), sx = absmax / 127, q = clamp(round(x / sx), -127, 127) with the
 * IEEE division and ties rounded away from zero (the reference's per_token_quant_int8), and
 *   y[m, n] = h( (float(acc) * sx[m]) * sw[n] ),   acc = sum_k xq[m, k] * wq[k, n]  in int32 over ALL of K (exact),
 * float() rounding to nearest even.  gated_silu as tm_linear_forward; splits = 0: heuristic, else 1..16 split-K slices whose raw int32
 * accumulators are summed as integers before the one conversion: y is the same bits for every split.
 * tm_linear_forward_int8 quantises, runs the GEMM and reduces; workspace >= tm_linear_int8_workspace(w, M) bytes.
 * tm_linear_forward returns TM_INVALID on such a handle: there is no weight-only arm. */
int    tm_linear_prepare_int8(tm_linear* w, const void* weight, const void* scales_f32_N, tm_stream_t st);
int    tm_quant_int8_token(void* xq, float* sx, const void* x, int ldx, int M, int K, tm_stream_t st);
size_t tm_linear_int8_workspace(const tm_linear* w, int M);
int    tm_linear_forward_int8(const tm_linear* w, const void* x, int ldx, void* y, int ldy, int M, int gated_silu, int splits,
                              void* workspace, tm_stream_t st);
size_t tm_linear_fp8_workspace(const tm_linear* w, int M);
int    tm_quant_fp8_rows(void* xq, float* sx, const void* x, int ldx, int M, int K, int ldsx, tm_stream_t st);
int    tm_linear_forward_fp8(const tm_linear* w, const void* x, int ldx, void* y, int ldy, int M, int gated_silu, int splits,
                             void* workspace, tm_stream_t st);
int    tm_linear_destroy(tm_linear* w);
/* ---- Mixture-of-experts FFN block (MoeFfnLayer, models/llama/moe_ffn_layer.cc:43-53,133-325; routing
 * kernels/gemm/moe_utils_v2.cu:355-690; grouped linear LlamaLinear.cu:67-127) -------------------------------------
 * out[t] = sum over the top_k experts e of token t of w_e(t) * W2_e( silu(W1_e x_t) * (W3_e x_t) ), with
 * logits = x Wg (fp32), top-k on the logits (ties: lower expert id), w = softmax over the selected experts
 * (norm_topk != 0) or over all experts, times routed_scale.  Expert weights: weight_type TM_WEIGHT_U4 / TM_WEIGHT_FP8 /
 * TM_WEIGHT_F16, boundary layouts of tm_linear_prepare; w13 = [hidden][2*inter] with (gate_j, up_j) column-interleaved, w2 =
 * [inter][hidden].  TM_WEIGHT_F16: the weights are fp16 [K][N], scales = zeros = NULL, and the forward has no activation-quantisation
 * stage.  FP8 w13: w1 and w3 are block-quantised separately in a checkpoint, so the scale row of w13 is
 * [w1's inter/128 blocks | w3's inter/128 blocks] (inter % 128 == 0) -- also for the engine's *.w1w3.scales slots.  gate: fp16 [hidden][experts].  All pointers device.  topk_ids_out / topk_w_out (device
 * [tokens][top_k], may be NULL) expose the routing for tests.
 * Bounds: 1 <= top_k <= 8, top_k <= experts <= 256 (Mixtral 8 / 2, Qwen3-MoE 128 / 8).  Up to 64 experts the router is the serial
 * one written for Mixtral; above, or for every count with TM_MOE_ROUTER=wide, the wide one (hidden % 128 == 0).  Both fill the
 * same tables.  experts x ceil(tokens / 64) must stay within 65535 (the grouped GEMMs' grid.z).
 * tm_moe_router runs the router alone (gate + top-k + routing tables): logits_out fp32 [tokens][experts] (may be NULL),
 * offsets int32 [experts + 1], f2n int32 [tokens * top_k] (flat row -> token), en2f int32 [top_k][tokens] (choice j of token t ->
 * flat row); the tokens of an expert are in ascending order.
 * tm_moe_forward_stages enqueues a subset of tm_moe_forward's launches (bits: gate + top-k 1, routing tables 2, grouped w1w3 with its
 * activation quantisation 4, grouped w2 8, combine 16; 31 = tm_moe_forward) on what an earlier forward of the same x and tokens
 * left in `workspace`: the measurement tool times the launches one by one with it.
 * Shared expert (Qwen2-MoE: the layer has a routed MoE AND a dense feed_forward, the shared expert, whose output the combine scales per
 * token by a sigmoid gate before the routed experts are added -- models/llama/unified_decoder.cc:295-318, moe_ffn_layer.cc:295-325,
 * invokeMoeCombine kernels/gemm/moe_utils_v2.cu:1032-1105; weights lmdeploy/turbomind/models/qwen2.py:110-128):
 * tm_moe_set_shared_gate copies the gate vector (device fp16 [hidden]) into the block; from then on the block is run by
 * tm_moe_forward_shared, whose `shared` (device fp16 [tokens][hidden]) is the shared expert's FFN output for the same x:
 *   out[t] = fp16( float(shared[t]) * sigmoid(x_t . gate) + sum_e w_e(t) * float(y_e(t)) )
 * with the logit and the sum in fp32, in ONE combine launch.  `shared` may equal `out` (the reference combines in place); x must not.
 * tm_moe_forward / tm_moe_forward_stages on such a block return TM_INVALID instead of dropping the term;
 * tm_moe_forward_shared_stages is tm_moe_forward_stages for it (`shared` is read by the combine stage only).
 * MXFP4 experts and the gpt-oss block (lmdeploy/turbomind/models/gpt_oss.py; src/turbomind/kernels/activation.cu:17-24,
 * kernels/gemm/transform.h:83-90, kernels/gemm/cast.cu:220-227, models/llama/moe_ffn_layer.cc:43-53,272-275,310-313):
 * weight_type TM_WEIGHT_MXFP4: tm_moe_set_expert takes the checkpoint layout -- weight = blocks uint8 [N][K/2] (N = output channels,
 * the low nibble of a byte is the even k) and scales = uint8 [N][K/32] (one ue8m0 byte per 32 k), zeros unused (NULL); w13's N rows are
 * (gate_j, up_j)-interleaved.  Code c is sign c >> 3 and magnitude {0, .5, 1, 1.5, 2, 3, 4, 6}[c & 7]; scale byte s is the fp16 with
 * exponent field clamp(s - 112, 0, 30); w = fp16(value * scale), exact when finite; from there on the arithmetic of fp16 experts.
 * tm_mxfp4_dequant_f16 writes that operand, as the grouped GEMM builds it from the repacked image, to out_kn fp16 [K][N].
 * tm_moe_set_activation: 0 = SiLU (default), 1 = gpt-oss: g = min(g, 7), u = clamp(u, -7, 7), g * sigmoid(1.702 g) * (1 + u) in fp32 on
 * the fp16-rounded (and biased) gate / up.  tm_moe_set_gate_bias: device fp32 [experts], added to the router logits before the top-k (NULL: none again; any expert format).
 * tm_moe_set_expert_bias: device fp16 b13 [2 * inter] ((gate_j, up_j)-interleaved, added in fp16 to the w1w3 output before the
 * activation; needs activation 1) and b2 [hidden] (added in fp16 to every routed row of that expert before the weighted combine);
 * experts never given a bias have zero biases.  The activation and the biases are built for TM_WEIGHT_F16 and TM_WEIGHT_MXFP4 experts;
 * the setters return TM_INVALID for u4 / fp8 blocks, and blocks that never call them launch exactly what they launched before. */
typedef struct tm_moe tm_moe;
int    tm_moe_create(tm_moe** out, int hidden, int inter, int experts, int top_k, int weight_type, int norm_topk,
                     float routed_scale);
int    tm_moe_set_gate(tm_moe* m, const void* gate, tm_stream_t st);
int    tm_moe_set_shared_gate(tm_moe* m, const void* gate_fp16_hidden, tm_stream_t st);
int    tm_moe_set_expert(tm_moe* m, int expert, const void* w13_weight, const void* w13_scales, const void* w13_zeros,
                         const void* w2_weight, const void* w2_scales, const void* w2_zeros, tm_stream_t st);
int    tm_moe_set_activation(tm_moe* m, int kind);
/* fp8 experts: 0 = 128 x 128 block scales (default), 1 = channel (tm_linear_prepare_fp8_channel's form).  One call per block, before
 * the first tm_moe_set_expert, whose scales arguments are then fp32 [2 * inter] ((gate_j, up_j)-interleaved like the columns) and
 * [hidden]; x is quantised per token and the gated-SiLU output per (token, expert) row. */
int    tm_moe_set_fp8_scale_mode(tm_moe* m, int mode);
int    tm_moe_set_gate_bias(tm_moe* m, const void* bias_fp32_experts, tm_stream_t st);
int    tm_moe_set_expert_bias(tm_moe* m, int expert, const void* b13_fp16, const void* b2_fp16, tm_stream_t st);
int    tm_mxfp4_dequant_f16(void* out_kn, const void* blocks, const void* scales, int K, int N, tm_stream_t st);
size_t tm_moe_workspace(const tm_moe* m, int tokens);
int    tm_moe_forward(tm_moe* m, void* out, const void* x, int tokens, void* workspace, int* topk_ids_out, float* topk_w_out,
                      tm_stream_t st);
int    tm_moe_forward_stages(tm_moe* m, void* out, const void* x, int tokens, void* workspace, unsigned stages, tm_stream_t st);
int    tm_moe_forward_shared(tm_moe* m, void* out, const void* x, const void* shared, int tokens, void* workspace, int* topk_ids_out,
                             float* topk_w_out, tm_stream_t st);
int    tm_moe_forward_shared_stages(tm_moe* m, void* out, const void* x, const void* shared, int tokens, void* workspace,
                                    int* topk_ids_out, float* topk_w_out, unsigned stages, tm_stream_t st);
int    tm_moe_router(tm_moe* m, const void* x, int tokens, int* topk_ids, float* topk_w, float* logits_out, int* offsets, int* f2n,
                     int* en2f, tm_stream_t st);
int    tm_moe_destroy(tm_moe* m);

/* IntegralQuantizer<half,4> (kernels/quantization.cu:384-440): w fp16 [K][N] -> qweight int32 [K][N/8],
 * scales/zeros fp16 [K/g][N], dequant fp16 [K][N] (may be NULL).  Groups run along K. */
int tm_quantize_groupwise(void* qweight, void* scales, void* zeros, void* dequant, const void* w, int K, int N,
                          int group_size, tm_stream_t st);

/* ---- native point-to-point communicator (the reference's comm/cuda_ipc backend; RCCL stays the default) ----------------
 * Fused one-shot all-reduce + residual + RMSNorm over peer-mapped segments: replaces AllreduceResidualBiasRMSnorm
 * (src/turbomind/comm/cuda_ipc/fused_allreduce.cu:406-500, exchange as in allreduce.cu:249-343) and, for the lm_head's
 * (value, index) candidates, AllGather (comm/cuda_ipc/allgather.cu).  Every rank owns a symmetric segment of
 * tm_p2p_segment_bytes(rows, H) bytes -- [256 B of flags | tile 0 | tile 1], a tile = rows x H fp16 -- that its peers
 * map: tm_p2p_segment_create allocates it (zeroed) and returns a 64-byte IPC handle, tm_p2p_segment_open maps a peer's
 * handle (another PROCESS: one process per GPU), tm_p2p_segment_close unmaps (opened = 1) or frees (opened = 0).
 * segs[r] = rank r's segment as seen from this rank (segs[me] = the local one); state = 4 zeroed local words (the rank's call
 * counter and tickets).  Every rank must issue the same sequence of tm_p2p_* calls.
 * tm_p2p_allreduce_norm: y = RMSNorm(resid += fp16(sum_r partial_r)), M <= rows; rank-ordered fp32 sum, so every rank
 * holds the same bits.  tm_p2p_allgather: dst[r][0..words) = rank r's src (32-bit words, words * 4 <= tile bytes).
 * A rank that waits longer than ~1 s for a peer gives up, writes the call number into state[3] and returns garbage. */
size_t tm_p2p_segment_bytes(int rows, int H);
int tm_p2p_segment_create(size_t bytes, void** dev_ptr, void* handle64);
int tm_p2p_segment_open(const void* handle64, void** dev_ptr);
int tm_p2p_segment_close(void* dev_ptr, int opened);
int tm_p2p_allreduce_norm(void* const* segs, int tp, int me, void* state, int rows, const void* partial, void* y, void* resid,
                          const void* weight, float eps, int M, int H, tm_stream_t st);
int tm_p2p_allgather(void* const* segs, int tp, int me, void* state, int rows, int H, const void* src, void* dst, int words,
                     tm_stream_t st);
/* Two-shot form for large messages -- AllreduceResidualBiasRMSnorm_Simple_Push / _Pull and the two-shot all-reduce of the reference
 * (src/turbomind/comm/cuda_ipc/fused_allreduce.cu:25-405, allreduce.cu:22-248): reduce-scatter (rank r sums rows
 * [r * slice, (r + 1) * slice), slice = ceil(M / tp), of all ranks' partials in rank order), residual + RMSNorm on the owned slice,
 * all-gather of the normed rows by pushing them into every peer's segment: (tp - 1) / tp of one message read and written per rank
 * instead of (tp - 1) messages read.  y: all M normed rows (the bits of the one-shot form); resid: updated for the rank's OWN
 * slice only (the reference shards the residual stream the same way).  Segments of tm_p2p_segment_bytes2(rows, rows2, H) bytes =
 * [256 B flags | one-shot tile 0 | tile 1 (rows x H each) | in2 | out2 (rows2 x H each)], M <= rows2; shares `state` and the call
 * sequence with the one-shot calls (it advances the epoch by two). */
size_t tm_p2p_segment_bytes2(int rows, int rows2, int H);
/* One-shot form whose workgroups do not wait for each other (round 6): one workgroup owns a token row end to end -- its own call counter
 * (state[4 + row]), write-through system-scope stores of its partial row, ONE flag word per (sender, row) in every peer's segment, system-
 * scope loads of the peers' rows -- no tickets, no shared epoch, no residency requirement, no L2 write-back / invalidate on the path; same
 * arithmetic and bits as tm_p2p_allreduce_norm.  Segments of tm_p2p_segment_bytes_rows(rows, rows2, H) bytes = the two-shot layout followed
 * by [row tile 0 | row tile 1 (rows x H each) | flags [8][rows]]; state = 4 + rows zeroed local words; M <= rows.  Its calls are
 * independent of the shared call sequence of the other tm_p2p_* entry points (own tiles, own flags).  This is what the engine's decode-sized
 * exchanges run (fused_allreduce.cu:406-500 called at unified_decoder.cc:278-285,328-335). */
size_t tm_p2p_segment_bytes_rows(int rows, int rows2, int H);
int tm_p2p_allreduce_norm_rows(void* const* segs, int tp, int me, void* state, int rows, int rows2, const void* partial, void* y, void* resid,
                               const void* weight, float eps, int M, int H, tm_stream_t st);
int tm_p2p_allreduce_norm_2shot(void* const* segs, int tp, int me, void* state, int rows, int rows2, const void* partial, void* y,
                                void* resid, const void* weight, float eps, int M, int H, tm_stream_t st);

/* debug / measurement: device buffer of 8192 x 8 uint64 (512 KB) that receives s_memrealtime stamps (100 MHz: kernel
 * entry, loop entry, loop exit, exit, ...) of every GEMM / decode-attention workgroup launched afterwards; launches of more
 * than 8192 workgroups are not traced; NULL switches it off. */
int tm_debug_set_gemm_trace(void* dev_buf);
/* Arena form of the same trace (round 5, tools/fixed_cost_table.py): every traced launch (decode GEMMs, decode attention, the
 * norm kernels) is given ITS OWN region of `dev_buf` (capacity_workgroups x 8 uint64), in launch order -- so the launches of a
 * captured hipGraph keep distinct regions and one replay leaves the stamps of every kernel of the decode step.  Slots per
 * workgroup: 0 entry, 5 prologue loads issued, 1 activations landed (first stage barrier), 6 wave 0's first weight unit landed,
 * 2 loop exit, 7 k-phase merge barrier, 3 stores drained, 4 (XCC id << 32 | HW_ID); attention: 1 prologue done, 2 / 6 / 7
 * waves 0 / 1 / 3 done, 5 all waves done.  NULL switches it off and forgets the records.
 * tm_debug_trace_records: text, one line per traced launch `index tag grid.x grid.y grid.z offset_in_workgroups`; returns the
 * bytes the text needs.  Host-side bookkeeping is not thread-safe against concurrent LAUNCHES from other engines. */
int     tm_debug_trace_arena(void* dev_buf, int64_t capacity_workgroups);
int64_t tm_debug_trace_records(char* host_out, int64_t cap);
/* Host-only: the (workgroup shape, split-K) the decode GEMM dispatch picks for a W4A16 linear of K x N at M rows --
 * use_table bit 0: the measured table first (tm_engine_tune_gemm / tm_gemm_import), then the heuristic; clear: heuristic only;
 * bits 8 .. 11: the linear's role -- 0 any, 1 w_qkv, 2 wo, 3 w1w3, 4 w2 (the table is keyed (role, K, N, M): the tuner times each
 * role with its own consumer kernel; an entry of role 0, e.g. an imported line without a role column, serves every role).
 * Shapes: 0..3 decode tiles (M <= 64), 4 / 5 the 128-row tiles (M > 64), 6..9 shapes 3, 0, 2, 1 on 32-row blocks
 * (gemm_decode.hip), 11 the loader / consumer decode kernel (gemm_decode_lc.hip, M <= 64), 12 the 256 x 256 prefill tile with
 * the weights dequantised once per workgroup tile through LDS (gemm_prefill.hip, M > 64).  (10 was a vendor-library path: gone.) */
int tm_debug_pick_tiling(int K, int N, int M, int use_table, int* shape, int* splits);
/* Host-only: the tiling of the general kernel (gemm_w4a16.hip: the fp16 lm_head, e4m3 weight-only linears, u4 with N % 32 != 0)
 * for a K x N linear of `weight_type` (TM_WEIGHT_*) and `role` (0 any, 1 w_qkv, 2 wo, 3 w1w3, 4 w2, 5 lm_head) at M rows:
 * config4 = {tiles per wave, split-K, waves, k-phases} -- the measured entry (tm_engine_tune_gemm / tm_gemm_import, `G` lines)
 * first, then the heuristic.  Reference: the same DispatchCache serves every GEMM of the model (gemm.cu:92-224). */
int tm_debug_pick_general(int weight_type, int role, int K, int N, int M, int* config4);
/* Host-only: the measured row-tile height of the grouped expert GEMMs (u4 and fp16: 16 / 32 / 64, e4m3 on the fp8 matrix cores: 32 / 64)
 * for `tokens` rows per forward; *rows = 0: no entry, the launcher's own rule (twice the expected rows per expert) applies. */
int tm_debug_grouped_tile(int weight_type, int K, int N, int tokens, int* rows);
/* Host-only: every (shape, splits) pair the start-up tuner (tm_engine_tune_gemm; gemm::Gemm::Run's dispatch candidates,
 * src/turbomind/kernels/gemm/gemm.cu:92-224) may pick for a K x N linear at M rows; *count = how many exist (<= 128), the first
 * min(cap, *count) are written.  The full-size parity tests sweep exactly this list. */
int tm_debug_tiling_candidates(int K, int N, int M, int* shapes, int* splits, int cap, int* count);
/* Host-only: every (tiles per wave, split-K) pair the start-up tuner times for a dense linear of the general kernel (gemm_w4a16.hip:
 * the fp16 lm_head, TM_WEIGHT_F16, and e4m3 weight-only linears, TM_WEIGHT_FP8) of K x N at M rows with a split-K workspace of
 * `workspace_bytes` -- exactly gen_dense_candidates (the tuner adds the heuristic's own pick when it is not in the list).  *count =
 * how many exist (0 for other weight types and M > 256), the first min(cap, *count) are written.  The general-kernel parity tests
 * sweep exactly this list. */
int tm_debug_general_candidates(int weight_type, int K, int N, int M, int64_t workspace_bytes, int* nt, int* splits, int cap,
                                int* count);
/* Operator-level calls that follow treat tm_kv_cache::block_ptrs as a rectangular table: sequence b starts at b * stride
 * (cu_block_nums must say the same); 0 = ragged (default).  The engine's own table is rectangular and always takes this
 * path: the decode kernel then needs no dependent pointer loads (test hook for that path). */
int tm_debug_set_block_stride(int stride);
/* Grouped expert GEMMs launched by the CALLING thread (tm_moe_forward) use `rows`-row tiles: u4 / fp16 / fp8 weight-only 16, 32 or
 * 64 (decode-sized forwards, tokens <= 64), e4m3 on the fp8 matrix cores 32 or 64 (any size); 0 = off, the measured entry or
 * the launcher's own rule (test hook: every row tile against the oracle, whatever the routing). */
int tm_debug_set_grouped_rows(int rows);
/* Router of the MoE block for this process: -1 = what TM_MOE_ROUTER says (auto | wide), 0 = auto, 1 = wide.  Not thread-safe (a
 * plain global that every launch reads): for tests and the benchmark tool only, set while no thread enqueues a forward. */
int tm_debug_set_moe_router(int mode);

/* ----------------------------------------------------------------------------------------------
 * Engine level (static batcher around LanguageModel::Forward)
 * --------------------------------------------------------------------------------------------*/
typedef struct tm_model_config {
    /* head_dim: 64 or 128; q_heads / tp * head_dim must be a multiple of 128.  head_dim 64 decodes on the VALU attention kernel behind
     * tm_kv_rope_store (no fused prologue) for every quant_policy; qk_norm needs head_dim 128. */
    int   hidden, layers, q_heads, kv_heads, head_dim, inter, vocab;
    float rms_eps;
    float rope_base;
    int   rope_type; /* 0 default, 1 linear, 2 llama3, 3 yarn, 4 dynamic (tm_rope_param) */
    float rope_factor, rope_low_freq_factor, rope_high_freq_factor;
    int   rope_original_max_position;
    /* yarn: the correction range's length; dynamic: prompts longer than this take a base of their own (an engine whose session_len
     * does not exceed it runs exactly as rope_type 0) */
    int   rope_max_position_embeddings;
    float rope_yarn_beta_fast, rope_yarn_beta_slow, rope_yarn_attention_factor;
    int   group_size;   /* 128; u4 weights: 128 or -- dense models, gemm_u4_g32.hip -- 32 */
    int   weight_type;  /* TM_WEIGHT_U4 (AWQ), TM_WEIGHT_F16, TM_WEIGHT_FP8, TM_WEIGHT_MXFP4 or TM_WEIGHT_I8 for the decoder linears; lm_head is fp16.
                         * TM_WEIGHT_MXFP4 (W4A4, tm_linear_prepare_mxfp4's form): dense models at tp = 1, any head_dim the engine serves;
                         * slots "*.blocks" uint8 [N][K/2] and "*.scales" uint8 [N][K/32] for w_qkv (q | k | v rows stacked), wo, w1w3
                         * ((gate_j, up_j) rows interleaved) and w2; every such linear runs tm_quant_mxfp4_rows + the block-scaled FP4 MFMA
                         * GEMM for every M, eager and in the decode graph; the GEMM tuner and the folded norm pass them by; refused
                         * with TM_INVALID: tp > 1, moe_experts > 0, hidden_valid (padded widths).
                         * TM_WEIGHT_I8 (W8A8, tm_linear_prepare_int8's form): dense models; slots "*.weight" int8 [K][N] and "*.scales"
                         * fp32 [N] for the four decoder linears; each runs tm_quant_int8_token + the int8 MFMA GEMM for every M and
                         * reduces its own split-K; refused with TM_INVALID: moe_experts > 0, hidden_valid (padded widths) */
    /* mixture of experts (0 experts = dense FFN): every layer's FFN is a router + `moe_experts` expert FFNs of width
     * `inter` (sharded over tp like the dense FFN), `moe_top_k` per token (Mixtral: 8 / 2, norm_topk = 1) */
    int   moe_experts, moe_top_k, moe_norm_topk;
    float moe_routed_scale;
    /* gpt-oss MoE block (all 0 = the engine as before).  moe_expert_format: 0 = the experts follow weight_type, 3 = TM_WEIGHT_MXFP4
     * experts whatever the other linears are (gpt-oss: fp16 attention, MXFP4 experts) in the slots "layers.{i}.moe_ffn.experts.{x}.
     * w1w3.blocks" uint8 [2 * inter][hidden / 2] / ".w1w3.scales" uint8 [2 * inter][hidden / 32] / ".w2.blocks" uint8 [hidden][inter / 2] /
     * ".w2.scales" uint8 [hidden][inter / 32] (tm_moe_set_expert's layout).  moe_act: tm_moe_set_activation's kind.  moe_bias != 0 ->
     * slots "...experts.{x}.w1w3.bias" fp16 [2 * inter], "...experts.{x}.w2.bias" fp16 [hidden] and "layers.{i}.moe_ffn.gate.bias" fp32
     * [experts]; needs moe_act 1.  moe_act / moe_bias need fp16 or MXFP4 experts; MXFP4 experts and moe_bias need tp == 1 (the w2 bias
     * would need a per-rank rule). */
    int   moe_expert_format, moe_act, moe_bias;
    /* Qwen2-MoE shared expert (0 = none; needs moe_experts > 0): every MoE layer ALSO has a dense FFN of this width (sharded over tp like
     * the dense FFN; moe_shared_inter / tp % 128 == 0) in the slots "layers.{i}.feed_forward.w1w3.*" / ".w2.*" -- the reference's names:
     * the shared expert is the layer's feed_forward -- and a gate "layers.{i}.moe_ffn.shared_gate.weight" fp16 [hidden], replicated.
     * FFN output = sigmoid(x . gate) * feed_forward(x) + the routed experts (tm_moe_forward_shared). */
    int   moe_shared_inter;
    /* Sliding-window attention and attention sinks (AttentionParams::window_size / ::sinks, kernels/attention/attention_params.h:55-72).
     * attn_window: the window of every layer, 0 = none (tm_engine_set_layer_windows overrides it per layer); a window >= session_len is
     * full attention.  attn_sinks != 0 -> slot "layers.{i}.attention.sinks" fp16 [q_heads / tp], one natural-log logit per local head.
     * An engine with a windowed layer or sinks decodes like head_dim 64: tm_kv_rope_store + the VALU attention kernel, no fused
     * prologue, no folded norm.  KV blocks older than the window stay allocated. */
    int   attn_window, attn_sinks;
    /* gpt-oss (all three: tp == 1, no folded norm).
     * attn_out_bias != 0 -> slot "layers.{i}.attention.wo.bias" fp16 [hidden], added behind the o projection in the order of the
     * reference's invokeResidualBiasRMSNorm: r = h(h(r + wo_out) + bias), in every layer.
     * hidden_valid (0 = hidden): the model's true hidden size when `hidden` (and `inter`) are the zero-padded sizes the engine runs at
     * -- the loader pads every tensor with +0 (MXFP4: code 0) up to the next multiple of 128 -- so that the RMSNorms divide by it and
     * keep the pad columns of the residual stream at +0 (tm_rmsnorm_valid).
     * rope_yarn_truncate: tm_rope_param::yarn_truncate (1 = the reference's rounded correction range, 0 = fractional). */
    int   attn_out_bias, hidden_valid, rope_yarn_truncate;
    /* weight_type TM_WEIGHT_FP8 only (0 = the engine as before): 0 = 128 x 128 block scales, slots "*.scales" fp32
     * [K / 128][ceil(N / 128)]; 1 = channel (per-tensor and per-channel FP8 checkpoints): slots "*.scales" fp32 [N], one scale per output
     * column -- a per-tensor scale repeated over its columns, the scales of fused linears (q | k | v, (gate_j, up_j)-interleaved w1w3,
     * experts alike) concatenated / interleaved like their columns.  Every dense decoder linear and every expert then runs
     * tm_quant_fp8_token + the channel-scaled fp8 x fp8 GEMM (tm_linear_prepare_fp8_channel) for every M; lm_head and embeddings stay
     * fp16; the folded norm and the dense GEMM tuner pass these linears by; TM_FP8_MFMA=0 is refused when the weights are prepared. */
    int   fp8_scale_mode;
    /* Qwen attention prologue (0 = off): attn_bias -> slot "layers.{i}.attention.w_qkv.bias" fp16 [local qkv columns] added to
     * q / k / v (Qwen2); qk_norm -> slots "layers.{i}.attention.{q,k}_norm.weight" fp16 [head_dim], per-head RMSNorm of q / k with
     * rms_eps (Qwen3).  Order: norm -> bias -> RoPE. */
    int   attn_bias, qk_norm;
} tm_model_config;

typedef struct tm_engine_config {
    tm_model_config model;
    int   tp;                 /* tensor-parallel world size (one process per GPU)            */
    int   rank;               /* this process' rank                                          */
    int   device;             /* HIP device ordinal                                          */
    int   max_batch_size;     /* TurbomindEngineConfig.max_batch_size                        */
    int   session_len;        /* max context per sequence                                    */
    int   quant_policy;       /* 0 | 4 | 8 | 42 (lmdeploy/messages.py:20-27); 42 = TurboQuant KV: head_dim 128, no window / sinks, tp 1 */
    int   cache_block_seq_len;/* 64                                                          */
    float cache_max_entry_count; /* fraction of free HBM for KV blocks if cache_blocks == 0 */
    int   cache_blocks;       /* explicit number of KV blocks (0 = derive)                   */
    int   max_prefill_token_num; /* tokens per prefill iteration (messages.py:334: 8192)    */
    int   decode_splits;      /* 0 = heuristic                                               */
    int   use_graph;          /* capture the decode step in a hipGraph                       */
} tm_engine_config;

typedef struct tm_engine tm_engine;

int tm_engine_create(tm_engine** out, const tm_engine_config* cfg);
/* after tm_engine_start: *per_seq_tables = 1 when the engine keeps one RoPE table region per batch slot behind the shared one
 * (rope_type 4 with rope_factor > 1 and session_len > rope_max_position_embeddings), *table_bytes = bytes of those regions (0 without) */
int tm_engine_rope_info(tm_engine* e, int* per_seq_tables, int64_t* table_bytes);
/* after tm_engine_start: *ring_blocks = the KV block ring of a sequence (0: no ring -- a layer without a window, a ring that would
 * not be shorter than ceil(session_len / 64), or TM_KV_RING=0), *free_blocks = blocks of the pool that no sequence owns right now
 * (the scheduler's count while a continuous-batching session is open; its parking block is neither free nor owned).
 * TM_CONFLICT while the engine thread runs. */
int tm_engine_kv_info(tm_engine* e, int* ring_blocks, int64_t* free_blocks);
int tm_engine_destroy(tm_engine* e);
/* Per-layer sliding windows (gpt-oss alternates sliding and full layers): window[i] replaces attn_window for layer i, 0 = full
 * attention.  Before tm_engine_start; layers must equal the model's; a negative window is TM_INVALID. */
int tm_engine_set_layer_windows(tm_engine* e, const int* window, int layers);
/* Multimodal RoPE sections (Qwen2-VL / Qwen2.5-VL mrope_section): a setter like tm_engine_set_layer_windows rather than three more ints
 * in struct tm_model_config -- a choice, not a constraint (every caller that fills the struct positionally stays as it is).  Frequency pair j of a head rotates by the t coordinate for j < sec_t, by h for the next sec_h
 * pairs, by w for the rest (tm_kv_rope_store_mrope).  Before tm_engine_start.  0 / 0 / 0 = none (the engine as created); otherwise
 * three non-negative sizes that sum to head_dim / 2, head_dim 128, rope_type 0 .. 3 (one shared table) -- TM_INVALID by name else.
 * Such an engine (tp 1, quant_policy != 42) accepts coordinates and a position delta in tm_engine_set_multimodal and decodes every
 * static batch with a per-slot delta array (zeros for text): the fused prologue's pos_delta for int8 / int4 KV, tm_kv_rope_store_mrope
 * otherwise.  Without multimodal input it computes what the engine without sections computes, bit for bit. */
int tm_engine_set_mrope_section(tm_engine* e, int sec_t, int sec_h, int sec_w);
/* RCCL bootstrap for tp > 1: rank 0 calls tm_comm_unique_id (128 bytes, host), broadcasts it out of band
 * (torch.distributed / TCPStore), then every rank calls tm_engine_comm_init. */
int tm_comm_unique_id(void* host_out128);
int tm_engine_comm_init(tm_engine* e, const void* host_id128);
/* native communicator (opt-in; see tm_p2p_* below): export = allocate this rank's segment, return its IPC handle; import =
 * map the tp ranks' handles (rank order) and route the row-parallel all-reduces of forwards with <= rows tokens through it */
int tm_engine_comm_drop_rccl(tm_engine* e);   /* continue on the native communicator alone (every rank must call it) */
int tm_engine_comm_native_export(tm_engine* e, int rows, void* handle64);              /* after tm_engine_comm_init */
int tm_engine_comm_native_import(tm_engine* e, const void* handles, int count);        /* count = tp handles, rank order */
/* Collective bring-up check of the native communicator (every rank, right after the import): two fused launches over a known pattern;
 * *ok = 0 -> every rank calls tm_engine_comm_native_drop and the decode-sized exchanges stay on RCCL + the residual-norm launch.  The
 * hop between devices (system-scope visibility over xGMI) is what no single-GPU test exercises; the default tensor-parallel arrangement
 * -- native fused all-reduce + residual + RMSNorm for decode-sized forwards (the reference's AllreduceResidualBiasRMSnorm,
 * src/turbomind/comm/cuda_ipc/fused_allreduce.cu:406-500, called at unified_decoder.cc:278-285,328-335), RCCL for prefill-sized ones --
 * is taken only when it passed on every rank. */
int tm_engine_comm_native_selftest(tm_engine* e, int* ok);
int tm_engine_comm_native_drop(tm_engine* e);

/* Weight hand-off: named Param slots, already TP-sharded / QKV-fused / w1w3-interleaved by the loader
 * (lmdeploy/turbomind/builders/_base.py:72-113).  Names: "layers.{i}.attention.w_qkv.{qweight,scales,zeros}",
 * "layers.{i}.attention.wo.*", "layers.{i}.feed_forward.w1w3.*", "layers.{i}.feed_forward.w2.*"
 * (".weight" instead for fp16 linears), "layers.{i}.attention_norm.weight", "layers.{i}.ffn_norm.weight",
 * "tok_embeddings.weight", "norm.weight", "output.weight".
 * tm_engine_weight_bytes: expected byte size of a slot (0 + TM_INVALID for unknown names).
 * tm_engine_weight_copy : host -> device staging copy; byte size must match exactly. */
int64_t tm_engine_weight_bytes(tm_engine* e, const char* name);
int     tm_engine_weight_copy(tm_engine* e, const char* name, const void* host_src, int64_t bytes);
/* Device-side synthetic init (random weights with the real shapes): N(0,1)*0.1/sqrt(K) fp16
 * master -> group-128 asymmetric u4; norms 1+0.02N; embeddings 0.02N.  For benchmarks without checkpoints. */
int     tm_engine_init_synthetic(tm_engine* e, uint64_t seed);
/* ModelRoot::prepare(): repack every linear, free staging */
int     tm_engine_process_weights(tm_engine* e);
/* allocate KV pool + activation buffers, build RoPE table (TurboMind::CreateEngine) */
int     tm_engine_start(tm_engine* e);

/* Static batch.  Admit `batch` sequences (host token ids, concatenated; host lens), run chunked prefill and
 * produce the first token of every sequence.  Each sequence reserves ceil((len + max_new_tokens)/64) blocks. */
int tm_engine_prefill(tm_engine* e, const int* host_ids, const int* host_lens, int batch, int max_new_tokens);
/* run `steps` decode iterations for the admitted batch (every sequence generates one token per step,
 * ignore_eos semantics).  Asynchronous on the engine stream; tm_engine_sync() waits. */
int tm_engine_decode(tm_engine* e, int steps);
/* Speculative decoding by prompt lookup (n-gram drafting) for a static batch of greedy sequences: a step verifies k drafted tokens per
 * sequence in ONE forward over batch * (k + 1) rows and emits 1 .. k + 1 tokens per sequence -- the tokens plain greedy decoding emits.
 * tm_engine_set_speculative: before tm_engine_prefill (after tm_engine_start); k = 0 switches it off, 1 <= k <= 7, 1 <= ngram_min <=
 *   ngram_max <= 8.  Armed, tm_engine_prefill reserves k tokens of KV slack per sequence (prompt + max_new_tokens + k <= session_len):
 *   the rows behind the accepted ones are computed, stored and never read -- the next step overwrites them.
 * tm_engine_decode_spec: `steps` steps of propose (from the device token history) -> verify forward -> accept; asynchronous.  The
 *   forward is the prefill-shaped one (plain w_qkv, K/V store, then tm_verify_attention's kernel for int8 / int4 KV at head_dim 128,
 *   flatten + prefill attention otherwise), the lm_head over every row, arg-max.  With use_graph the step is captured as one linear
 *   chain after an eager first step (the flatten + prefill-attention path stays eager: it needs host-side maximum lengths).
 * tm_engine_verify: one step with the caller's drafts (host_drafts [batch][k] ids in [0, vocab), host_n_draft [batch] in [0, k]) in
 *   place of the proposer: where a draft model plugs in.  Synchronous.
 * tm_engine_fetch_spec: host_tokens [batch][max_new_tokens], host_counts [batch] tokens emitted per sequence (the prefill's first
 *   token included); tokens of a sequence stop at max_new_tokens (ignore_eos semantics: the host cuts at stop ids).
 * tm_engine_fetch_spec_logits: logits of the last step's rows, fp16 [batch][k + 1][vocab] (row j: the distribution behind input row j).
 * tm_engine_spec_stats: (sequence-steps that emitted, drafted, accepted, emitted) since tm_engine_set_speculative; emitted = accepted +
 *   sequence-steps.
 * Refused with TM_INVALID by name: tp > 1, quant_policy 42, a layer with a sliding window or sinks, M-RoPE sections, multimodal input,
 * sampling / logits processors / logprobs armed for the batch, a continuous-batching session while k > 0 (tm_engine_submit*,
 * tm_engine_step*, tm_engine_serve_start), tm_engine_decode on a batch admitted with k > 0 after a speculative step. */
int tm_engine_set_speculative(tm_engine* e, int k, int ngram_max, int ngram_min);
int tm_engine_decode_spec(tm_engine* e, int steps);
int tm_engine_verify(tm_engine* e, const int* host_drafts, const int* host_n_draft);
int tm_engine_fetch_spec(tm_engine* e, int* host_tokens, int* host_counts);
int tm_engine_fetch_spec_logits(tm_engine* e, void* host_out);
int tm_engine_spec_stats(tm_engine* e, int64_t* host_stats);
/* Prompt scoring (Pipeline.get_ppl; the reference's return_ppl path, models/output_processor.cc:236-300).  Synchronous.
 * `batch` sequences (host ids concatenated, host lens) run through chunked prefill with the lm_head over EVERY prompt row and
 * per-row cross-entropy against the next token, from the raw logits (no penalties, bans or sampling).  host_nll receives
 * sum(len_b - 1) floats: sequence by sequence, position p scored against ids[b][p + 1].  Each sequence holds ceil(len / 64)
 * blocks (at most its block ring, tm_engine_kv_info) for the call only; on return every block is free again and the engine is idle (batch slots, next ids, logits and
 * the decode graph untouched; the scoring scratch stays allocated until tm_engine_destroy).  Refusals:
 * TM_CONFLICT (engine thread running), TM_INVALID (a batch admitted / scheduler session open, tp > 1, len < 2, an id
 * outside [0, vocab)), TM_TOO_LONG (len >= session_len), TM_OOM (not enough free KV blocks). */
int tm_engine_score(tm_engine* e, const int* host_ids, const int* host_lens, int batch, float* host_nll);
int tm_engine_sync(tm_engine* e);
/* per-sequence time-to-first-token of the last tm_engine_prefill, milliseconds since the call started (host [batch]) */
int tm_engine_prefill_times(tm_engine* e, float* host_ms);
/* Run `steps` EAGER decode steps with HIP events around every kernel category on the engine stream and return the
 * mean milliseconds per step per category (host float[TM_PROF_NUM]) and launches per step (host int[TM_PROF_NUM],
 * may be NULL).  Categories: */
enum {
    TM_PROF_EMBED = 0, TM_PROF_GEMM_QKV, TM_PROF_KV_STORE, TM_PROF_ATTN, TM_PROF_GEMM_O, TM_PROF_RES_NORM,
    TM_PROF_GEMM_GATE_UP, TM_PROF_GEMM_DOWN, TM_PROF_LM_HEAD, TM_PROF_SAMPLE, TM_PROF_ALLREDUCE, TM_PROF_NUM
};
int tm_engine_profile_decode(tm_engine* e, int steps, float* host_ms_per_step, int* host_launches_per_step);
/* copy generated tokens so far to host: out [batch][max_new_tokens] int32 (row-major), n_generated (host) */
int tm_engine_fetch(tm_engine* e, int* host_out, int* n_generated);
/* last step's logits of the local vocab shard, fp16 [batch][vocab/tp] -> host (debug / parity tests) */
int tm_engine_fetch_logits(tm_engine* e, void* host_out);
/* parity tests: intermediate state of the last forward -> host.  what = 0: the residual stream, fp16 [a rows][hidden]
 * (UnifiedDecoder's residual buffer, models/llama/unified_decoder.cc:226-330); what = 1: the bytes of KV block b of
 * static-batch sequence a, all layers (block layout = kernels/attention/block.h:126-219); what = 2: int64 count of
 * continuous-batching steps whose decode rows shared a forward with an admission's prefill.  `bytes` must match exactly. */
int tm_engine_debug_read(tm_engine* e, int what, int a, int b, void* host_out, int64_t bytes);
/* Per-sequence sampling parameters (GenerationConfig: temperature, top_k, top_p, min_p, random_seed;
 * lmdeploy/messages.py:35-205).  top_k == 1 is greedy.  The uniform draw of a step is Philox(seed, context length). */
typedef struct tm_sampling {
    float    temperature; /* > 0 */
    int      top_k;       /* <= 0: no top-k filter */
    float    top_p;       /* >= 1: no top-p filter */
    float    min_p;       /* 0: off */
    uint64_t seed;
} tm_sampling;
/* Static batch: sampling parameters of the NEXT tm_engine_prefill (host array [batch], copied); NULL / never called =
 * greedy arg-max.  Cleared by tm_engine_release.  TP > 1 (RCCL communicator): the vocabulary shards of the logits
 * are all-gathered and every rank draws the same token from the full row (models/language_model.cc:304-333 gathers the
 * logits as well) -- over RCCL, or through the native P2P segments when no RCCL communicator exists. */
int tm_engine_set_sampling(tm_engine* e, const tm_sampling* host_params, int batch);
/* Static batch: the NEXT tm_engine_prefill records, for every generated token of every sequence, the first n (1 .. TM_MAX_LOGPROBS;
 * 0 = off) kept candidates with their logprobs and the drawn token's own logprob -- GenerationConfig.logprobs, i.e. the request's
 * output_logprobs of generation/sampling.cc:173-178,229-279 seen through lmdeploy/turbomind/turbomind.py:472-503.  The draw then runs
 * through the sampling kernels (greedy sequences as top_k = 1 rows: one kept candidate with logprob 0, as upstream).  Cleared by
 * tm_engine_release.  tm_engine_fetch_logprobs copies the records to the host: vals / idx [batch][max_new_tokens][n] (entries beyond
 * num are undefined), num / sel [batch][max_new_tokens] (columns beyond the generated steps: num = 0). */
int tm_engine_set_logprobs(tm_engine* e, int n);
/* Multimodal input of ONE sequence of a static batch (the reference's input_embeddings, input_embedding_ranges, mrope_position_ids and
 * mrope_position_delta: lmdeploy/turbomind/turbomind.py:632-674).  Host pointers, copied by tm_engine_set_multimodal. */
typedef struct tm_mm_input {
    int         prompt_len;     /* tokens of this sequence's prompt, as tm_engine_prefill will get it */
    const void* emb_rows;       /* fp16 [n_rows][hidden]: the rows that replace the token-table lookup, in prompt order (NULL: none) */
    int         n_rows;
    const int*  ranges;         /* [n_ranges][2]: [begin, end) in prompt coordinates, sorted, disjoint, lengths summing to n_rows */
    int         n_ranges;
    const int*  mrope_pos;      /* [n_pos][3]: (t, h, w) of the first n_pos prompt tokens, all >= 0 (NULL / 0: none) */
    int         n_pos;          /* <= prompt_len */
    int         position_delta; /* every later token (rest of the prompt, decode) sits at linear position + delta on all axes; >= -prompt_len */
} tm_mm_input;
/* Static batch: multimodal inputs of the NEXT tm_engine_prefill (host array [batch], one entry per sequence, copied), which must have
 * the same batch and prompt lengths and consumes them -- also when it fails, for whatever reason: nothing stays armed behind a
 * tm_engine_prefill call; NULL clears.  A prompt row inside a range takes its fp16 row from emb_rows, bit
 * for bit, and its token id is not read.  Coordinates and a non-zero delta need a model with sections (tm_engine_set_mrope_section).  Chunked prompts continue
 * across prefill iterations; decode steps use the delta.  tm_engine_release or the next prefill clears the state.  TM_INVALID with the
 * reason in tm_last_error: ranges unsorted, overlapping, outside the prompt or not summing to n_rows; n_pos > prompt_len; a negative
 * coordinate; position_delta < -prompt_len; coordinates or a non-zero delta on a model without sections; tp > 1; quant_policy 42.
 * Continuous batching (tm_engine_submit*) and tm_engine_score do not take multimodal input. */
int tm_engine_set_multimodal(tm_engine* e, const tm_mm_input* host, int batch);
/* Continuous batching: the same records for ONE queued request (call right after its submit, before the next scheduler step): every
 * token the request generates from then on carries its first n kept candidates.  tm_engine_poll_logprobs copies the records of the
 * first min(max_tokens, generated) tokens: vals / idx [tokens][n] (entries beyond num[t]: 0 / -1), num / sel [tokens]; *n_tokens =
 * tokens recorded, *n_per_token = n (0: the request did not ask).  The arrays may be NULL to query the counts.  While any request with
 * logprobs is in the session the decode step does not ride on prefill forwards (no mixed steps). */
int tm_engine_request_logprobs(tm_engine* e, int64_t req_id, int n);
int tm_engine_poll_logprobs(tm_engine* e, int64_t req_id, float* host_vals, int* host_idx, int* host_num, float* host_sel, int max_tokens,
                            int* n_tokens, int* n_per_token);
int tm_engine_fetch_logprobs(tm_engine* e, float* host_vals, int* host_idx, int* host_num, float* host_sel);
/* Per-sequence logits processors (GenerationConfig: repetition_penalty, min_new_tokens, bad_token_ids,
 * stop_token_ids; applied in the reference's order, see tm_logits_process).  stop ids end a sequence of the
 * continuous-batching path like its eos id and are banned with it until min_new_tokens tokens exist; the static
 * batch has no engine-side stop (the caller cuts), there they only matter for min_new_tokens. */
typedef struct tm_logits_param {
    float repetition_penalty; /* > 0; 1 = off */
    int   min_new_tokens;     /* 0 = off */
    int   n_bad_ids;
    int   bad_ids[TM_MAX_BAD_IDS];
    int   n_stop_ids;
    int   stop_ids[TM_MAX_STOP_IDS];
} tm_logits_param;
/* Static batch: parameters of the NEXT tm_engine_prefill (host array [batch], copied); NULL = none.  Cleared by
 * tm_engine_release.  Works with tp > 1 (each rank processes its vocabulary shard). */
int tm_engine_set_logits_params(tm_engine* e, const tm_logits_param* host_params, int batch);

/* release the batch (blocks return to the pool); also ends a continuous-batching session */
int tm_engine_release(tm_engine* e);
/* Measured GEMM dispatch (the reference's warm-up tuning, turbomind.cc:363-487 / kernels/gemm/gemm.cu:92-224): time every
 * (workgroup shape, split-K) candidate of the W4A16 kernels for the model's w_qkv / wo / w1w3 / w2 at M rows -- M <= 256: a decode
 * batch, keyed by the exact M; M = 512, 1024, 2048, 4096, 8192 (<= max_prefill_token_num): the size class of prefill forwards
 * with up to M tokens -- as a hipGraph over the engine's own layer weights, each GEMM followed by the kernel that consumes it,
 * and remember the winner per (K, N, M).  After tm_engine_start, before the first batch.  export_path (may be NULL): write the table as text lines
 * "K N M shape splits".  Environment equivalents read by tm_engine_start: TM_GEMM_TUNE=1 (M = max_batch_size),
 * TM_GEMM_EXPORT=<file>, TM_GEMM_IMPORT=<file>; TM_GEMM_TUNE_VERBOSE=1 prints every measurement to stderr. */
int tm_engine_tune_gemm(tm_engine* e, int M, const char* export_path);
int tm_gemm_import(const char* path);
/* write the process's measured dispatch tables (P32 lines + `G` lines) without an engine: what rank 0 hands to the other ranks */
int tm_gemm_export(const char* path);


/* ----------------------------------------------------------------------------------------------
 * Continuous batching.  Replaces ModelRequest.forward / cancel + the engine thread's
 * schedule-forward-update loop (bind.cpp:743-793, engine/engine.cc:434-470,770-870, model_request.cc:36-135):
 * requests are queued, admitted in arrival order when a batch slot and enough KV blocks (prompt + max_new_tokens,
 * 64-token blocks; at most the block ring of a sliding-window model, tm_engine_kv_info) are free, prefilled (chunked, <= max_prefill_token_num prompt tokens per step) and then decoded
 * together with everything else that is running; a sequence ends on eos_id (eos_id < 0: ignore_eos), at
 * max_new_tokens or on cancel, and its slot / blocks are reused by the next admission.  Greedy sampling.
 * The first tm_engine_submit switches the engine into this mode (no static batch may be admitted);
 * tm_engine_release leaves it.  The caller drives the loop: one tm_engine_step = admissions + ONE decode step.
 * submit: 0 queued | TM_INVALID (empty prompt, max_new_tokens < 1) | TM_TOO_LONG (> session_len) |
 *         TM_OOM (can never fit the block pool).  poll: status 0 = waiting / running, TM_FINISH, TM_CANCEL;
 *         copies min(cap, n_tokens) generated tokens.  Unknown ids: TM_INVALID. */
int tm_engine_submit(tm_engine* e, const int* host_ids, int n, int max_new_tokens, int eos_id, int64_t* req_id);
/* like tm_engine_submit with sampling parameters (NULL = greedy) */
int tm_engine_submit_ex(tm_engine* e, const int* host_ids, int n, int max_new_tokens, int eos_id, const tm_sampling* sampling,
                         int64_t* req_id);
/* ... and logits-processor parameters (NULL = none) */
int tm_engine_submit_gen(tm_engine* e, const int* host_ids, int n, int max_new_tokens, int eos_id, const tm_sampling* sampling,
                         const tm_logits_param* logits_param, int64_t* req_id);
int tm_engine_step(tm_engine* e, int* n_active, int* n_waiting);
/* tm_engine_step_many: up to max_steps iterations of tm_engine_step in one call (stops when nothing runs and nothing waits); *steps_done =
 * iterations executed.  What a tensor-parallel rank group mirrors to its ranks instead of single steps -- the per-rank engine loops of
 * src/turbomind/engine/engine.cc:770-870 exchange admissions, not steps -- and the cheaper host loop at tp = 1 (one poll per burst). */
int tm_engine_step_many(tm_engine* e, int max_steps, int* steps_done, int* n_active, int* n_waiting);
int tm_engine_poll(tm_engine* e, int64_t req_id, int* status, int* host_tokens, int cap, int* n_tokens);
int tm_engine_cancel(tm_engine* e, int64_t req_id);
/* drop the record of a FINISHED request (status != 0) once its tokens were read: a long-lived serving session would
 * otherwise keep every prompt / output until tm_engine_release.  TM_INVALID: unknown id or still queued / running. */
int tm_engine_forget(tm_engine* e, int64_t req_id);

/* Engine thread (the reference's Engine::Impl::InternalThreadEntry, engine/engine.cc:770-870, + the Gateway signal
 * thread that runs the Python callback, bind.cpp:942-952).  After tm_engine_serve_start an engine-owned thread runs
 * the schedule -> forward -> update loop whenever a request is queued or running, and sleeps otherwise;
 * submit / submit_ex / poll / cancel / wait may then be called from ANY thread (they are serialised against the loop by
 * the engine's mutex; without the loop they are serialised against each other the same way).  tm_engine_step returns
 * TM_CONFLICT while the loop runs.  `on_update` (may be NULL) is called ON THE ENGINE THREAD, outside the engine lock,
 * after every scheduler step, once per token produced in that step (a newly admitted request gets its first token
 * from the prefill and its second from the decode pass of the same step), with the request's status at that token
 * (0 = streaming, TM_FINISH) and its number of generated tokens so far; it is never called again for a request
 * after a non-zero status (the reference's callback contract, turbomind.py:808-812).  It may call poll / submit / cancel.
 * A device error inside the loop ends every unfinished request with TM_FAIL, stops the loop and is reported by
 * tm_engine_serve_stop (return code + tm_last_error).  serve_stop joins the thread; requests that are still queued or
 * running stay where they are (a later serve_start or tm_engine_step continues them). */
typedef void (*tm_request_cb)(void* user, int64_t req_id, int status, int n_tokens);
int tm_engine_serve_start(tm_engine* e, tm_request_cb on_update, void* user);
int tm_engine_serve_stop(tm_engine* e);
/* block until request req_id has more than `have_tokens` generated tokens or a non-zero status, or until timeout_ms
 * elapsed (timeout_ms < 0: no timeout); returns the poll result.  Needs the engine thread (TM_INVALID otherwise). */
int tm_engine_wait(tm_engine* e, int64_t req_id, int have_tokens, int timeout_ms, int* status, int* n_tokens);

/* The scheduler by itself (host-only bookkeeping: queue, slots, block accounting) -- what the engine embeds,
 * exported so that its policy is testable without a GPU (engine/scheduler.cc:1018-1078 at the level used here). */
/* Host-only, exported for the CPU tests like the scheduler below: where a tensor-parallel prefill forward of nseq sequences (row offsets
 * cu_q[0 .. nseq], cu_q[0] = 0) splits into the two micro-batches whose all-reduces overlap the other one's kernels (DESIGN.md 6;
 * no reference counterpart: the reference hides the exchange in a fused kernel, comm/cuda_ipc/fused_allreduce.cu:406-500).
 * *seqs_a = sequences of the first micro-batch, *rows_a = its rows; 0 / 0: no usable boundary (fewer than two sequences, or the smaller side
 * below min_rows / 2 rows) -- the engine then splits the row-wise part of every layer by rows instead. */
int tm_prefill_split(const int* cu_q, int nseq, int min_rows, int* seqs_a, int* rows_a);
/* Host-only: the KV block ring of a model whose every layer has a sliding window.  *ring_blocks =
 * ceil((window - 1 + chunk_tokens) / 64) + 1, window = the largest layer window, chunk_tokens = the most tokens one sequence
 * contributes to one prefill forward (the engine: max(max_batch_size, 64, max_prefill_token_num)).  A sequence then owns
 * min(ceil((prompt + max_new_tokens) / 64), ring_blocks) blocks and its logical block i is its physical block i % ring_blocks. */
int tm_kv_ring_blocks(int window, int chunk_tokens, int* ring_blocks);
typedef struct tm_sched tm_sched;
int tm_sched_create(tm_sched** out, int max_batch, int num_blocks, int session_len);
/* block ring: every request owns at most ring_blocks blocks (0 = off, whole contexts are reserved: the default).  The never-fits
 * test of tm_sched_submit, tm_sched_admit and tm_sched_admit_ready count with it; tm_sched_query's n_blocks is what the request
 * owns.  Before the first tm_sched_submit only, TM_INVALID afterwards.  The engine sets it when it creates its scheduler. */
int tm_sched_set_ring(tm_sched* s, int ring_blocks);
int tm_sched_destroy(tm_sched* s);
int tm_sched_submit(tm_sched* s, const int* ids, int n, int max_new_tokens, int eos_id, int64_t* req_id);
/* admit waiting requests for one step: writes up to cap (request id, slot) pairs */
int tm_sched_admit(tm_sched* s, int token_budget, int64_t* req_ids, int* slots, int cap, int* n_admitted);
/* *ready = 1 if tm_sched_admit would admit at least one request right now (no side effects): the engine asks before it keeps a
 * decode step in flight across scheduler steps (two-phase schedule / forward overlap, turbomind.cc:171) */
int tm_sched_admit_ready(tm_sched* s, int* ready);
int tm_sched_on_token(tm_sched* s, int slot, int token, int* finished);
int tm_sched_cancel(tm_sched* s, int64_t req_id, int* released_slot);
/* status (Request::k*), slot (-1 unless running), tokens generated, blocks held; TM_INVALID for unknown ids */
int tm_sched_query(tm_sched* s, int64_t req_id, int* status, int* slot, int* n_generated, int* n_blocks);
int tm_sched_counts(tm_sched* s, int* n_active, int* n_waiting, int* n_free_blocks);
/* every unfinished request ends with `status` (the engine uses TM_FAIL after a device error) */
int tm_sched_abort_all(tm_sched* s, int status);
/* forget a finished request; TM_INVALID for unknown / unfinished ids */
int tm_sched_forget(tm_sched* s, int64_t req_id);
/* the engine's stream (hipStream_t) so callers can bracket it with their own events */
tm_stream_t tm_engine_stream(tm_engine* e);
/* introspection for benchmarks: bytes of quantised weights + scales + lm_head, KV bytes per token, #blocks */
/* What the tensor-parallel data path of this engine actually runs on (for benchmark records; any pointer may be NULL):
 * backend: 0 = no collectives (tp = 1), bit 0 = RCCL communicator up (comm/nccl/nccl.cu:356-398), bit 1 = native P2P communicator
 * imported (comm/cuda_ipc role); ranks = the communicator's own rank count (ncclCommCount), not the launcher's world size;
 * graph_captured: 1 = decode steps replay a hipGraph (collectives captured inside), 0 = eager launches (never captured yet,
 * use_graph = 0, or the capture with collectives failed and the engine fell back). */
int tm_engine_comm_info(tm_engine* e, int* backend, int* ranks, int* graph_captured);
/* The overlap the north star names ("RCCL all-reduce over xGMI overlapped on a side HIP stream"), as counters a benchmark / test can read
 * (any pointer may be NULL): side_stream = 1 when prefill-sized tensor-parallel forwards run their all-reduces on the engine's side stream
 * under the other half's kernels (TM_COMM_STREAM, default on; needs the RCCL communicator); forwards = forwards that ran that way so far;
 * microbatch_forwards = how many of them split at a sequence boundary into two micro-batches that leapfrog through all layers (the rest
 * split the row-wise part of every layer into two row halves); allreduces = all-reduces enqueued on the side stream so far (4 per dense
 * layer of such a forward).  The reference hides the exchange
 * inside a fused kernel (comm/cuda_ipc/fused_allreduce.cu:406-500, unified_decoder.cc:278,328); decode-sized forwards do the same here
 * (comm_p2p.hip) or call RCCL on the engine stream. */
int tm_engine_comm_overlap_info(tm_engine* e, int* side_stream, int64_t* forwards, int64_t* microbatch_forwards, int64_t* allreduces);
int tm_engine_stats(tm_engine* e, int64_t* weight_bytes, int64_t* kv_bytes_per_token, int64_t* num_blocks,
                    int* decode_splits);

#ifdef __cplusplus
}
#endif
#endif /* TM_MI355X_H */
