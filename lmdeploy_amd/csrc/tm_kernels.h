// Internal launcher declarations (host side of every HIP kernel in this library).
#pragma once
#include <stdio.h>
#include "tm_common.h"
#include <vector>

namespace tmk {

// ---- paged KV cache geometry (reference: kernels/attention/block.h:126-219) ----------------
struct KvLayout {
    int kv_heads;
    int head_dim;   // 64 | 128
    int block_len;  // 64
    int bits;       // 16 | 8 | 4 | 42 (TurboQuant: K rows of 4-bit codes, V rows of 2-bit codes; turboquant.h)
    // K and V rows have sizes of their own: equal (bits * head_dim / 8) for 16 / 8 / 4, head_dim / 2 and head_dim / 4 for 42
    __host__ __device__ int k_token_size() const { return bits == 42 ? head_dim / 2 : token_data_size(); }
    __host__ __device__ int v_token_size() const { return bits == 42 ? head_dim / 4 : token_data_size(); }
    __host__ __device__ int layer_size() const
    {
        return bits == 42 ? kv_heads * tq_head_data_size() + kv_heads * 2 * tq_head_param_size() :
                            kv_heads * 2 * head_data_size() + kv_heads * 2 * head_param_size();
    }
    // ---- bits 16 / 8 / 4: the offsets the kernels of those widths compile (unchanged by the TurboQuant rows below) ----
    __host__ __device__ int token_data_size() const { return bits * head_dim / 8; }
    __host__ __device__ int token_param_size() const { return bits < 16 ? 4 : 0; }
    __host__ __device__ int head_data_size() const { return block_len * token_data_size(); }
    __host__ __device__ int head_param_size() const { return block_len * token_param_size(); }
    __host__ __device__ int k_data(int head, int ti) const { return head * 2 * head_data_size() + ti * token_data_size(); }
    __host__ __device__ int v_data(int head, int ti) const { return k_data(head, ti) + head_data_size(); }
    __host__ __device__ int k_param(int head, int ti) const
    {
        return kv_heads * 2 * head_data_size() + head * 2 * head_param_size() + ti * token_param_size();
    }
    __host__ __device__ int v_param(int head, int ti) const { return k_param(head, ti) + head_param_size(); }
    // ---- bits 42: per kv head K rows [block_len][head_dim / 2], then V rows [block_len][head_dim / 4]; behind the data of all heads,
    // per head, K params [block_len][4 B], then V params.  Only the code paths of bits 42 call these. ----
    __host__ __device__ int tq_head_data_size() const { return block_len * (head_dim / 2 + head_dim / 4); }
    __host__ __device__ int tq_head_param_size() const { return block_len * 4; }
    __host__ __device__ int tq_k_data(int head, int ti) const { return head * tq_head_data_size() + ti * (head_dim / 2); }
    __host__ __device__ int tq_v_data(int head, int ti) const
    {
        return head * tq_head_data_size() + block_len * (head_dim / 2) + ti * (head_dim / 4);
    }
    __host__ __device__ int tq_k_param(int head, int ti) const
    {
        return kv_heads * tq_head_data_size() + head * 2 * tq_head_param_size() + ti * 4;
    }
    __host__ __device__ int tq_v_param(int head, int ti) const { return tq_k_param(head, ti) + tq_head_param_size(); }
};

struct KvCacheView {
    const uint64_t* block_ptrs;     // device array of block base addresses (char**)
    const int*      cu_block_nums;  // [B+1] prefix offsets into block_ptrs
    int             block_stride = 0;  // > 0: the table is rectangular, sequence b starts at b * block_stride (cu_block_nums[b] says the
                                       // same): the MFMA decode kernel then fetches a sequence's block pointers with ONE load that
                                       // depends on nothing but kernel arguments (64 pointers, one per lane) instead of two dependent
                                       // hops (prefix offset -> pointer) in front of every cache block
    int64_t         layer_offset;   // bytes: layer * layout.layer_size()
    KvLayout        layout;
};

// ---- norm.hip ---------------------------------------------------------------------------
// Hv (0 = H): the row's valid width; Hv != H runs the variant for zero-padded rows (norm_row.h, VALID): sum over [0, Hv), divisor Hv,
// columns [Hv, H) of the inputs never read and written as +0
int launch_rmsnorm(half_t* y, const half_t* x, const half_t* w, float eps, int M, int H, hipStream_t st, int Hv = 0);
int launch_residual_rmsnorm(half_t* y, half_t* resid, const half_t* hidden, const float* partial, int splits,
                            const half_t* bias, const half_t* w, float eps, int M, int H, hipStream_t st, int Hv = 0);

// ---- kv_cache.hip -----------------------------------------------------------------------
// RoPE(q,k) in fp16 from a (cos,sin) table, quantise K/V of the new tokens and scatter them into the
// paged cache.  q is rotated in place inside the qkv buffer.
// Qwen prologue (all nullptr: today's kernel): qkv_bias [q_heads + 2 kv_heads][D] is added to q, k and v (fp16); q_norm /
// k_norm [D] run a per-head RMSNorm (eps qk_eps) on q / k first.  Order: norm -> bias -> RoPE.
int launch_kv_rope_store(half_t* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                         const half2_t* cos_sin, int max_pos, KvCacheView cache, hipStream_t st,
                         const half_t* qkv_bias = nullptr, const half_t* q_norm = nullptr, const half_t* k_norm = nullptr,
                         float qk_eps = 0.f, const int* rope_row0 = nullptr);
// The same with M-RoPE in sections (Qwen2-VL): frequency pair j reads table row clamp(c, 0, max_pos - 1) of its section's coordinate
// (t: j < sec_t, h: j < sec_t + sec_h, w behind).  mrope_pos device int [total_tokens][3]; nullptr: all three = linear position +
// pos_delta[b] (pos_delta device int [batch], nullptr = 0).  One shared table (no per-sequence rows), head_dim 128, kv bits 16 / 8 / 4.
int launch_kv_rope_store_mrope(half_t* qkv, int q_heads, const int* cu_q_len, const int* k_len, int batch, int total_tokens,
                               const half2_t* cos_sin, int max_pos, const int* mrope_pos, const int* pos_delta, int sec_t, int sec_h,
                               int sec_w, KvCacheView cache, hipStream_t st, const half_t* qkv_bias = nullptr,
                               const half_t* q_norm = nullptr, const half_t* k_norm = nullptr, float qk_eps = 0.f);

// per-pair inverse frequencies of one RoPE recipe (rope_inv_freq, c_api.hip) + the factor on cos / sin (YaRN; 1 otherwise): what the
// host table builder and rope_table_kernel share, so both build the same table
constexpr int kRopeMaxPairs = 64;
struct RopeInvFreq {
    float inv[kRopeMaxPairs];
    float attention_factor;
};
int launch_rope_table(half2_t* out, int max_pos, int dim, const RopeInvFreq& f, hipStream_t st);
// Gather + dequantise (two-rounding "flatten" form) the whole context of every sequence into linear
// scratch: K [kv_heads][k_stride][D]; V either [kv_heads][k_stride][D] or transposed [kv_heads][D][k_stride].
int launch_flatten_kv(half_t* k_out, half_t* v_out, int transpose_v, const int* cu_k_off, const int* k_len, int batch,
                      int max_k_len, int k_stride, KvCacheView cache, hipStream_t st);
// The same for a layer with a sliding window (cu_q_len [batch + 1]: the forward's query rows): 64-token tiles that end at or below
// max(k_len - q_len - window + 1, 0) are skipped -- not read, their scratch left unwritten: the windowed prefill kernel never stages them.
// window == 0 is launch_flatten_kv.
int launch_flatten_kv_window(half_t* k_out, half_t* v_out, int transpose_v, const int* cu_k_off, const int* k_len,
                             const int* cu_q_len, int window, int batch, int max_k_len, int k_stride, KvCacheView cache,
                             hipStream_t st);

// ---- attention_decode.hip ---------------------------------------------------------------
struct DecodeAttnParams {
    const half_t* q;         // [B][q_stride] roped queries (head h at h*D)
    int           q_stride;  // elements between consecutive tokens
    half_t*       out;       // [B][q_heads*D]
    const int*    k_len;     // [B] context length including the new token
    int           batch;
    int           q_heads;
    float         scale_log2;  // softmax_scale * log2(e)
    int           splits;
    float*        partial_o;   // [B][q_heads][splits][D]
    float*        partial_ml;  // [B][q_heads][splits][2]
    KvCacheView   cache;
    // Fused prologue (int8 MFMA kernel only): q/k/v of the new token are taken straight from the qkv GEMM output --
    // `qkv_splits` fp32 split-K slabs [qkv_splits][B][qkv_n] (or the fp16 [B][qkv_n] result when qkv_splits == 0) --
    // rotated, and K/V are quantised + stored by the attention kernel itself (the reference decode kernel does the
    // same: attention_universal.h:168-330).  Replaces splitk_reduce + kv_rope_store on the decode path.
    const float*   qkv_slabs = nullptr;
    const half_t*  qkv_f16   = nullptr;
    int            qkv_splits = 0;
    int            qkv_n      = 0;
    const half2_t* cos_sin    = nullptr;
    int            max_pos    = 0;
    uint64_t*      dbg        = nullptr;  // optional per-workgroup timing stamps (tm_debug_set_gemm_trace)
    // Qwen prologue of the fused path (nullptr: none; see launch_kv_rope_store): bias [qkv_n] on q / k / v, per-head
    // RMSNorm of q / k with the [D] weights q_norm / k_norm (both or neither), norm -> bias -> RoPE
    const half_t*  qkv_bias = nullptr;
    const half_t*  q_norm   = nullptr;
    const half_t*  k_norm   = nullptr;
    float          qk_eps   = 0.f;
    // Sliding window and attention sinks (VALU kernel only, never with the fused prologue; reference: attention_params.h:55-72).
    // window > 0: the query at k_len - 1 sees keys j with k_len - 1 - j < window (0 = all).  sinks [q_heads]: natural-log logits that
    // join the softmax denominator and carry no value (nullptr = none).
    int            window = 0;
    const half_t*  sinks  = nullptr;
    // Fused prologue only: per-sequence position delta (M-RoPE models, device int [batch]); the new token's RoPE row becomes
    // clamp(k_len - 1 + pos_delta[b], 0, max_pos - 1).  nullptr: the prologue as it was (its own kernel instantiations).
    const int*     pos_delta = nullptr;
};
int launch_decode_attention(const DecodeAttnParams& p, hipStream_t st);
int launch_decode_attention_i8_mfma(const DecodeAttnParams& p, hipStream_t st);  // attention_decode_mfma.hip
// attention_decode_tq.hip: KV bits 42 (TurboQuant), head_dim 128, in the rotated domain; no window, sinks or fused prologue
int launch_decode_attention_tq(const DecodeAttnParams& p, hipStream_t st);
size_t decode_attention_workspace_bytes(int batch, int q_heads, int head_dim, int splits);

// ---- attention_verify_mfma.hip ----------------------------------------------------------
// Paged split-K attention for 1 .. 8 query rows per sequence over int8 / int4 KV at head_dim 128 (the verify forward of speculative
// decoding).  The rows' K / V are in the cache already (launch_kv_rope_store first); k_len counts every row of the forward, row j of
// sequence b sees the tokens t < k_len[b] - q_len[b] + j + 1.  No window, no sinks, no fused prologue.
constexpr int kVerifyMaxRows = 8;
struct VerifyAttnParams {
    const half_t* q;         // [rows][q_stride] roped queries (head h at h*D)
    int           q_stride;
    half_t*       out;       // [rows][q_heads*D], forward row order
    const int*    cu_q_len;  // [B+1] device
    const int*    k_len;     // [B] device, context lengths including every row of this forward
    int           batch;
    int           q_heads;
    float         scale_log2;
    int           splits;
    float*        partial_o;   // [rows][q_heads][splits][D]
    float*        partial_ml;  // [rows][q_heads][splits][2]
    KvCacheView   cache;
    int           max_q_len;   // 1 .. kVerifyMaxRows: the host's bound on q_len[b]; sizes the grid, longer sequences are cut to it
};
int launch_verify_attention(const VerifyAttnParams& p, hipStream_t st);

// ---- speculative.hip: prompt-lookup proposer and greedy acceptance of speculative decoding ----
struct SpecState {
    int* hist;       // [B][hist_stride] token history: prompt + emitted tokens
    int  hist_stride;
    int* hist_len;   // [B]
    int* emitted;    // [B] tokens emitted so far (the prefill's first token included)
    int* generated;  // [B][max_new]
    int  max_new;
    int* k_len;      // [B] tokens in the KV cache
    int* next_id;    // [B] last emitted token = row 0 of the next step
    long long* totals;  // [4] steps (live sequence-steps), drafted, accepted, emitted
};
constexpr int kSpecMaxDraft = 7;
constexpr int kSpecMaxNgram = 8;
// one workgroup per sequence: drafts [B][k] (unused entries 0), n_draft [B]
int launch_spec_propose(int* drafts, int* n_draft, const SpecState& s, int batch, int k, int ngram_max, int ngram_min, hipStream_t st);
// start of a batch: hist[b][0 .. k_len[b]) holds the prompt; the prefill's first token (next_id) joins it, hist_len = k_len + 1, emitted = 1
int launch_spec_begin(const SpecState& s, int batch, hipStream_t st);
// rows of the verify forward: ids [B][k+1] = (next_id, drafts), cu_q [B+1] = (k+1) b, k_len_fw [B] = k_len + k + 1
int launch_spec_rows(int* ids, int* k_len_fw, const int* drafts, const SpecState& s, int batch, int k, hipStream_t st);
// greedy acceptance: out_ids [B][k+1] is the arg-max behind every input row; step_emitted [B] (nullptr: not wanted) = tokens emitted by this step
int launch_spec_accept(const int* out_ids, const int* drafts, const int* n_draft, const SpecState& s, int batch, int k, int* step_emitted,
                       hipStream_t st);

// ---- attention_prefill.hip --------------------------------------------------------------
struct PrefillAttnParams {
    const half_t* q;         // [T][q_stride] roped
    int           q_stride;
    half_t*       out;       // [T][q_heads*D]
    const half_t* k;         // [kv_heads][k_stride][D]
    const half_t* vt;        // [kv_heads][D][k_stride]
    int           k_stride;
    const int*    cu_q_len;  // [B+1]
    const int*    cu_k_off;  // [B+1] start of every sequence in k / vt (multiple of 64)
    const int*    k_len;     // [B]
    int           batch;
    int           max_q_len;
    int           q_heads;
    int           kv_heads;
    float         scale_log2;
    int           head_dim = 128;  // D: 64 | 128
    int           window   = 0;        // > 0: row at position q sees keys t with 0 <= q - t < window (0 = causal only)
    const half_t* sinks    = nullptr;  // [q_heads] natural-log sink logits (nullptr = none)
};
int launch_prefill_attention(const PrefillAttnParams& p, hipStream_t st);

// ---- gemm_w4a16.hip ---------------------------------------------------------------------
// What a linear IS, resolved once where it is declared from (weight_type, fp8_scale_mode, expert?) by linear_format(): the key of the
// format table in linear.hip, which owns everything that depends on it (staging parts, repack, activation quantisation, run, bytes).
enum class LinearFormat : int { U4, F16, FP8_BLOCK, FP8_CHANNEL, MXFP4_EXPERT, MXFP4_DENSE, INT8_CHANNEL, U4_G32, COUNT };
struct LinearWeight {
    int       K = 0, N = 0, group = 128;
    LinearFormat fmt = LinearFormat::U4;
    bool      gated = false;     // FP8_BLOCK only: a w1w3 whose block-scale row is [w1 blocks | w3 blocks] for interleaved columns
    int       type = 0;          // 0 = u4 (AWQ), 1 = f16 dense, 2 = fp8 e4m3 with 128x128 block scales, 3 = MXFP4 (e2m1 codes, one ue8m0
                                 // scale byte per 32 k; experts weight-only: gemm_mxfp4.hip, dense linears W4A4: gemm_mxfp4_mfma.hip),
                                 // 4 = int8 codes with one fp32 scale per output column (W8A8: gemm_int8.hip)
    int       role = 0;          // key of the measured dispatch table next to (K, N, M): 0 = any (operator-level handles, imported
                                 // tables without a role column), 1 w_qkv, 2 wo, 3 w1w3, 4 w2 -- two roles of equal (K, N) are timed
                                 // with DIFFERENT consumers by the tuner and keep separate winners
    void*     packed = nullptr;  // fragment-ordered weights (nullptr for a u4 linear prepared p32_only)
    uint32_t* sz     = nullptr;  // fragment-ordered (s, -z*s) half2 pairs (u4), (s, 0) (fp8), four adjusted scale bytes per k-block (MXFP4)
    size_t    packed_bytes = 0, sz_bytes = 0;
    // u4 only, N % 32 == 0: the decode kernel's layout (gemm_decode.hip, "P32": 2176-byte units of 32 columns x 128 k
    // with their (s, -z*s) pairs); `packed` / `sz` stay the layout of the M > 64 kernels
    void*     packed32 = nullptr;
    size_t    packed32_bytes = 0;
    // fp8 only, N % 32 == 0: the fp8 x fp8 kernel's layout (gemm_fp8.hip, "P8": 4224-byte units of 32 columns x 128 k with
    // their even / odd column block scales)
    // MXFP4 dense (linear_weight_prepare_mxfp4_dense): the "P4" image of gemm_mxfp4_mfma.hip lives here too (2176-byte units of
    // 32 columns x 128 k with their scale bytes); such a weight has no `packed` / `sz` image
    void*     packed8 = nullptr;
    size_t    packed8_bytes = 0;
    // fp8 only, channel-scaled weights (linear_weight_prepare_fp8_channel): the N fp32 column scales, stored behind the last
    // P8 unit of `packed8` (not owned).  Such a weight has no `packed` / `sz` image: it runs on the fp8 matrix cores only.
    // int8 (linear_weight_prepare_int8): the same P8 image and column scales, run on the int8 matrix cores only.
    // u4 with groups of 32 (U4_G32, linear_weight_prepare_u4_g32): the "G32" image of gemm_u4_g32.hip lives here too (2560-byte units of
    // 32 columns x 128 k with their four (s, -z*s) pairs per column); such a weight has no `packed` / `packed32` / `sz` image
    float*    cscale = nullptr;
    // u4 only, optional (linear_weight_build_f16_image; the engine builds it for dense linears unless TM_PREFILL_F16_IMAGE=0): the fp16
    // [N][K] image of the dequantised weights -- bit for bit the operand the fused tiles build on chip -- that prefill-sized forwards
    // contract on the matrix pipe without any dequantisation work in the loop (gemm_prefill_f16.hip, shape kShapeF16).  2 bytes per
    // parameter of HBM next to the 0.53 the decode path streams: 14 GB for an 8 B model on a 288 GB device.
    half_t*   image16 = nullptr;
};
struct GemmConfig {
    int nt;      // n-tiles (16 cols) per wave: 1,2,4
    int splits;  // split-K
    int waves;   // waves per workgroup: 4 or 8
    int kphases; // split-K inside the workgroup: 1 or 2 (8 waves only)
    int kstage;  // max k-blocks per barrier (0 = auto: 4)
    int d32_shape = -1;  // >= 0: a P32 kernel (gemm_decode.hip / gemm_decode_lc.hip / gemm_prefill.hip) with this workgroup shape
    unsigned* tickets = nullptr;  // arrival counters (zero between launches) of the kShapeMerge shapes: >= ceil(N / 64) * ceil(M / 32) words
};
// (shape 10 was "dequantise + the vendor library's fp16 GEMM" in round 3: removed -- no vendor GEMM on any path of this library)
constexpr int kShapePre256     = 12;   // gemm_prefill.hip: 256 x 256 tiles, weights dequantised once per workgroup tile through LDS (M > 64)
constexpr int kShapeF16        = 13;   // gemm_prefill_f16.hip: 256 x 256 tiles over the resident fp16 image, both operands by LDS-DMA (M > 64; LinearWeight::image16)
constexpr int kShapeLC         = 11;   // gemm_decode_lc.hip: 8 consumer + 4 loader waves, 128 columns x M <= 64 rows per workgroup
// kShapeMerge + s (s = 0..3, 6..9; round 6): the decode tile s whose split-K slices are merged INSIDE the launch by the last-arriving
// slice of each column tile, for the fp16 / gated-SiLU epilogues (the folded-norm producers, epilogue 3, always merge that way): a
// gated w1w3 can then split K across CUs (256-column tiles, half the activation bytes per CU) without slabs leaving the launch.
// Needs arrival counters: NormFold::tickets (engine) / the tail of the workspace (tm_linear_forward).
constexpr int kShapeMerge      = 16;
// 256 columns x 2 k-phases x 16 waves on 2-k-block stages (gemm_dec32_kernel<MH, 8, 2, 2, 2>; round 6): the 256-column decode tile that does not
// spill (shape 1 = the same wave layout on 4-k-block stages with a 4-deep ring: 60 B / lane of scratch at the 128-register cap)
constexpr int kShapeWide2      = 10;
inline bool dec32_is_merge_shape(int shape)
{
    const int b = shape - kShapeMerge;
    return (b >= 0 && b <= 3) || (b >= 6 && b <= 10);
}
// Load-time repack (reference: LinearWeight::prepare, models/linear_weight.cc:101-324)
// p32_only: build ONLY the P32 image (gemm_decode.hip) -- for linears that every M dispatches to those kernels
// (dec32_serves_every_m): the 16-column image of gemm_kernel would never be read.
int    linear_weight_prepare_u4(LinearWeight& w, const int32_t* qweight /*[K][N/8]*/, const half_t* scales,
                                const half_t* zeros, hipStream_t st, bool p32_only = false);
bool   dec32_serves_every_m(int K, int N);  // dense u4 linear, N % 32 == 0, K % 128 == 0, TM_GEMM_D32 / _PREFILL on
int    linear_weight_prepare_f16(LinearWeight& w, const half_t* weight /*[K][N]*/, hipStream_t st);
int    linear_weight_prepare_fp8(LinearWeight& w, const uint8_t* weight /*[K][N] e4m3*/, const float* block_scales /*[K/128][ceil(N/128)]*/,
                                 bool gated_scales /* w1w3: scale row = [w1 blocks | w3 blocks] for interleaved columns */, hipStream_t st);
void   linear_weight_free(LinearWeight& w);
int    linear_weight_build_f16_image(LinearWeight& w, hipStream_t st);  // u4 linear with its P32 image -> w.image16 ([N][K] fp16)
int    launch_dequant_p32_f16(half_t* out_nk /*[N][K]*/, const LinearWeight& w, hipStream_t st);  // gemm_decode.hip: the operand as an fp16 image
size_t gemm_workspace_bytes(int M, int N, int splits);
// bytes of the packed image gemm_kernel streams for a K x N linear of `type` (KB * N/16 * 1024 * WV): the kernel addresses it with
// 32-bit offsets, so linears whose image reaches 2^31 bytes are refused where shapes are accepted (kGeneralImageLimit)
size_t gemm_general_image_bytes(int K, int N, int type);
constexpr size_t kGeneralImageLimit = (size_t)1 << 31;
int    launch_splitk_reduce(half_t* y, int ldy, const float* partial, int splits, int M, int N, bool gated, hipStream_t st);
GemmConfig gemm_pick_config(const LinearWeight& w, int M);  // a P32 kernel when it applies, else ...
GemmConfig gemm_pick_config_general(const LinearWeight& w, int M);  // ... the tiling of gemm_kernel (gemm_w4a16.hip)
// y[M][N (or N/2 if gated)] = x[M][K] . W ; if cfg.splits > 1 fp32 slabs land in `workspace` and, unless
// `defer_reduce`, a reduce kernel writes y.
int launch_linear(const LinearWeight& w, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated_silu,
                  GemmConfig cfg, float* workspace, bool defer_reduce, int* slabs, hipStream_t st);

// ---- linear.hip: the one place that knows the linear formats (a table with one row per LinearFormat) --------------
LinearFormat linear_format(int weight_type, int fp8_scale_mode, bool expert, int group = 128);  // (group: u4 only -- 32 is a format of its own)
enum class PartKind : int { AWQ_QWEIGHT, AWQ_SCALES, AWQ_ZEROS, F16, E4M3, F32_SCALES, E2M1, UE8M0, I8 };  // what a staging part holds
struct LinearStaging {  // the parts a checkpoint fills for one linear, in the order linear_weight_prepare takes them
    int         n = 0;
    const char* suffix[3];  // slot name behind the linear's prefix: "qweight", "scales", ...
    PartKind    kind[3];
    size_t      bytes[3];
};
LinearStaging linear_staging(LinearFormat fmt, int K, int N, int group);
// The table's quantisation column: how the GEMM input is quantised in front of the launch.  A format that also keeps a weight-only image
// (FP8_BLOCK) quantises, and runs on the matrix cores, only for a caller that brings activation buffers; without them it answers NONE.
enum class ActQuant : int { NONE, FP8_ROW128, FP8_TOKEN, MXFP4_ROW32, INT8_TOKEN };
ActQuant linear_act_quant(LinearFormat fmt, bool have_act_buffers);
// repack the staged parts (device pointers, linear_staging order) into the device image(s) of w.fmt.  The u4 policy of the caller (the
// engine's dense linears; ignored by every other format): p32_only as linear_weight_prepare_u4, f16_image = linear_weight_build_f16_image too
int    linear_weight_prepare(LinearWeight& w, const void* const* parts, hipStream_t st, bool p32_only = false, bool f16_image = false);
bool   linear_weight_prepared(const LinearWeight& w);
// formats whose launcher picks its own tile per M class: nothing for the measured dispatch tables to time (quantised inputs, U4_G32)
bool   linear_own_tiling(LinearFormat fmt, bool have_act_buffers);
void   linear_weight_take(LinearWeight& dst, LinearWeight& src);  // dst owns src's images, src is left unprepared
size_t linear_weight_bytes(const LinearWeight& w);  // codes + scales of a prepared weight as the checkpoint carries them (0: not prepared)
struct LinearScratch {
    float*    ws = nullptr;  // split-K slabs; a split that does not fit ws_bytes runs as one slice
    size_t    ws_bytes = 0;
    unsigned* tickets  = nullptr;  // arrival counters (GemmConfig::tickets): with them a measured in-launch merge shape may run
    void *    xq = nullptr, *sx = nullptr;  // codes and scales of the quantised GEMM input (FP8_ROW128 scales: [K / 128][ldsx]) ...
    int       ldsx = 0, rows = 0;           // ... and the rows both hold
    int       splits = 0;  // quantised-input formats: an explicit split-K (operator-level callers); 0 = the launcher's own
};
// y[M][N (or N/2 if gated_silu)] = x[M][K] . W for every format.  A quantised input (linear_act_quant of what the scratch carries) is
// quantised, launched with 16 slabs if they fit or one slice, and reduced unless `defer` (an int8 linear always reduces itself: its slabs are
// raw int32 accumulators, the deferred hand-off carries fp32); the others run gemm_pick_config's tiling through
// launch_linear.  `defer` and a split launch leave the fp32 slabs in scratch.ws, *slabs > 1; otherwise y holds the result, *slabs = 1.
int linear_forward(const LinearWeight& w, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated_silu, const LinearScratch& scratch,
                   bool defer, int* slabs, hipStream_t st);

// ---- gemm_decode.hip: W4A16 decode GEMM (M <= 64), 32x32x16 MFMA, 16 waves per CU ------------------------------
size_t p32_bytes(int K, int N);
int    launch_repack_p32(void* out, const int32_t* qweight, const half_t* scales, const half_t* zeros, int K, int N, hipStream_t st);
bool   dec32_supported(const LinearWeight& w, int M);
void   dec32_pick(const LinearWeight& w, int M, int* shape_out, int* splits_out);  // measured table first, then the heuristic
void   dec32_pick_ex(const LinearWeight& w, int M, int* shape_out, int* splits_out, bool use_table);
// the tiling of a folded-norm launch (NormFold below): the measured / heuristic pick when its kernel carries the folded epilogue, else
// the heuristic's, else the tile that always does
void   dec32_pick_fold(const LinearWeight& w, int M, bool producer, int* shape_out, int* splits_out);
// measured dispatch table of the decode linears: key (K, N, M <= 64) -> (shape, splits)
void   dec32_table_set(int K, int N, int M, int shape, int splits, int role = 0);
bool   dec32_table_get(int K, int N, int M, int* shape, int* splits, int role = 0);  // the role's entry, else the role-0 entry
void   dec32_table_clear();
int    dec32_table_export(const char* path);
int    dec32_table_import(const char* path);
int    dec32_candidates(const LinearWeight& w, int M, int (*out)[2], int cap);
int    dec32_m_bucket(int M);  // table key of a forward with M rows: M itself up to 256, then 512, 1024, ... 8192
// Measured dispatch of everything that is NOT a P32 kernel (reference: gemm.cu:92-224 caches every problem the
// warm-up of turbomind.cc:363-487 meets, not only the dense u4 ones).  One table, key (kind, role, K, N, M bucket):
//   kind kGenDense + type   : gemm_kernel of a dense linear (fp16 lm_head, e4m3 weight-only, u4 with N % 32 != 0) -> {nt, splits, waves, kphases}
//   kind kGenGrouped + type : row-tile height of the grouped expert GEMMs (u4 and f16: 16 / 32 / 64 rows, fp8 MFMA: 32 / 64) -> {rows, 0, 0, 0}
// Text form (same file as the P32 table): `G kind role K N M a b c d`.  role 5 = lm_head; grouped entries use role 0.
constexpr int kGenDense   = 16;
constexpr int kGenGrouped = 32;
void   gen_table_set(int kind, int role, int K, int N, int M, const int v[4]);
bool   gen_table_get(int kind, int role, int K, int N, int M, int v[4]);  // the role's entry, else the role-0 entry
void   gen_table_erase(int kind, int role, int K, int N, int M);
void   gen_table_clear();                   // dec32_table_clear() calls it: both tables travel and reset together
// tuner / test hook: the grouped GEMMs launched by THIS thread use `rows`-row tiles (0: off), all of them (K = N = 0) or only the
// K x N expert linear
void   gen_grouped_rows_override(int rows, int K = 0, int N = 0);
int    gen_grouped_rows_forced(int K, int N);  // this thread's override for a K x N grouped GEMM (0: none)
int    gen_table_export_lines(FILE* f);      // appends the G lines; returns their number
bool   gen_table_import_line(const char* line);  // a `G ...` line; false = not valid (ignored)
int    gen_dense_candidates(const LinearWeight& w, int M, size_t workspace_bytes, GemmConfig* out, int cap);
int    gen_grouped_candidates(const LinearWeight& proto, int m_cap, int* rows_out, int cap);
// RMSNorm folded into the neighbouring decode GEMMs (round 5; gemm_decode_common.h has the arithmetic).  One struct, two roles:
//   producer (resid != nullptr): the row-parallel GEMM (wo / w2) adds its fp16 output to the residual stream in its own epilogue
//     (split-K: the last-arriving slice of a column tile sums the slices' slabs in slice order), writes y = h(f32(r) * f32(g)) and
//     ss_out[tile][m] = partial sum of f32(r)^2 over the tile's columns; tiles_out = column tiles written (set by the launcher)
//   consumer (ss_in != nullptr): the GEMM fed with that y multiplies its fp32 accumulators by 1 / sqrt(sum_tiles ss / H + eps)
// Replaces: invokeResidualBiasRMSNorm behind wo / w2 (rms_norm.cu:286-362, unified_decoder.cc:226,278,328) -- the residual stream is
// bit-identical to the unfused sequence; the normalised activations differ by one fp16 rounding (applied after the contraction).
struct NormFold {
    const float*  ss_in    = nullptr;
    int           ss_tiles = 0;
    float         inv_h = 0.f, eps = 0.f;
    half_t*       resid   = nullptr;
    const half_t* norm_w  = nullptr;
    float*        ss_out  = nullptr;
    unsigned*     tickets = nullptr;
    int           tiles_out = 0;
};
constexpr int kFoldMaxRows = 128;  // rows of a forward whose RMSNorms fold into the decode GEMMs (round 6: BASELINE config 3 runs batch 128)
bool   dec32_fold_shape_m(int shape, int M, bool producer);  // can (shape, M) run as a folded producer / consumer?
bool   dec32_fold_shape(int shape);  // shapes whose kernel carries the folded-norm epilogue / prologue (0..3, 6..9)
int    launch_linear_dec32(const LinearWeight& w, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated_silu, int shape,
                           int splits, float* workspace, int* slabs_out, hipStream_t st, NormFold* nf = nullptr);

// ---- gemm_fp8.hip: fp8 x fp8 linear on v_mfma_f32_32x32x16_fp8_fp8 (activations quantised per row and 128 channels) ---
constexpr int kP8Unit = 4096 + 128;  // a P8 unit: 32 columns x 128 k of codes + its scale words
size_t p8_bytes(int K, int N);
int    fp8_splits(int col_wgs, int KB, int want);  // split-K of the P8 kernels: `want` if > 0, else the heuristic
int    launch_repack_p8(void* out, const uint8_t* weight, const float* block_scales, int K, int N, bool gated, hipStream_t st);
bool   fp8_mfma_supported(const LinearWeight& w);
size_t fp8_act_workspace_bytes(int rows, int K);
constexpr int kFp8TokenMaxK = 32768;
int    linear_weight_prepare_fp8_channel(LinearWeight& w, const uint8_t* weight /*[K][N] e4m3*/, const float* scales /*[N] fp32, device*/,
                                         hipStream_t st);
// per-token form (channel-scaled weights): one scale per row over all of K, sx[M]; K % 128 == 0, K <= kFp8TokenMaxK
int    launch_quant_fp8_token(uint8_t* xq, float* sx, const half_t* x, int ldx, int M, int K, hipStream_t st);
int    launch_quant_fp8_rows(uint8_t* xq, float* sx, const half_t* x, int ldx, int M, int K, int ldsx, hipStream_t st);
int    launch_linear_fp8(const LinearWeight& w, const uint8_t* xq, const float* sx, int ldsx, half_t* y, int ldy, int M, bool gated_silu,
                         int splits, float* workspace, int* slabs_out, hipStream_t st);
int    launch_linear_fp8_grouped(const LinearWeight& proto, const void* d_groups, int E, const uint8_t* xq, const float* sx, int ldsx,
                                 int x_rows, half_t* y, int ldy, int m_cap, int m_hint, bool gated_silu, const int* seg,
                                 const int* row_idx, hipStream_t st);

// ---- gemm_mxfp4_mfma.hip: MXFP4 x MXFP4 dense linear on v_mfma_scale_f32_32x32x64_f8f6f4 (activations quantised per row and 32 channels) ---
size_t p4_bytes(int K, int N);
int    linear_weight_prepare_mxfp4_dense(LinearWeight& w, const uint8_t* blocks /*[N][K/2]*/, const uint8_t* scales /*[N][K/32]*/, hipStream_t st);
bool   mxfp4_dense_prepared(const LinearWeight& w);
int    launch_dequant_p4_f16(half_t* out_nk /*[N][K]*/, const LinearWeight& w, hipStream_t st);
size_t mxfp4_act_workspace_bytes(int rows, int K);
int    launch_quant_mxfp4_rows(uint8_t* xq /*[M][K/2]*/, uint8_t* sx /*[M][K/32]*/, const half_t* x, int ldx, int M, int K, hipStream_t st);
int    launch_linear_mxfp4(const LinearWeight& w, const uint8_t* xq, const uint8_t* sx, half_t* y, int ldy, int M, bool gated_silu, int splits,
                           float* workspace, int* slabs_out, hipStream_t st);

// ---- gemm_int8.hip: int8 x int8 linear (W8A8) on v_mfma_i32_32x32x32_i8: per-column weight scales, per-token activation scales ---
// the P8 image of gemm_fp8.hip (opaque bytes) + the N column scales behind it; K % 128 == 0, K <= kFp8TokenMaxK, N % 32 == 0
int    linear_weight_prepare_int8(LinearWeight& w, const uint8_t* weight /*[K][N] int8*/, const float* scales /*[N] fp32, device*/, hipStream_t st);
bool   int8_prepared(const LinearWeight& w);
// sx = max(max|x|, 1e-7) / 127 per row, q = clamp(round_half_away(x / sx), -127, 127); the limits of launch_quant_fp8_token
int    launch_quant_int8_token(uint8_t* xq, float* sx, const half_t* x, int ldx, int M, int K, hipStream_t st);
// y = h((float(acc) * sx[m]) * sw[n]); workspace: 16 int32 slabs [M][N] (gemm_workspace_bytes(M, N, 16)) or nullptr = one slice.  A split
// launch sums its raw int32 slabs in a reduce kernel of its own: y always holds the result, the same bits for every split
int    launch_linear_int8(const LinearWeight& w, const uint8_t* xq, const float* sx, half_t* y, int ldy, int M, bool gated_silu, int splits,
                          void* workspace, hipStream_t st);

// ---- gemm_u4_g32.hip: W4A16 with quantisation groups of 32 along K on v_mfma_f32_32x32x16_f16 (dense linears) ---
// the "G32" image: 2560-byte units of 32 columns x 128 k (codes + four (s, -z*s) pairs per column); K % 128 == 0, N % 32 == 0, image < 2^31 bytes
size_t g32_bytes(int K, int N);
int    linear_weight_prepare_u4_g32(LinearWeight& w, const int32_t* qweight /*[K][N/8]*/, const half_t* scales /*[K/32][N]*/,
                                    const half_t* zeros, hipStream_t st);
bool   u4_g32_prepared(const LinearWeight& w);
int    launch_dequant_g32_f16(half_t* out_nk /*[N][K]*/, const LinearWeight& w, hipStream_t st);
int    u4_g32_splits(int K, int N, int M, int want);  // the split-K depth launch_linear_u4_g32 runs for `want` (0: its heuristic), given a workspace
// workspace: 16 fp32 slabs [M][N] (gemm_workspace_bytes(M, N, 16)) or nullptr = one slice.  A split launch is reduced by the launcher:
// y always holds the finished fp16 result
int    launch_linear_u4_g32(const LinearWeight& w, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated_silu, int splits,
                            float* workspace, hipStream_t st);

// ---- comm_p2p.hip: fused one-shot all-reduce + residual + RMSNorm over peer-mapped buffers (TM_COMM=native) ------------
int launch_p2p_allreduce_norm(half_t* const* data, uint32_t* const* flags, int tp, int me, uint32_t* state, size_t tile,
                              const half_t* partial, half_t* y, half_t* resid, const half_t* weight, float eps, int M, int H,
                              hipStream_t st);
// two-shot form (reduce-scatter, norm on the owned row slice, all-gather by push) for messages of MBs; region = fp16 elements of
// one in2 / out2 region; the residual stream is updated for the rank's own slice only
int launch_p2p_allreduce_norm_2shot(half_t* const* in2, half_t* const* out2, uint32_t* const* flags, int tp, int me, uint32_t* state,
                                    size_t region, const half_t* partial, half_t* y, half_t* resid, const half_t* weight, float eps, int M,
                                    int H, hipStream_t st);
int launch_p2p_allreduce_norm_rows(half_t* const* rdata, uint32_t* const* rflags, int rows_cap, int tp, int me, uint32_t* state, size_t tile,
                                   const half_t* partial, half_t* y, half_t* resid, const half_t* weight, float eps, int M, int H, hipStream_t st);
void p2p_timeout_cap_ms(long ms);  // > 0: cap the peer-wait bound (bring-up self-test); 0: TM_P2P_TIMEOUT_MS again
int p2p_allreduce_capacity(int threads, bool one_vec);  // token rows per launch: workgroups resident at once on this device
// dst_stride_words: 32-bit words between the destinations of consecutive ranks (0 = words: dst is [tp][words])
int launch_p2p_allgather(half_t* const* data, uint32_t* const* flags, int tp, int me, uint32_t* state, size_t tile, const void* src,
                         void* dst, int words, hipStream_t st, size_t dst_stride_words = 0);

// sampling.hip: temperature / top-k / top-p / min-p sampling without a sort (see the file header)
size_t sample_workspace_bytes(int batch);
// logprobs of the kept candidates next to the draw (sample_logprobs_kernel): record r = (*step) * step_stride + (row0 + b) * row_stride
// of vals / idx ([records][cap]), num / sel ([records]); step == nullptr: 0; records of steps >= max_steps are dropped
constexpr int kMaxLogProb = 1024;  // = TM_MAX_LOGPROBS (src/turbomind/utils/constant.h:7)
struct SampleLogprobs {
    float*     vals;
    int*       idx;
    int*       num;
    float*     sel;
    int        cap;
    const int* step;
    int        step_stride, row_stride, row0, max_steps;
};
int    launch_sample(int* out_ids, int* kept_out, const half_t* logits, int batch, int V, int ld, const float* temperature,
                     const int* top_k, const float* top_p, const float* min_p, const float* uniform, void* workspace,
                     hipStream_t st, const SampleLogprobs* lp = nullptr);
int    launch_sample_uniform(float* u, const uint64_t* seeds, const int* counters, int batch, hipStream_t st);
float  philox_uniform_host(uint64_t seed, uint32_t ctr);

// logits processors (sampling.hip): persistent per-slot "token seen" bitmask, repetition penalty, banned ids,
// min-length ban of the end ids.  ban = [batch][kMaxBadIds], end = [batch][kMaxEndIds], padded with -1.
constexpr int kMaxBadIds = 32;  // = TM_MAX_BAD_IDS
constexpr int kMaxEndIds = 9;   // eos id + TM_MAX_STOP_IDS
// active (decode rows only, cu_q == nullptr): rows with active[row] == 0 are skipped
int launch_seen_update(uint32_t* seen, int words, const int* ids, const int* cu_q, int nseq, int n_tokens, int vocab,
                       hipStream_t st, const int* active = nullptr);
int launch_logits_process(half_t* logits, int batch, int V, int ld, int vocab_offset, const uint32_t* seen, int words,
                          const float* rep, const int* ban, const int* end, const int* k_len, const int* min_len,
                          hipStream_t st);

struct MoeBlock {
    int                       hidden = 0, inter = 0, experts = 0, top_k = 0;
    bool                      norm_topk    = true;
    float                     routed_scale = 1.f;
    half_t*                   gate         = nullptr;  // device fp16 [hidden][experts]
    half_t*                   shared_gate  = nullptr;  // device fp16 [hidden] (Qwen2-MoE: the shared expert's sigmoid gate) or nullptr; owned
    std::vector<LinearWeight> w13, w2;                 // per expert: gated (gate_j, up_j)-interleaved [H][2I], [I][H]
    void *                    groups13 = nullptr, *groups2 = nullptr;
    void *                    groups13_p8 = nullptr, *groups2_p8 = nullptr;  // fp8 experts: P8 unit pointers (gemm_fp8.hip)
    // gpt-oss block (all off by default: the block then launches what it always launched); fp16 and MXFP4 experts only
    int                       act       = 0;        // 0 = SiLU: silu(gate) * up; 1 = gpt-oss: clamped gate * sigmoid(1.702 gate) * (1 + up)
    float*                    gate_bias = nullptr;  // device fp32 [experts]: added to the router logits before the top-k; owned
    half_t*                   b13       = nullptr;  // device fp16 [experts][2 * inter], (gate_j, up_j)-interleaved like w13's columns; owned
    half_t*                   b2        = nullptr;  // device fp16 [experts][hidden]: added per routed row in the combine; owned
};
size_t moe_workspace_bytes(const MoeBlock& m, int tokens);
int    moe_prepare(MoeBlock& m, hipStream_t st);
enum : unsigned { kMoeGate = 1, kMoeRoute = 2, kMoeW13 = 4, kMoeW2 = 8, kMoeCombine = 16, kMoeAll = 31 };  // launches of moe_forward
int    moe_forward(const MoeBlock& m, half_t* out, int ldo, const half_t* x, int ldx, int tokens, void* workspace, int* topk_ids_out,
                   float* topk_w_out, hipStream_t st, unsigned stages = kMoeAll, const half_t* shared = nullptr);
void   moe_free(MoeBlock& m);
// mixture of experts (moe.hip, grouped GEMM in gemm_w4a16.hip)
int moe_build_groups(void** d_groups, const LinearWeight* experts, int E, hipStream_t st);
// act (gated only): 0 = SiLU, 1 = gpt-oss with the optional per-expert bias [E][N]; MXFP4 experts and act 1 run in gemm_mxfp4.hip
int launch_linear_grouped(const LinearWeight& proto, const void* d_groups, int E, const half_t* x, int ldx, int x_rows,
                          half_t* y, int ldy, int m_cap, int m_hint, bool gated_silu, const int* seg, const int* row_idx,
                          hipStream_t st, int act = 0, const half_t* bias = nullptr);
// gemm_mxfp4.hip: MXFP4 expert weights (blocks uint8 [N][K/2], scales uint8 [N][K/32]) and the gpt-oss gated epilogue
int linear_weight_prepare_mxfp4(LinearWeight& w, const uint8_t* blocks, const uint8_t* scales, hipStream_t st);
int launch_dequant_mxfp4_f16(half_t* out_kn /*[K][N]*/, const LinearWeight& w, hipStream_t st);  // the operand as the GEMM builds it
int launch_linear_grouped_mx(const LinearWeight& proto, const void* d_groups, int E, const half_t* x, int ldx, int x_rows, half_t* y,
                             int ldy, int m_cap, int m_hint, int epilogue /* 0 plain, 1 gated SiLU, 3 gated gpt-oss */,
                             const half_t* bias, const int* seg, const int* row_idx, hipStream_t st);
// bias: fp32 [E] added to the logits before the top-k (nullptr: none, the kernels without the add)
int launch_moe_gate(int* topk_ids, float* topk_w, float* logits_out, const half_t* x, int ldx, const half_t* wg, int T, int H,
                    int E, int k, bool norm_topk, float routed_scale, hipStream_t st, const float* bias = nullptr);
// router choice (TM_MOE_ROUTER): mode -1 = the environment's, 0 = auto (serial kernels up to 64 experts), 1 = wide for every E
void moe_router_override(int mode);
bool moe_router_wide(int E);
int launch_moe_route(int* offsets, int* f2n, int* en2f, const int* topk_ids, int T, int E, int k, hipStream_t st);
int launch_moe_combine(half_t* out, int ldo, const half_t* y, int ldy, const float* topk_w, const int* en2f, int T, int H, int k,
                       hipStream_t st);
// the same with a per-expert bias of the w2 linear: out[t] = fp16( sum_j w[t][j] * f32( h(y[en2f[j][t]] + b2[topk_ids[t][j]]) ) )
int launch_moe_combine_bias(half_t* out, int ldo, const half_t* y, int ldy, const float* topk_w, const int* en2f, const int* topk_ids,
                            const half_t* b2, int T, int H, int k, hipStream_t st);
// the same with a shared expert: out = fp16(f32(shared) * sigmoid(x . gate) + the routed sum); out may alias shared
int launch_moe_combine_shared(half_t* out, int ldo, const half_t* y, int ldy, const float* topk_w, const int* en2f, const half_t* shared,
                              int lds, const half_t* x, int ldx, const half_t* gate, int T, int H, int k, hipStream_t st);

extern uint64_t* g_gemm_dbg;  // gemm_w4a16.hip: optional per-workgroup timing stamps (tm_debug_set_gemm_trace)
// The trace buffer holds kTraceMaxWorkgroups x 8 stamps; a launch with more workgroups is not traced.  (The only unbounded
// device write the library had: a trace buffer sized for one kernel left set while a larger grid ran -- the probable origin of
// the one-off "memory access fault" of a round-2 diagnostic script; tests/test_gpu_fullsize.py::..._with_canaries is clean.)
constexpr size_t kTraceMaxWorkgroups = 8192;
// Arena mode (tm_debug_trace_arena, round 5): every traced launch gets ITS OWN region of a caller-sized buffer, handed out in
// launch order, and a host-side record (tag, grid, offset) -- so that the launches of a captured hipGraph keep distinct regions
// and one replay leaves the stamps of every kernel of the step (tools/fixed_cost_table.py).  Allocation happens on the host at
// launch / capture time; launches that no longer fit are not traced.
struct TraceRecord {
    char   tag[24];
    int    gx, gy, gz;
    size_t offset_wgs;
};
uint64_t* trace_arena_alloc(size_t workgroups, const char* tag, int gx, int gy, int gz);  // nullptr: no arena / full
bool      trace_arena_active();
void      trace_arena_set(uint64_t* base, size_t cap_wgs);
size_t    trace_arena_records(char* out, size_t cap);
inline uint64_t* gemm_trace_for(size_t workgroups, const char* tag = "", int gx = 0, int gy = 0, int gz = 0)
{
    if (trace_arena_active()) {
        return trace_arena_alloc(workgroups, tag, gx, gy, gz);
    }
    return workgroups <= kTraceMaxWorkgroups ? g_gemm_dbg : nullptr;
}

// ---- misc.hip ---------------------------------------------------------------------------
int launch_embedding(half_t* out, const half_t* table, const int* ids, int T, int H, int vocab, hipStream_t st);
// rows with emb_index[t] >= 0 are row emb_index[t] of emb_rows ([n][H] fp16, bit for bit; ids[t] is not read), the others the table's
int launch_embedding_mixed(half_t* out, const half_t* table, const int* ids, const half_t* emb_rows, const int* emb_index, int T, int H,
                           int vocab, hipStream_t st);
int launch_fill_uniform_f16(half_t* out, size_t n, float amp, uint32_t seed, hipStream_t st);  // tuner stand-in activations
int launch_argmax(int* out_ids, half_t* out_val, const half_t* logits, int B, int V, int ld, int id_offset,
                  hipStream_t st);
int launch_gather_rows(half_t* out, const half_t* in, const int* rows, int n, int H, hipStream_t st);

// ---- cross_entropy.hip ------------------------------------------------------------------
// nll[r] = logf(sum exp(x_r - max) + 1e-9f) + max - x_r[targets[r]] over fp16 logits rows [rows][ld] of vocab V (fp32, raw logits);
// targets[r] < 0: 0 (row not read); targets[r] >= V: NaN.  rows == 0: no-op.
int launch_cross_entropy(float* nll, const half_t* logits, const int* targets, int rows, int V, int ld, hipStream_t st);
int launch_silu_mul(half_t* out, const half_t* gate_up, int M, int inter, hipStream_t st);
int launch_quantize_groupwise_u4(int32_t* qweight, half_t* scales, half_t* zeros, half_t* dequant, const half_t* w,
                                 int K, int N, int group, hipStream_t st);

}  // namespace tmk
