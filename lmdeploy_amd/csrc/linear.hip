// The linear formats, in one table (host code only: this file emits no kernel).  One row per LinearFormat says which staging parts a
// checkpoint fills and how large they are, how the GEMM input is quantised in front of the launch, and what the weight weighs;
// linear_weight_prepare is the one switch from a format to the repack that builds its device image(s).  The engine, the operator handles
// of c_api.hip and the MoE block go through the functions below and know no format themselves: a new format is a row and a case here, its
// repack and GEMM kernels in a kernel file of their own, and its creation-time argument checks.
// (reference: LinearWeight::prepare, models/linear_weight.cc:101-324; LlamaLinear.cu:67-127)
#include "../../include/tm_mi355x.h"
#include "tm_common.h"
#include "tm_kernels.h"

namespace tmk {

namespace {

struct FormatRow {
    struct {
        const char* suffix;  // staging part (boundary layout); unused ones stay nullptr
        PartKind    kind;
        size_t (*bytes)(int K, int N, int group);
    } part[3];
    ActQuant    quant;      // quantisation of the GEMM input in front of the format's matrix-core kernel
    const char* needs_act;  // error text of a launch without activation buffers; nullptr: a weight-only image runs without them
    size_t (*bytes)(int K, int N);  // algorithmic size: codes + scales as the checkpoint carries them
};

using PK = PartKind;
constexpr const char* kNoFp8Act = "internal: channel-scaled fp8 linear without its activation buffers";
constexpr const char* kNoMxAct  = "internal: mxfp4 dense linear without its activation buffers";
constexpr const char* kNoI8Act  = "internal: int8 linear without its activation buffers";
size_t mx_codes(int K, int N, int) { return (size_t)N * (K / 2); }    // the checkpoint layout: e2m1 codes [N][K/2] ...
size_t mx_scales(int K, int N, int) { return (size_t)N * (K / 32); }  // ... + one ue8m0 byte per 32 k [N][K/32]
size_t e4m3_codes(int K, int N, int) { return (size_t)K * N; }  // (int8 codes too: one byte each)
size_t col_scales(int, int N, int) { return (size_t)N * 4; }
size_t sz_u4(int K, int N, int g) { return (size_t)(K / g) * N * 2; }  // fp16 [K/group][N]

const FormatRow kFormats[] = {  // index = LinearFormat
    // U4: AWQ int32 [K][N/8] + fp16 scales / zeros
    {{{"qweight", PK::AWQ_QWEIGHT, [](int K, int N, int) { return (size_t)K * N / 2; }}, {"scales", PK::AWQ_SCALES, sz_u4}, {"zeros", PK::AWQ_ZEROS, sz_u4}},
     ActQuant::NONE, nullptr, [](int K, int N) { return (size_t)K * N / 2 + (size_t)(K / 128) * N * 4; }},
    // F16: fp16 [K][N]
    {{{"weight", PK::F16, [](int K, int N, int) { return (size_t)K * N * 2; }}},
     ActQuant::NONE, nullptr, [](int K, int N) { return (size_t)K * N * 2; }},
    // FP8_BLOCK: e4m3 [K][N] + fp32 128 x 128 block scales (weight_format.py:349-393); counted with the scales expanded per column
    {{{"weight", PK::E4M3, e4m3_codes}, {"scales", PK::F32_SCALES, [](int K, int N, int) { return (size_t)(K / 128) * ((N + 127) / 128) * 4; }}},
     ActQuant::FP8_ROW128, nullptr, [](int K, int N) { return (size_t)K * N + (size_t)(K / 128) * N * 4; }},
    // FP8_CHANNEL: e4m3 [K][N] + one fp32 scale per output column (those of a fused linear concatenated / interleaved like its columns)
    {{{"weight", PK::E4M3, e4m3_codes}, {"scales", PK::F32_SCALES, col_scales}},
     ActQuant::FP8_TOKEN, kNoFp8Act, [](int K, int N) { return (size_t)K * N + (size_t)N * 4; }},
    // MXFP4_EXPERT: weight-only grouped GEMM
    {{{"blocks", PK::E2M1, mx_codes}, {"scales", PK::UE8M0, mx_scales}},
     ActQuant::NONE, nullptr, [](int K, int N) { return (size_t)K * N / 2 + (size_t)(K / 128) * N * 4; }},
    // MXFP4_DENSE: the same parts; W4A4 on the block-scaled FP4 matrix cores
    {{{"blocks", PK::E2M1, mx_codes}, {"scales", PK::UE8M0, mx_scales}},
     ActQuant::MXFP4_ROW32, kNoMxAct, [](int K, int N) { return (size_t)K * N / 2 + (size_t)N * (K / 32); }},
    // INT8_CHANNEL: int8 [K][N] + one fp32 scale per output column (fused linears as FP8_CHANNEL); W8A8 on the int8 matrix cores
    {{{"weight", PK::I8, e4m3_codes}, {"scales", PK::F32_SCALES, col_scales}},
     ActQuant::INT8_TOKEN, kNoI8Act, [](int K, int N) { return (size_t)K * N + (size_t)N * 4; }},
    // U4_G32: the parts of U4 sized with group 32 (compressed-tensors pack-quantized); weight-only on a kernel of its own (gemm_u4_g32.hip)
    {{{"qweight", PK::AWQ_QWEIGHT, [](int K, int N, int) { return (size_t)K * N / 2; }}, {"scales", PK::AWQ_SCALES, sz_u4}, {"zeros", PK::AWQ_ZEROS, sz_u4}},
     ActQuant::NONE, nullptr, [](int K, int N) { return (size_t)K * N / 2 + (size_t)(K / 32) * N * 4; }},
};
static_assert(sizeof(kFormats) / sizeof(kFormats[0]) == (size_t)LinearFormat::COUNT, "one row per LinearFormat, in its order");

const FormatRow& row_of(LinearFormat fmt) { return kFormats[(int)fmt]; }

}  // namespace

LinearFormat linear_format(int weight_type, int fp8_scale_mode, bool expert, int group)
{
    return weight_type == TM_WEIGHT_F16   ? LinearFormat::F16 :
           weight_type == TM_WEIGHT_FP8   ? (fp8_scale_mode == 1 ? LinearFormat::FP8_CHANNEL : LinearFormat::FP8_BLOCK) :
           weight_type == TM_WEIGHT_MXFP4 ? (expert ? LinearFormat::MXFP4_EXPERT : LinearFormat::MXFP4_DENSE) :
           weight_type == TM_WEIGHT_I8    ? LinearFormat::INT8_CHANNEL :
           group == 32                    ? LinearFormat::U4_G32 :
                                            LinearFormat::U4;
}

LinearStaging linear_staging(LinearFormat fmt, int K, int N, int group)
{
    LinearStaging s;
    for (const auto& p : row_of(fmt).part) {
        if (p.suffix) {
            s.suffix[s.n] = p.suffix, s.kind[s.n] = p.kind, s.bytes[s.n++] = p.bytes(K, N, group);
        }
    }
    return s;
}

ActQuant linear_act_quant(LinearFormat fmt, bool have_act_buffers)
{
    return row_of(fmt).needs_act || have_act_buffers ? row_of(fmt).quant : ActQuant::NONE;
}

int linear_weight_prepare(LinearWeight& w, const void* const* p, hipStream_t st, bool p32_only, bool f16_image)
{
    switch (w.fmt) {
        case LinearFormat::U4: {
            const int rc = linear_weight_prepare_u4(w, (const int32_t*)p[0], (const half_t*)p[1], (const half_t*)p[2], st, p32_only);
            return rc || !f16_image || !w.packed32 ? rc : linear_weight_build_f16_image(w, st);
        }
        case LinearFormat::F16: return linear_weight_prepare_f16(w, (const half_t*)p[0], st);
        case LinearFormat::FP8_BLOCK: return linear_weight_prepare_fp8(w, (const uint8_t*)p[0], (const float*)p[1], w.gated, st);
        case LinearFormat::FP8_CHANNEL: return linear_weight_prepare_fp8_channel(w, (const uint8_t*)p[0], (const float*)p[1], st);
        case LinearFormat::MXFP4_EXPERT: return linear_weight_prepare_mxfp4(w, (const uint8_t*)p[0], (const uint8_t*)p[1], st);
        case LinearFormat::MXFP4_DENSE: return linear_weight_prepare_mxfp4_dense(w, (const uint8_t*)p[0], (const uint8_t*)p[1], st);
        case LinearFormat::INT8_CHANNEL: return linear_weight_prepare_int8(w, (const uint8_t*)p[0], (const float*)p[1], st);
        case LinearFormat::U4_G32: return linear_weight_prepare_u4_g32(w, (const int32_t*)p[0], (const half_t*)p[1], (const half_t*)p[2], st);
        default: break;
    }
    TM_REQUIRE(false, "internal: linear format without a prepare case");
}

bool linear_weight_prepared(const LinearWeight& w) { return w.packed || w.packed32 || w.packed8; }

bool linear_own_tiling(LinearFormat fmt, bool have_act_buffers)
{
    return fmt == LinearFormat::U4_G32 || linear_act_quant(fmt, have_act_buffers) != ActQuant::NONE;
}

void linear_weight_take(LinearWeight& dst, LinearWeight& src)
{
    dst        = src;
    src.packed = src.packed32 = src.packed8 = nullptr;
    src.sz = nullptr, src.cscale = nullptr, src.image16 = nullptr;
}

size_t linear_weight_bytes(const LinearWeight& w) { return linear_weight_prepared(w) ? row_of(w.fmt).bytes(w.K, w.N) : 0; }

int linear_forward(const LinearWeight& w, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated_silu, const LinearScratch& s,
                   bool defer, int* slabs, hipStream_t st)
{
    const bool     have = s.xq && s.sx && M <= s.rows;
    const ActQuant q    = linear_act_quant(w.fmt, have);
    int            nslab = 1, rc;
    if (w.fmt == LinearFormat::U4_G32) {
        // one tile per M class, the launcher's own split-K and reduce: y holds the finished result, nothing is deferred
        rc = launch_linear_u4_g32(w, x, ldx, y, ldy, M, gated_silu, s.splits, gemm_workspace_bytes(M, w.N, 16) <= s.ws_bytes ? s.ws : nullptr, st);
    }
    else if (q == ActQuant::NONE) {
        GemmConfig cfg = gemm_pick_config(w, M);
        cfg.splits     = gemm_workspace_bytes(M, w.N, cfg.splits) > s.ws_bytes ? 1 : cfg.splits;
        cfg.tickets    = s.tickets;
        defer          = defer && cfg.splits > 1;
        // (not deferred: launch_linear would report the slabs it reduced itself)
        rc = launch_linear(w, x, ldx, y, ldy, M, gated_silu, cfg, s.ws, defer, defer ? &nslab : nullptr, st);
    }
    else {
        // The GEMM input is quantised into the caller's code / scale buffers, then the format's matrix-core kernel runs, for every M --
        // one tile choice per M class, nothing to pick from a table.  Split-K slabs are written scaled (int8: raw, and reduced by its launcher).
        TM_REQUIRE(have, row_of(w.fmt).needs_act);  // (a format that quantises without them needs them)
        float* const ws = gemm_workspace_bytes(M, w.N, 16) <= s.ws_bytes ? s.ws : nullptr;  // room for the launcher's 16 slabs, or one slice
        if (q == ActQuant::INT8_TOKEN) {
            rc = launch_quant_int8_token((uint8_t*)s.xq, (float*)s.sx, x, ldx, M, w.K, st);
            rc = rc ? rc : launch_linear_int8(w, (const uint8_t*)s.xq, (const float*)s.sx, y, ldy, M, gated_silu, s.splits, ws, st);
        }
        else if (q == ActQuant::MXFP4_ROW32) {
            rc = launch_quant_mxfp4_rows((uint8_t*)s.xq, (uint8_t*)s.sx, x, ldx, M, w.K, st);
            rc = rc ? rc : launch_linear_mxfp4(w, (const uint8_t*)s.xq, (const uint8_t*)s.sx, y, ldy, M, gated_silu, s.splits, ws, &nslab, st);
        }
        else {
            rc = q == ActQuant::FP8_TOKEN ? launch_quant_fp8_token((uint8_t*)s.xq, (float*)s.sx, x, ldx, M, w.K, st) :
                                            launch_quant_fp8_rows((uint8_t*)s.xq, (float*)s.sx, x, ldx, M, w.K, s.ldsx, st);
            rc = rc ? rc : launch_linear_fp8(w, (const uint8_t*)s.xq, (const float*)s.sx, s.ldsx, y, ldy, M, gated_silu, s.splits, ws, &nslab, st);
        }
        if (rc == 0 && nslab > 1 && !defer) {
            rc    = launch_splitk_reduce(y, ldy, ws, nslab, M, w.N, gated_silu, st);
            nslab = 1;
        }
    }
    if (slabs) {
        *slabs = nslab;
    }
    return rc;
}

}  // namespace tmk
