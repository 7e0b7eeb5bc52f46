// W4A16 linear with quantisation groups of 32 along K (compressed-tensors `pack-quantized`, group_size 32) on the CDNA4 matrix cores
// (v_mfma_f32_32x32x16_f16).  The group-128 kernels (gemm_decode.hip, gemm_prefill.hip, gemm_w4a16.hip) bake 128 into their images and
// stay as they are; this file is the whole of LinearFormat::U4_G32: repack, GEMM, debug read-back.
//
// Replaces: the reference's int4 GEMM family at group_size 32 (CompressedTensorFormat, lmdeploy/turbomind/weight_format.py:294-346;
//           _SUPPORTED_GROUP_SIZES, converter.py:86-92; kernels/gemm/transform.h:68-74 for the dequantisation).
// Arithmetic, as for U4 (oracle.w4a16_dequant / w4a16_linear / w4a16_linear_gated_silu with group = 32):
//   w[k, n] = h(fma(h(q), s, h(-z * s)))  with (s, z) of group k / 32 -- h(-z * s) rounded once at load time, the fma one packed fp16 fma;
//   y[m, n] = h(sum_k x[m, k] * w[k, n])  fp16 x fp16 products summed in fp32 on the matrix core, one rounding to fp16 (or the gated-SiLU
//   epilogue h(silu(a_2j) * a_2j+1) on the fp32 sums of the interleaved (gate_j, up_j) columns).
//
// Image ("G32"): units of 32 columns x 128 k, unit (kb, cg) at (kb * N / 32 + cg) * 2560 bytes, k-block major like the P32 / P8 images:
//   bytes [0, 2048)     codes: two 1-KiB vectors v; lane l = 32 hf + c (column c of the unit, lane half hf) owns 16 bytes at v * 1024 + l * 16,
//                       dword d of them is the lane's A operand of MFMA k-step 4v + d: the 8 codes k = 128 kb + 16 (4v + d) + 8 hf + e,
//                       e = 0..7, with e = 2i in nibble i and e = 2i + 1 in nibble i + 4 -- so (word >> 4i) & 0x000f000f | 0x64006400 is the
//                       fp16 pair (1024 + q[2i], 1024 + q[2i + 1]), fragment register i, and 1024 is taken off exactly;
//   bytes [2048, 2560)  pairs: column c owns 16 bytes at 2048 + c * 16 = the four half2 (s, h(-z * s)) of groups 4 kb + 0..3.  Every 16-k
//                       MFMA step lies inside one group (steps 2g and 2g + 1 are group g of the k-block), so a step's dequantisation is
//                       four packed fmas with one per-column constant pair.
// Lane map of the GEMM: the WEIGHTS are the A operand (lane l: row = column c = l & 31 of the unit, k = 8 (l >> 5) + e), x is the B operand
//   (lane l: column = x row 32 h + (l & 31), the same k), so D has the x row on the lane and the weight columns in the registers:
//   register r = column (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the unit.  A lane therefore owns runs of four adjacent output columns of one x
//   row -- whole (gate, up) pairs for the gated epilogue, an 8-byte fp16 store otherwise.
// Workgroup: 4 waves = 4 column units (128 columns) x 32 MH rows (MH = 1, 2: the decode tile, M <= 64; MH = 4: 128-row tiles above it), every
//   wave on its own unit over the whole k-slice.  Weights stream HBM -> registers (three 16-byte buffer loads per lane and k-block); the
//   tile's x rows of a k-block (32 MH x 256 bytes) are fetched once per workgroup by buffer loads into registers and staged in LDS, rows
//   padded to 272 bytes so that 16 lanes' ds_read_b128 of one k-step fall on 64 distinct banks.  One stage, two barriers per k-block: the
//   loads of k-block i + 1 (x and weights) are issued right behind the second barrier and stay in flight under the MFMAs of k-block i
//   (the compiler's counted vmcnt waits; no FLAT access anywhere).  Rows past M are clamped re-reads that are never stored; the buffer
//   descriptors are sized to the image and to the tile's x rows.
// Split-K (grid.y): slices write fp32 slabs [slice][M][N] and this file's launcher runs the reduce (the shared fp32 reduce kernel, the same
//   epilogue expressions), so y always holds the finished fp16 result: no slab goes on to a norm or an attention prologue.
#include "tm_common.h"
#include "tm_kernels.h"
#include <algorithm>

namespace tmk {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kG32Unit = 2048 + 512;

size_t g32_bytes(int K, int N)
{
    return (size_t)(K / 128) * (N / 32) * kG32Unit;
}

// the A operand of one 16-k step: four fp16 pairs of dequantised weights from one code dword and the column's (s, h(-z s)) pair
__device__ __forceinline__ half8_t g32_dequant_word(uint32_t word, uint32_t pair)
{
    const half2_t sz = bit_cast<half2_t>(pair);
    const half2_t s2 = {sz[0], sz[0]}, zs2 = {sz[1], sz[1]};
    const half2_t k1024 = {(half_t)1024.f, (half_t)1024.f};
    half8_t       a;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const half2_t hq = bit_cast<half2_t>(((word >> (4 * i)) & 0x000f000fu) | 0x64006400u) - k1024;  // h(q), exact
        const half2_t w  = h2_fma(hq, s2, zs2);
        a[2 * i]         = w[0];
        a[2 * i + 1]     = w[1];
    }
    return a;
}

// ---- load-time repack: one thread per dword of the image ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void repack_g32_kernel(uint32_t* __restrict__ out, const int32_t* __restrict__ qw /*[K][N/8]*/,
                                                         const half_t* __restrict__ scales /*[K/32][N]*/, const half_t* __restrict__ zeros,
                                                         int K, int N)
{
    const size_t idx   = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)(K / 128) * (N / 32) * (kG32Unit / 4);
    if (idx >= total) {
        return;
    }
    const int    ncg  = N / 32;
    const size_t unit = idx / (kG32Unit / 4);
    const int    r    = (int)(idx % (kG32Unit / 4));
    const int    kb   = (int)(unit / ncg);
    const int    cg   = (int)(unit % ncg);
    if (r < 512) {
        const int v = r >> 8, l = (r >> 2) & 63, d = r & 3;
        const int col = cg * 32 + (l & 31);
        const int k0  = kb * 128 + 16 * (4 * v + d) + 8 * (l >> 5);
        uint32_t  w   = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint32_t q = ((uint32_t)qw[(size_t)(k0 + e) * (N / 8) + col / 8] >> (4 * (col & 7))) & 15u;
            w |= q << (4 * ((e >> 1) + 4 * (e & 1)));
        }
        out[idx] = w;
    }
    else {
        const int    c = (r - 512) >> 2, g = (r - 512) & 3;
        const size_t i = (size_t)(kb * 4 + g) * N + cg * 32 + c;
        const half_t s = scales[i];
        const half_t z = zeros[i];
        const half2_t pr = {s, (half_t)((-z) * s)};  // one fp16 rounding (cast.cu:151-156), as repack_sz_kernel
        out[idx]         = bit_cast<uint32_t>(pr);
    }
}

int linear_weight_prepare_u4_g32(LinearWeight& w, const int32_t* qweight, const half_t* scales, const half_t* zeros, hipStream_t st)
{
    TM_REQUIRE(w.group == 32, "u4 group-32 linear: group_size 32");
    TM_REQUIRE(w.K % 128 == 0 && w.N % 32 == 0 && g32_bytes(w.K, w.N) < ((size_t)1 << 31),
               "u4 group-32 linear " + std::to_string(w.K) + " x " + std::to_string(w.N) + ": K % 128 == 0, N % 32 == 0 and an image below 2^31 bytes");
    TM_REQUIRE(!w.packed && !w.packed32, "u4 group-32 linear: the handle already holds a weight of another format");
    w.type          = 0;
    w.packed8_bytes = g32_bytes(w.K, w.N);
    if (!w.packed8) {
        TM_HIP_CHECK(hipMalloc(&w.packed8, w.packed8_bytes));
    }
    const size_t nd = w.packed8_bytes / 4;
    repack_g32_kernel<<<(unsigned)((nd + 255) / 256), 256, 0, st>>>((uint32_t*)w.packed8, qweight, scales, zeros, w.K, w.N);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

bool u4_g32_prepared(const LinearWeight& w)
{
    return w.fmt == LinearFormat::U4_G32 && w.type == 0 && w.group == 32 && w.packed8 != nullptr;
}

// ---- debug read-back: the fp16 [N][K] operand rebuilt from the image with the GEMM's own dequantisation -----------------------------
__global__ __launch_bounds__(256) void dequant_g32_kernel(half_t* __restrict__ out /*[N][K]*/, const uint32_t* __restrict__ img, int K, int N)
{
    const size_t idx   = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)(K / 128) * (N / 32) * 512;
    if (idx >= total) {
        return;
    }
    const int    ncg  = N / 32;
    const size_t unit = idx / 512;
    const int    r    = (int)(idx % 512);
    const int    kb   = (int)(unit / ncg);
    const int    cg   = (int)(unit % ncg);
    const int    v = r >> 8, l = (r >> 2) & 63, d = r & 3;
    const int    step = 4 * v + d;
    const uint32_t* u = img + unit * (kG32Unit / 4);
    const half8_t   a = g32_dequant_word(u[r], u[512 + (l & 31) * 4 + (step >> 1)]);
    const int col = cg * 32 + (l & 31);
    const int k0  = kb * 128 + 16 * step + 8 * (l >> 5);
    *(half8_t*)(out + (size_t)col * K + k0) = a;
}

int launch_dequant_g32_f16(half_t* out_nk, const LinearWeight& w, hipStream_t st)
{
    TM_REQUIRE(u4_g32_prepared(w), "fp16 image: a u4 group-32 linear with its image");
    const size_t nd = (size_t)(w.K / 128) * (w.N / 32) * 512;
    dequant_g32_kernel<<<(unsigned)((nd + 255) / 256), 256, 0, st>>>(out_nk, (const uint32_t*)w.packed8, w.K, w.N);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- GEMM -----------------------------------------------------------------------------------------------------------------------
struct G32Params {
    const half_t* x;  // [M][ldx]
    int           ldx;
    const void*   wp;  // G32 units
    half_t*       y;
    int           ldy;
    float*        partial;  // [splits][M][N] fp32 slabs
    int           M, N, K, KB, ncg;
    int           kb_per_split;
    int           epilogue;  // 0 fp16, 1 gated SiLU fp16, 2 fp32 slab of split blockIdx.y
};

constexpr int kG32XRow = 256 + 16;  // LDS bytes of one x row of a k-block: 128 fp16 + 16 bytes, so 16 lanes' ds_read_b128 hit 64 distinct banks

template<int MH>
__global__ __launch_bounds__(256) void gemm_u4_g32_kernel(G32Params p)
{
    constexpr int ROWS = 32 * MH;
    constexpr int NX   = ROWS * 16 / 256;  // 16-byte pieces of the x stage per thread
    __shared__ __attribute__((aligned(16))) char xs[ROWS * kG32XRow];

    const int  tid   = threadIdx.x;
    const int  lane  = tid & 63;
    const int  wave  = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int  l31   = lane & 31;
    const int  half  = lane >> 5;
    const int  cg    = blockIdx.x * 4 + wave;
    const bool live  = cg < p.ncg;           // wave-uniform; a wave past the last unit keeps the barriers and stores nothing
    const int  cgc   = min(cg, p.ncg - 1);
    const int  m0    = blockIdx.z * ROWS;
    const int  Mloc  = min(ROWS, p.M - m0);
    const int  kb0   = blockIdx.y * p.kb_per_split;
    const int  nkb   = min(p.kb_per_split, p.KB - kb0);

    const half_t* xt   = p.x + (size_t)m0 * p.ldx;  // the tile's rows: offsets below stay far from 2^31
    const auto    rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.wp, 0, p.KB * p.ncg * kG32Unit, 0x00020000);
    const auto    rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)xt, 0, ((Mloc - 1) * p.ldx + p.K) * 2, 0x00020000);

    // x stage of one k-block: ROWS rows x 256 bytes, piece c = tid + 256 j = row c / 16 (clamped past the tile's rows), 16-byte unit c % 16
    int xg[NX], xl[NX];
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        const int c = tid + 256 * j;
        xg[j]       = min(c >> 4, Mloc - 1) * p.ldx * 2 + (c & 15) * 16;
        xl[j]       = (c >> 4) * kG32XRow + (c & 15) * 16;
    }
    floatx16 acc[MH];
#pragma unroll
    for (int h = 0; h < MH; ++h) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[h][r] = 0.f;
        }
    }

    auto load_unit = [&](int i, u32x4& c0, u32x4& c1, u32x4& pr) {
        const int uo = ((kb0 + min(i, nkb - 1)) * p.ncg + cgc) * kG32Unit;
        c0 = __builtin_amdgcn_raw_buffer_load_b128(rs_w, lane * 16, uo, 0);
        c1 = __builtin_amdgcn_raw_buffer_load_b128(rs_w, 1024 + lane * 16, uo, 0);
        pr = __builtin_amdgcn_raw_buffer_load_b128(rs_w, 2048 + l31 * 16, uo, 0);
    };
    auto load_x = [&](int i, u32x4 (&xr)[NX]) {
        const int kbyte = (kb0 + min(i, nkb - 1)) * 256;
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            xr[j] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xg[j], kbyte, 0);
        }
    };
    u32x4 c0, c1, pr, xr[NX];
    load_x(0, xr);
    load_unit(0, c0, c1, pr);
    const char* const xb = xs + l31 * kG32XRow + half * 16;  // the lane's B piece of k-step 0, row block 0
    for (int i = 0; i < nkb; ++i) {
        __syncthreads();  // every wave has read stage i - 1
#pragma unroll
        for (int j = 0; j < NX; ++j) {
            *(u32x4*)(xs + xl[j]) = xr[j];
        }
        __syncthreads();
        u32x4 n0, n1, npr;
        load_x(i + 1, xr);  // in flight under the MFMAs (the last iteration re-reads its own k-block)
        load_unit(i + 1, n0, n1, npr);
#pragma unroll
        for (int step = 0; step < 8; ++step) {
            const half8_t a = g32_dequant_word(step < 4 ? c0[step & 3] : c1[step & 3], pr[step >> 1]);
#pragma unroll
            for (int h = 0; h < MH; ++h) {
                const half8_t b = *(const half8_t*)(xb + h * 32 * kG32XRow + step * 32);
                acc[h]          = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[h], 0, 0, 0);
            }
        }
        c0 = n0, c1 = n1, pr = npr;
    }
    if (!live) {
        return;
    }

#pragma unroll
    for (int h = 0; h < MH; ++h) {
        const int m = 32 * h + l31;
        if (m >= Mloc) {
            continue;
        }
        const size_t mg = (size_t)m0 + m;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int     n = cg * 32 + 8 * g4 + 4 * half;
            const floatx4 a = {acc[h][4 * g4], acc[h][4 * g4 + 1], acc[h][4 * g4 + 2], acc[h][4 * g4 + 3]};
            if (p.epilogue == 2) {
                *(floatx4*)(p.partial + ((size_t)blockIdx.y * p.M + mg) * p.N + n) = a;
            }
            else if (p.epilogue == 1) {  // the expressions of splitk_reduce_kernel: a split and an unsplit launch agree on equal sums
                const float s0 = a[0] / (1.0f + __builtin_expf(-a[0]));
                const float s1 = a[2] / (1.0f + __builtin_expf(-a[2]));
                const half2_t o = {(half_t)(s0 * a[1]), (half_t)(s1 * a[3])};
                *(half2_t*)(p.y + mg * p.ldy + (n >> 1)) = o;
            }
            else {
                const half4_t o = {(half_t)a[0], (half_t)a[1], (half_t)a[2], (half_t)a[3]};
                *(half4_t*)(p.y + mg * p.ldy + n) = o;
            }
        }
    }
}

// the split-K depth of a launch: `want` if > 0, else enough slices for two workgroups per CU; then evened out over the k-blocks
int u4_g32_splits(int K, int N, int M, int want)
{
    const int KB = K / 128, rows_per = M <= 32 ? 32 : M <= 64 ? 64 : 128;
    const int col_wgs = (N / 32 + 3) / 4 * ((M + rows_per - 1) / rows_per);
    int       sp      = want > 0 ? want : (512 + col_wgs - 1) / col_wgs;
    sp                = std::max(1, std::min(sp, std::min(16, KB)));
    const int per     = (KB + sp - 1) / sp;
    return (KB + per - 1) / per;
}

// y[M][N (N / 2 gated)] = x . W.  splits = 0: the heuristic; workspace = room for 16 fp32 slabs [M][N], or nullptr: one slice.  A split
// launch is reduced here; y always holds the result.
int launch_linear_u4_g32(const LinearWeight& w, const half_t* x, int ldx, half_t* y, int ldy, int M, bool gated_silu, int splits,
                         float* workspace, hipStream_t st)
{
    TM_REQUIRE(u4_g32_prepared(w), "u4 group-32 linear: a weight prepared by linear_weight_prepare_u4_g32");
    TM_REQUIRE(splits >= 0 && splits <= 16, "u4 group-32 linear: 0 <= splits <= 16");
    TM_REQUIRE(ldx % 8 == 0 && ldx >= w.K && ldy % 4 == 0 && ((size_t)x & 15) == 0 && ((size_t)y & 7) == 0,
               "u4 group-32 linear: 16-byte aligned x rows (ldx % 8 == 0, ldx >= K), 8-byte aligned y rows (ldy % 4 == 0)");
    if (M == 0) {
        return 0;
    }
    TM_REQUIRE((size_t)127 * ldx * 2 + (size_t)w.K * 2 < ((size_t)1 << 31), "u4 group-32 linear: 128 rows of x reach 2^31 bytes");
    G32Params p{};
    p.x = x, p.ldx = ldx, p.wp = w.packed8, p.y = y, p.ldy = ldy, p.partial = workspace;
    p.M = M, p.N = w.N, p.K = w.K, p.KB = w.K / 128, p.ncg = w.N / 32;
    const int rows_per = M <= 32 ? 32 : M <= 64 ? 64 : 128;
    const int zb       = (M + rows_per - 1) / rows_per;
    TM_REQUIRE(zb <= 65535, "u4 group-32 linear: row blocks exceed grid.z (65535): split the forward into fewer tokens");
    const int sp   = workspace ? u4_g32_splits(w.K, w.N, M, splits) : 1;
    p.kb_per_split = (p.KB + sp - 1) / sp;
    p.epilogue     = sp > 1 ? 2 : (gated_silu ? 1 : 0);
    const dim3 grid((p.ncg + 3) / 4, sp, zb);
    if (rows_per == 32) {
        gemm_u4_g32_kernel<1><<<grid, 256, 0, st>>>(p);
    }
    else if (rows_per == 64) {
        gemm_u4_g32_kernel<2><<<grid, 256, 0, st>>>(p);
    }
    else {
        gemm_u4_g32_kernel<4><<<grid, 256, 0, st>>>(p);
    }
    TM_HIP_CHECK(hipGetLastError());
    return sp > 1 ? launch_splitk_reduce(y, ldy, workspace, sp, M, w.N, gated_silu, st) : 0;
}

}  // namespace tmk
