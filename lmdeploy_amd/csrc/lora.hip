// Multi-LoRA delta for gfx950: y[m] += (x[m] A_a^T) B_a^T for the rows m that carry an adapter a = adapter_of_row[m], added in place to the
// finished fp16 result of a base linear -- ONE launch per linear, both contractions on v_mfma_f32_16x16x32_f16, the rank-sized
// intermediate never leaves the CU.  Up to 8 resident adapters (slots) per linear, rank <= 64 per column segment, up to 3 segments (the
// fused w_qkv: one shrink over the stacked A_q | A_k | A_v, an expand whose q / k / v columns each read their own rank slice).
//
// Arithmetic contract (include/tm_mi355x.h: tm_lora_apply):
//   t[r]    = fp16( sum_k x[m][k] * A[r][k] )                        products exact, sum in fp32, ONE rounding to fp16
//   y[m][n] = fp16( float(y[m][n]) + sum_r float(t[r]) * B[n][r] )   sum in fp32 (r over the rank slice of n's segment), one rounding
//   a row whose id is -1 (or names an empty slot), a column outside every segment, and every byte of y outside [0, N) of a row: not written.
// lora_alpha / r (use_rslora: lora_alpha / sqrt(r)) is folded into B by whoever fills the table; ranks are zero-padded to multiples of 16.
//
// Two kernels:
//   lora_plan_kernel   once per forward: a stable counting sort of the rows by slot (one workgroup, 256 threads, each a contiguous chunk
//                      of rows) -> tiles of 16 rows of ONE slot: plan = { n_tiles | slot[T] | live[T] | rows[T][16] }, T <= M / 16 + 8.
//                      Neither x nor y is ever reordered: the rows reach the MFMA operands through indexed loads and leave through
//                      indexed stores.  A prefill forward hands ids per SEQUENCE and cu_q; the row's sequence is searched in cu_q.
//   lora_delta_kernel  grid (T_max row tiles, ceil(N / NT) column tiles), 256 threads = 4 waves; a workgroup whose tile index is past
//                      n_tiles, or whose slot is empty, leaves at once.
//     shrink  T[16][RT] (RT = the slot's stacked rank, <= 192): the four waves split K in steps of 32 (wave w: steps w, w + 4, ...),
//             every wave holds RT / 16 accumulator tiles; operand lanes, l = lane:
//               a (x)    row l % 16 of the tile,        k = 32 step + 8 (l / 16) .. + 7   one 16-byte indexed load of x
//               b (A)    rank j 16 + l % 16,            the same k run                     one 16-byte load of A [RT][K]
//               d        T[4 (l / 16) + i][j 16 + l % 16], i = 0 .. 3
//             a k run past K (K % 32 == 16) enters as zeros.  The partial tiles go to LDS, are summed over the four waves in fp32 in
//             wave order and rounded ONCE to fp16.
//     expand  wave w owns the 16-column subtiles w, w + 4, ... of the workgroup's NT columns; per subtile (one segment, rank slice
//             [t_off, t_off + R)) the TRANSPOSED product, so that a lane ends up with 4 consecutive columns of one row:
//               a (B)    column n0 + l % 16,            r = 32 step + 8 (l / 16) .. + 7   one 16-byte load of B [N][ldb], straight from
//                                                                                           global memory into the operand registers
//               b (T)    row l % 16 of the tile,        the same r run                     one 16-byte LDS read
//               d        y[row l % 16][n0 + 4 (l / 16) + i]                                one 8-byte indexed load, add, 8-byte store
//     Every column tile of a row tile recomputes the shrink: A is at most 192 x K fp16 and stays in L2, x's 16 rows likewise.
//     No atomics: an element of y has exactly one writer.
//   LDS map (dynamic, RT-sized): [ part: 4 waves x 16 rows x (RT + 4) fp32 | t16: 16 rows x (RT + 8) fp16 ] = 288 RT + 1280 bytes
//     (55.25 KiB at RT = 192, 19.25 KiB at rank 64 one segment, 5.75 KiB at rank 16; RT = the widest filled slot of the table).  The + 4 floats spread the four 4-row groups of a
//     d tile over the 64 banks; the + 8 halves keep the 16-byte reads of t16 aligned and off one bank.
//   NT (columns per workgroup) is 64, 128 or 256 -- the largest that still gives one workgroup per CU (256) from the tiles a dense batch
//     of M rows makes, ceil(M / 16) x ceil(N / NT): a 64-row decode step on N = 4096 runs 4 x 64 workgroups at NT = 64; a prefill forward
//     takes NT = 256 and recomputes the shrink a quarter as often.  Resource report (hipcc -Rpass-analysis=kernel-resource-usage,
//     gfx950): see DESIGN.md 7.15.
#include "tm_kernels.h"
#include <algorithm>

#define TM_TRY_RC(expr)          \
    do {                        \
        const int _rc = (expr); \
        if (_rc) {              \
            return _rc;         \
        }                       \
    } while (0)

namespace tmk {

namespace {

constexpr int kPlanThreads = 256;

// the plan's arrays behind the workspace pointer (T = lora_plan_tiles(M))
struct PlanView {
    int* n_tiles;
    int* slot;
    int* live;
    int* rows;
};
__host__ __device__ inline PlanView plan_view(void* ws, int T)
{
    int* p = (int*)ws;
    return PlanView{p, p + 4, p + 4 + T, p + 4 + 2 * T};
}

__global__ void __launch_bounds__(kPlanThreads) lora_plan_kernel(void* ws, int T, const int* __restrict__ ids, const int* __restrict__ cu_q,
                                                                  int nseq, int M, int nslots)
{
    __shared__ int cnt[kPlanThreads][kLoraMaxSlots + 1];  // per thread and slot: rows counted, then the thread's first position
    __shared__ int total[kLoraMaxSlots], base[kLoraMaxSlots + 1];
    const int tid   = threadIdx.x;
    const int chunk = (M + kPlanThreads - 1) / kPlanThreads;
    const int m0 = tid * chunk, m1 = min(M, m0 + chunk);
    // the slot of row m: ids[m], or ids[sequence of m]; anything outside [0, nslots) counts as none
    auto slot_of = [&](int m, int& seq) {
        int id;
        if (cu_q) {
            while (seq + 1 < nseq && m >= cu_q[seq + 1]) {
                ++seq;
            }
            id = ids[seq];
        }
        else {
            id = ids[m];
        }
        return (unsigned)id < (unsigned)nslots ? id : -1;
    };
    for (int s = 0; s < kLoraMaxSlots; ++s) {
        cnt[tid][s] = 0;
    }
    int seq = 0;
    for (int m = m0; m < m1; ++m) {
        const int s = slot_of(m, seq);
        if (s >= 0) {
            cnt[tid][s] += 1;
        }
    }
    __syncthreads();
    if (tid < kLoraMaxSlots) {  // exclusive prefix over the threads, per slot
        int run = 0;
        for (int t = 0; t < kPlanThreads; ++t) {
            const int c  = cnt[t][tid];
            cnt[t][tid] = run;
            run += c;
        }
        total[tid] = run;
    }
    __syncthreads();
    PlanView pv = plan_view(ws, T);
    if (tid == 0) {
        int b = 0;
        for (int s = 0; s < kLoraMaxSlots; ++s) {
            base[s] = b;
            b += (total[s] + 15) / 16;
        }
        base[kLoraMaxSlots] = b;  // <= M / 16 + 8 <= T
        *pv.n_tiles         = b;
    }
    __syncthreads();
    seq = 0;
    for (int m = m0; m < m1; ++m) {
        const int s = slot_of(m, seq);
        if (s >= 0) {
            const int pos                              = cnt[tid][s]++;
            pv.rows[(base[s] + pos / 16) * 16 + pos % 16] = m;
        }
    }
    for (int t = tid; t < base[kLoraMaxSlots]; t += kPlanThreads) {
        int s = 0;
        while (t >= base[s + 1]) {
            ++s;
        }
        pv.slot[t] = s;
        pv.live[t] = min(16, total[s] - 16 * (t - base[s]));
    }
}

struct DeltaArgs {
    const half_t*       x;
    half_t*             y;
    const LoraTableDev* tab;
    const int*          plan;
    int                 ldx, ldy, K, N, T, nsub;  // nsub: 16-column subtiles per wave (NT = 64 nsub)
    int                 nseg, seg_begin[kLoraMaxSegments], seg_end[kLoraMaxSegments];
};

constexpr int kMaxRankTiles = kLoraMaxSegments * kLoraMaxRank / 16;  // 12

__global__ void __launch_bounds__(256) lora_delta_kernel(const DeltaArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const PlanView pv   = plan_view(const_cast<int*>(p.plan), p.T);
    const int      tile = blockIdx.x;
    if (tile >= *pv.n_tiles) {
        return;
    }
    const LoraSlotDev* const S = &p.tab->slot[pv.slot[tile]];
    const int RT = S->rt;
    if (RT == 0) {  // a row names a slot nothing was loaded into: as if it named none
        return;
    }
    const int live = pv.live[tile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l16 = lane & 15, lq = lane >> 4;
    const int row = l16 < live ? pv.rows[tile * 16 + l16] : -1;
    const int PS = RT + 4, TS = RT + 8;
    float*    part = (float*)lds;                                   // [4][16][PS]
    half_t*   t16  = (half_t*)(lds + (size_t)4 * 16 * PS * 4);      // [16][TS]
    const int ntr  = RT / 16;

    // ---- shrink: this wave's K steps of T = x A^T ----
    floatx4 acc[kMaxRankTiles];
#pragma unroll
    for (int j = 0; j < kMaxRankTiles; ++j) {
        acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const half_t* xrow  = p.x + (size_t)(row < 0 ? 0 : row) * p.ldx;
    // Two K steps in flight: the loads of the wave's next step are issued before the MFMAs of the current one (a step is 1 + RT / 16
    // dependent-free 16-byte loads and as many MFMAs; one step at a time left the wave waiting for memory).  A step past K loads zeros.
    const half_t* const Arow = S->A + (size_t)l16 * p.K;
    auto load = [&](int k0, half8_t& a, half8_t(&b)[kMaxRankTiles]) {
        const int  k  = k0 + 8 * lq;
        const bool in = k < p.K;
        a             = (in && row >= 0) ? *(const half8_t*)(xrow + k) : zero8;
#pragma unroll
        for (int j = 0; j < kMaxRankTiles; ++j) {
            b[j] = (in && j < ntr) ? *(const half8_t*)(Arow + (size_t)j * 16 * p.K + k) : zero8;
        }
    };
    auto mma = [&](const half8_t& a, const half8_t(&b)[kMaxRankTiles]) {
#pragma unroll
        for (int j = 0; j < kMaxRankTiles; ++j) {
            if (j < ntr) {
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b[j], acc[j], 0, 0, 0);
            }
        }
    };
    half8_t a0, a1, b0[kMaxRankTiles], b1[kMaxRankTiles];
    load(wave * 32, a0, b0);
    for (int k0 = wave * 32; k0 < p.K; k0 += 256) {
        load(k0 + 128, a1, b1);
        mma(a0, b0);
        load(k0 + 256, a0, b0);
        mma(a1, b1);
    }
#pragma unroll
    for (int j = 0; j < kMaxRankTiles; ++j) {
        if (j < ntr) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                part[(wave * 16 + 4 * lq + i) * PS + j * 16 + l16] = acc[j][i];
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 16 * RT; e += 256) {
        const int m = e / RT, r = e % RT;
        float     s = part[m * PS + r];
        s += part[(16 + m) * PS + r];
        s += part[(32 + m) * PS + r];
        s += part[(48 + m) * PS + r];
        t16[m * TS + r] = (half_t)s;
    }
    __syncthreads();

    // ---- expand: y^T subtiles = B T^T ----
    for (int j = 0; j < p.nsub; ++j) {
        const int n0 = (blockIdx.y * p.nsub * 4 + j * 4 + wave) * 16;
        if (n0 >= p.N) {
            break;
        }
        int g = -1;
        for (int s = 0; s < p.nseg; ++s) {
            if (n0 >= p.seg_begin[s] && n0 < p.seg_end[s]) {
                g = s;
            }
        }
        const int R = g < 0 ? 0 : S->rank[g];
        if (R == 0) {
            continue;
        }
        const int     toff = S->toff[g];
        const half_t* brow = S->B + (size_t)(n0 + l16) * S->ldb;
        floatx4       d    = {0.f, 0.f, 0.f, 0.f};
        for (int r0 = 0; r0 < R; r0 += 32) {
            const int     r  = r0 + 8 * lq;
            const bool    in = r < R;
            const half8_t a  = in ? *(const half8_t*)(brow + r) : zero8;
            const half8_t b  = in ? *(const half8_t*)(t16 + l16 * TS + toff + r) : zero8;
            d                = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, d, 0, 0, 0);
        }
        if (row >= 0) {
            half4_t* const py = (half4_t*)(p.y + (size_t)row * p.ldy + n0 + 4 * lq);
            half4_t        v  = *py;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = (half_t)((float)v[i] + d[i]);
            }
            *py = v;
        }
    }
}

}  // namespace

size_t lora_plan_workspace_bytes(int M)
{
    const size_t T = (size_t)lora_plan_tiles(M);
    return (4 + 2 * T + 16 * T) * sizeof(int);
}

int launch_lora_plan(void* plan_ws, const int* ids, const int* cu_q, int nseq, int M, int nslots, hipStream_t stream)
{
    TM_REQUIRE(plan_ws && ids, "lora plan: null pointer");
    TM_REQUIRE(M >= 1, "lora plan: M >= 1");
    TM_REQUIRE(nslots >= 1 && nslots <= kLoraMaxSlots, "lora: at most 8 adapter slots");
    TM_REQUIRE(!cu_q || nseq >= 1, "lora plan: cu_q without sequences");
    lora_plan_kernel<<<1, kPlanThreads, 0, stream>>>(plan_ws, lora_plan_tiles(M), ids, cu_q, nseq, M, nslots);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int lora_table_check(const LoraTable& t)
{
    TM_REQUIRE(t.slots >= 1 && t.slots <= kLoraMaxSlots, "lora: at most 8 adapter slots");
    TM_REQUIRE(t.nseg >= 1 && t.nseg <= kLoraMaxSegments, "lora: at most 3 column segments");
    TM_REQUIRE(t.K >= 16 && t.N >= 16 && t.K % 16 == 0 && t.N % 16 == 0, "lora: K and N must be multiples of 16");
    for (int g = 0; g < t.nseg; ++g) {
        TM_REQUIRE(t.seg_begin[g] % 16 == 0 && t.seg_end[g] % 16 == 0 && 0 <= t.seg_begin[g] && t.seg_begin[g] < t.seg_end[g]
                       && t.seg_end[g] <= t.N && (g == 0 || t.seg_begin[g] >= t.seg_end[g - 1]),
                   "lora: column segments must be ascending, disjoint, inside [0, N) and multiples of 16");
    }
    return 0;
}

int lora_slot_check(const LoraTable& t, const int* seg_rank, int ldb, LoraSlotDev* out)
{
    LoraSlotDev s{};
    int         widest = 0;
    for (int g = 0; g < t.nseg; ++g) {
        TM_REQUIRE(seg_rank[g] <= kLoraMaxRank, "lora: rank over 64 per segment");
        TM_REQUIRE(seg_rank[g] >= 0 && seg_rank[g] % 16 == 0, "lora: ranks are zero-padded to multiples of 16");
        s.rank[g] = seg_rank[g];
        s.toff[g] = s.rt;
        s.rt += seg_rank[g];
        widest = std::max(widest, seg_rank[g]);
    }
    TM_REQUIRE(s.rt > 0, "lora: an adapter needs a rank in at least one segment");
    TM_REQUIRE(ldb >= widest && ldb % 8 == 0, "lora: ldb must cover the widest segment rank and be a multiple of 8");
    s.ldb = ldb;
    *out  = s;
    return 0;
}

int lora_table_init(LoraTable& t, int K, int N, int nseg, const int* seg_begin, const int* seg_end, int slots)
{
    TM_REQUIRE(seg_begin && seg_end, "lora: null pointer");
    TM_REQUIRE(nseg >= 1 && nseg <= kLoraMaxSegments, "lora: at most 3 column segments");
    t = LoraTable{};
    t.K = K, t.N = N, t.slots = slots, t.nseg = nseg;
    for (int g = 0; g < nseg; ++g) {
        t.seg_begin[g] = seg_begin[g];
        t.seg_end[g]   = seg_end[g];
    }
    TM_TRY_RC(lora_table_check(t));
    TM_HIP_CHECK(hipMalloc((void**)&t.dev, sizeof(LoraTableDev)));
    TM_HIP_CHECK(hipMemcpy(t.dev, &t.host, sizeof(LoraTableDev), hipMemcpyHostToDevice));
    return 0;
}

// device copies of A / B, then the slot's entry of the device table; a replaced slot's copies are freed once the device is idle
int lora_table_set(LoraTable& t, int slot, const void* A, const void* B, const int* seg_rank, int ldb)
{
    TM_REQUIRE(t.dev && A && B && seg_rank, "lora: null pointer");
    TM_REQUIRE(slot >= 0 && slot < t.slots, "lora: slot outside the table (at most 8 adapter slots)");
    LoraSlotDev s{};
    TM_TRY_RC(lora_slot_check(t, seg_rank, ldb, &s));
    const size_t a_bytes = (size_t)s.rt * t.K * 2, b_bytes = (size_t)t.N * ldb * 2;
    half_t *     dA = nullptr, *dB = nullptr;
    hipError_t   err = hipMalloc((void**)&dA, a_bytes);
    err = err != hipSuccess ? err : hipMalloc((void**)&dB, b_bytes);
    err = err != hipSuccess ? err : hipMemcpy(dA, A, a_bytes, hipMemcpyDefault);
    err = err != hipSuccess ? err : hipMemcpy(dB, B, b_bytes, hipMemcpyDefault);
    if (err != hipSuccess) {  // the table stays as it was
        (void)hipFree(dA), (void)hipFree(dB);
        TM_HIP_CHECK(err);
    }
    s.A = dA, s.B = dB;
    const LoraSlotDev old = t.host.slot[slot];
    t.host.slot[slot]     = s;
    TM_HIP_CHECK(hipMemcpy(&t.dev->slot[slot], &s, sizeof(s), hipMemcpyHostToDevice));
    TM_HIP_CHECK(hipDeviceSynchronize());
    (void)hipFree((void*)old.A), (void)hipFree((void*)old.B);
    t.rt_max = 0;
    for (int i = 0; i < t.slots; ++i) {
        t.rt_max = std::max(t.rt_max, t.host.slot[i].rt);
    }
    return 0;
}

void lora_table_free(LoraTable& t)
{
    for (int i = 0; i < kLoraMaxSlots; ++i) {
        (void)hipFree((void*)t.host.slot[i].A), (void)hipFree((void*)t.host.slot[i].B);
    }
    (void)hipFree(t.dev);
    t = LoraTable{};
}

int launch_lora_delta(const LoraTable& t, const half_t* x, int ldx, half_t* y, int ldy, int M, const void* plan_ws, hipStream_t stream)
{
    TM_REQUIRE(t.dev && x && y && plan_ws, "lora: null pointer");
    TM_TRY_RC(lora_table_check(t));
    TM_REQUIRE(M >= 1, "lora: M >= 1");
    TM_REQUIRE(ldx >= t.K && ldx % 8 == 0 && ldy >= t.N && ldy % 4 == 0, "lora: ldx >= K, ldx % 8 == 0, ldy >= N, ldy % 4 == 0");
    TM_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 7) == 0, "lora: x must be 16-byte aligned, y 8-byte aligned");
    DeltaArgs p{};
    p.x = x, p.y = y, p.tab = t.dev, p.plan = (const int*)plan_ws;
    p.ldx = ldx, p.ldy = ldy, p.K = t.K, p.N = t.N, p.T = lora_plan_tiles(M), p.nseg = t.nseg;
    for (int g = 0; g < t.nseg; ++g) {
        p.seg_begin[g] = t.seg_begin[g];
        p.seg_end[g]   = t.seg_end[g];
    }
    // the largest column tile that still gives every CU a workgroup from a dense batch's row tiles (header comment)
    const int dense = (M + 15) / 16;
    p.nsub          = 1;
    for (int nsub = 4; nsub > 1; nsub /= 2) {
        if ((int64_t)dense * ((t.N + 64 * nsub - 1) / (64 * nsub)) >= 256) {
            p.nsub = nsub;
            break;
        }
    }
    const int    rt_max = t.rt_max;  // widest stacked rank of a filled slot: sizes the dynamic LDS of every workgroup of the launch
    const size_t lds    = (size_t)4 * 16 * (rt_max + 4) * 4 + (size_t)16 * (rt_max + 8) * 2;
    if (rt_max == 0) {
        return 0;  // nothing loaded: nothing to add
    }
    const dim3 grid(p.T, (t.N + 64 * p.nsub - 1) / (64 * p.nsub));
    lora_delta_kernel<<<grid, 256, lds, stream>>>(p);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
