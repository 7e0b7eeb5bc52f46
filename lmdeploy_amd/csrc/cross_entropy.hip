// Per-row cross-entropy of fp16 logits against int32 targets: the prompt scoring behind tm_engine_score / Pipeline.get_ppl.
//
// Replaces: CrossEntropyLossKernel (src/turbomind/kernels/cross_entropy_kernels.cu:31-73).  Same formula per row,
//   nll = logf(sum_exp + 1e-9f) + max - x[target],   max starts at -FLT_MAX,
// in fp32 from the raw logits.  Differences: one pass over the row instead of two (an online (max, sum) pair per lane), and
// the per-row losses are written, not atomically added into one accumulator, so that the caller sums them in a fixed order
// (bitwise reproducible from run to run).
#include "tm_common.h"
#include "tm_kernels.h"
#include <cfloat>

namespace tmk {

namespace {

constexpr int kCeThreads = 256;  // 4 x wave64 per row
constexpr int kCeUnroll  = 4;    // 16-byte vectors in flight per lane before any of them is consumed

// (m, s) with s = sum exp(x - m).  m starts at -FLT_MAX, as the reference's max does: it never becomes -inf, so exp(x - m) of
// an x = -inf entry is exp(-inf) = 0 and an all -inf row ends with s = 0, m = -FLT_MAX -> loss = +inf (x[target] = -inf),
// without a special case.  fmaxf drops NaN from m; a NaN logit still reaches s through exp(NaN - m) and poisons the row.
struct OnlineSum {
    float m = -FLT_MAX;
    float s = 0.f;

    __device__ __forceinline__ void add8(const half8_t& v)
    {
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f[i] = (float)v[i];
        }
        float mx = fmaxf(fmaxf(fmaxf(f[0], f[1]), fmaxf(f[2], f[3])), fmaxf(fmaxf(f[4], f[5]), fmaxf(f[6], f[7])));
        if (mx > m) {  // one rescale per vector of 8
            s *= __expf(m - mx);
            m = mx;
        }
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            t += __expf(f[i] - m);
        }
        s += t;
    }

    __device__ __forceinline__ void add1(float f)
    {
        if (f > m) {
            s *= __expf(m - f);
            m = f;
        }
        s += __expf(f - m);
    }

    // merge rule s = s_a e^(m_a - m) + s_b e^(m_b - m); both m are finite (>= -FLT_MAX), so no -inf - -inf
    __device__ __forceinline__ void merge(float mb, float sb)
    {
        const float mm = fmaxf(m, mb);
        s              = s * __expf(m - mm) + sb * __expf(mb - mm);
        m              = mm;
    }
};

}  // namespace

// One workgroup per row (grid-strided over rows); nll[r] for target[r] in [0, V), 0 for target < 0 (row not read), NaN for
// target >= V.  Reduction: butterfly over the 64 lanes of a wave, then the 4 waves in fixed order through LDS -- no atomics.
__global__ __launch_bounds__(kCeThreads) void cross_entropy_rows_kernel(float* __restrict__ nll,
                                                                        const half_t* __restrict__ logits,
                                                                        const int* __restrict__ targets,
                                                                        int rows,
                                                                        int V,
                                                                        int ld)
{
    __shared__ float sm[kCeThreads / kWave], ss[kCeThreads / kWave];
    const int tid  = threadIdx.x;
    const int wave = tid / kWave;
    for (int row = blockIdx.x; row < rows; row += gridDim.x) {
        const int tgt = targets[row];
        if (tgt < 0) {  // uniform across the workgroup
            if (tid == 0) {
                nll[row] = 0.f;
            }
            continue;
        }
        const half_t* lp = logits + (size_t)row * ld;
        OnlineSum     acc;
        // 16-byte vectors need a 16-byte aligned row: ld % 8 == 0 and an aligned base (checked by the launcher: uniform)
        const bool vec  = (ld % 8 == 0) && (((uintptr_t)logits & 15) == 0);
        const int  nvec = vec ? V / 8 : 0;
        int        v    = tid;
        for (; v + (kCeUnroll - 1) * kCeThreads < nvec; v += kCeUnroll * kCeThreads) {
            half8_t x[kCeUnroll];
#pragma unroll
            for (int u = 0; u < kCeUnroll; ++u) {
                x[u] = *(const half8_t*)(lp + (size_t)(v + u * kCeThreads) * 8);
            }
#pragma unroll
            for (int u = 0; u < kCeUnroll; ++u) {
                acc.add8(x[u]);
            }
        }
        for (; v < nvec; v += kCeThreads) {
            acc.add8(*(const half8_t*)(lp + (size_t)v * 8));
        }
        for (int i = nvec * 8 + tid; i < V; i += kCeThreads) {  // tail V % 8, or the whole row on the scalar path
            acc.add1((float)lp[i]);
        }
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) {
            const float mo = __shfl_xor(acc.m, off);
            const float so = __shfl_xor(acc.s, off);
            acc.merge(mo, so);
        }
        if ((tid & (kWave - 1)) == 0) {
            sm[wave] = acc.m;
            ss[wave] = acc.s;
        }
        __syncthreads();
        if (tid == 0) {
            OnlineSum r;
            r.m = sm[0];
            r.s = ss[0];
            for (int w = 1; w < kCeThreads / kWave; ++w) {
                r.merge(sm[w], ss[w]);
            }
            nll[row] = tgt < V ? __logf(r.s + 1e-9f) + r.m - (float)lp[tgt] : __int_as_float(0x7fc00000);
        }
        __syncthreads();  // sm / ss are reused by the next row
    }
}

int launch_cross_entropy(float* nll, const half_t* logits, const int* targets, int rows, int V, int ld, hipStream_t st)
{
    TM_REQUIRE(rows >= 0 && V >= 1 && ld >= V, "rows >= 0, vocab >= 1, ld >= vocab");
    if (rows == 0) {
        return 0;
    }
    TM_REQUIRE(nll && logits && targets, "null pointer");
    // bandwidth-bound: at most ~2048 workgroups (8 per CU), the rest grid-strided
    cross_entropy_rows_kernel<<<std::min(rows, 2048), kCeThreads, 0, st>>>(nll, logits, targets, rows, V, ld);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
