// Speculative decoding by prompt lookup (n-gram drafting), device side: the proposer, the rows of the verify forward and the greedy
// acceptance.  All control stays on the device, so a speculative step is one fixed-shape chain of launches (capturable as a hipGraph).
//
// Proposer (spec_propose_kernel, one workgroup per sequence).  h = the sequence's token history (prompt + emitted tokens), L its length;
// h[L - 1] is the last emitted token, row 0 of the next verify forward.  For n = ngram_max down to ngram_min: the suffix h[L - n : L] is
// looked up among the starts i with h[i : i + n] == suffix and i + n <= L - 1 (so at least one token follows; overlap with the suffix is
// allowed); the LARGEST such i wins and the first n with a match wins.  The draft is h[i + n : min(i + n + k, L)]; no match: n_draft = 0.
// n_draft is capped at remaining - 1 (remaining = max_new - emitted): a step emits at most n_draft + 1 tokens.
//
// Acceptance (spec_accept_kernel, one thread per sequence).  ids[b][j] is the greedy token behind input row j.  a = the largest value
// <= n_draft with ids[j] == draft[j] for all j < a; ids[0 .. a] are emitted, cut at `remaining`; they join `generated` and the history,
// k_len += emitted (the KV of the rows behind them is dead and overwritten by the next step), next_id = the last emitted token.  A sequence
// with remaining == 0 emits nothing and keeps its k_len.  totals: (sequence-steps that emitted, drafted, accepted, emitted).
#include "tm_common.h"
#include "tm_kernels.h"

namespace tmk {

namespace {

__global__ __launch_bounds__(256) void spec_propose_kernel(int* drafts, int* n_draft, SpecState s, int k, int ngram_max, int ngram_min)
{
    __shared__ int best;
    const int      b   = blockIdx.x;
    const int      tid = threadIdx.x;
    const int*     h   = s.hist + (size_t)b * s.hist_stride;
    const int      L   = min(max(s.hist_len[b], 0), s.hist_stride);
    const int      remaining = max(s.max_new - s.emitted[b], 0);
    const int      cap = min(k, remaining - 1);
    int            found = -1, fn = 0;
    for (int n = ngram_max; n >= ngram_min && cap > 0; --n) {  // every condition is workgroup-uniform
        if (n > L - 1) {
            continue;
        }
        if (tid == 0) {
            best = -1;
        }
        __syncthreads();
        int local = -1;
        for (int i = tid; i + n <= L - 1; i += 256) {
            bool ok = true;
            for (int e = 0; e < n; ++e) {
                ok = ok && h[i + e] == h[L - n + e];
            }
            local = ok ? i : local;  // i grows: the last hit is this thread's largest
        }
        if (local >= 0) {
            atomicMax(&best, local);
        }
        __syncthreads();
        found = best;
        __syncthreads();  // everybody has read `best` before the next n resets it
        if (found >= 0) {
            fn = n;
            break;
        }
    }
    const int nd = found >= 0 ? min(min(k, L - (found + fn)), cap) : 0;
    for (int j = tid; j < k; j += 256) {
        drafts[(size_t)b * k + j] = j < nd ? h[found + fn + j] : 0;
    }
    if (tid == 0) {
        n_draft[b] = nd;
    }
}

// start of a batch: the history holds the prompt (k_len tokens, uploaded by the caller); the prefill's first token joins it
__global__ void spec_begin_kernel(SpecState s, int batch)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) {
        return;
    }
    const int L = min(max(s.k_len[b], 0), s.hist_stride);
    if (L < s.hist_stride) {
        s.hist[(size_t)b * s.hist_stride + L] = s.next_id[b];
    }
    s.hist_len[b] = min(L + 1, s.hist_stride);
    s.emitted[b]  = 1;
}

__global__ void spec_rows_kernel(int* ids, int* k_len_fw, const int* drafts, SpecState s, int batch, int k)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * (k + 1)) {
        return;
    }
    const int b = i / (k + 1), j = i - b * (k + 1);
    ids[i]      = j == 0 ? s.next_id[b] : drafts[(size_t)b * k + j - 1];
    if (j == 0) {
        k_len_fw[b] = s.k_len[b] + k + 1;
    }
}

__global__ void spec_accept_kernel(const int* out_ids, const int* drafts, const int* n_draft, SpecState s, int batch, int k, int* step_emitted)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) {
        return;
    }
    const int done      = s.emitted[b];
    const int remaining = max(s.max_new - done, 0);
    if (remaining == 0) {
        if (step_emitted) {
            step_emitted[b] = 0;
        }
        return;
    }
    const int  nd  = min(max(n_draft[b], 0), k);
    const int* ids = out_ids + (size_t)b * (k + 1);
    int        a   = 0;
    while (a < nd && ids[a] == drafts[(size_t)b * k + a]) {
        ++a;
    }
    const int n_emit = min(a + 1, remaining);
    const int L      = s.hist_len[b];
    for (int j = 0; j < n_emit; ++j) {
        s.generated[(size_t)b * s.max_new + done + j] = ids[j];
        if (L + j < s.hist_stride) {
            s.hist[(size_t)b * s.hist_stride + L + j] = ids[j];
        }
    }
    s.emitted[b]  = done + n_emit;
    s.hist_len[b] = min(L + n_emit, s.hist_stride);
    s.k_len[b] += n_emit;
    s.next_id[b] = ids[n_emit - 1];
    if (step_emitted) {
        step_emitted[b] = n_emit;
    }
    unsigned long long* t = (unsigned long long*)s.totals;
    atomicAdd(t + 0, 1ull);
    atomicAdd(t + 1, (unsigned long long)nd);
    atomicAdd(t + 2, (unsigned long long)(n_emit - 1));
    atomicAdd(t + 3, (unsigned long long)n_emit);
}

// proposer: reads the history and the emitted counts only; the others read or write every field
int check_state(const SpecState& s, int batch, int k, bool proposer = false)
{
    TM_REQUIRE(s.hist && s.hist_len && s.emitted, "null pointer");
    TM_REQUIRE(proposer || (s.generated && s.k_len && s.next_id && s.totals), "null pointer");
    TM_REQUIRE(batch >= 1 && k >= 1 && k <= kSpecMaxDraft, "speculative: batch >= 1, 1 <= k <= 7");
    TM_REQUIRE(s.hist_stride >= 1 && s.max_new >= 1, "speculative: history stride / max_new");
    return 0;
}

}  // namespace

int launch_spec_propose(int* drafts, int* n_draft, const SpecState& s, int batch, int k, int ngram_max, int ngram_min, hipStream_t st)
{
    TM_REQUIRE(drafts && n_draft, "null pointer");
    if (const int rc = check_state(s, batch, k, true)) {
        return rc;
    }
    TM_REQUIRE(1 <= ngram_min && ngram_min <= ngram_max && ngram_max <= kSpecMaxNgram, "speculative: 1 <= ngram_min <= ngram_max <= 8");
    spec_propose_kernel<<<batch, 256, 0, st>>>(drafts, n_draft, s, k, ngram_max, ngram_min);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_spec_begin(const SpecState& s, int batch, hipStream_t st)
{
    TM_REQUIRE(s.hist && s.hist_len && s.emitted && s.k_len && s.next_id && batch >= 1 && s.hist_stride >= 1, "null pointer / batch");
    spec_begin_kernel<<<(batch + 63) / 64, 64, 0, st>>>(s, batch);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_spec_rows(int* ids, int* k_len_fw, const int* drafts, const SpecState& s, int batch, int k, hipStream_t st)
{
    TM_REQUIRE(ids && k_len_fw && drafts, "null pointer");
    if (const int rc = check_state(s, batch, k)) {
        return rc;
    }
    spec_rows_kernel<<<(batch * (k + 1) + 255) / 256, 256, 0, st>>>(ids, k_len_fw, drafts, s, batch, k);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

int launch_spec_accept(const int* out_ids, const int* drafts, const int* n_draft, const SpecState& s, int batch, int k, int* step_emitted,
                       hipStream_t st)
{
    TM_REQUIRE(out_ids && drafts && n_draft, "null pointer");
    if (const int rc = check_state(s, batch, k)) {
        return rc;
    }
    spec_accept_kernel<<<(batch + 63) / 64, 64, 0, st>>>(out_ids, drafts, n_draft, s, batch, k, step_emitted);
    TM_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace tmk
