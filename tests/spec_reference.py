"""Speculative decoding by prompt lookup, in plain Python / numpy: the proposer rule, the greedy acceptance rule and a simulation of
a whole run over a next-token function.  The GPU kernels (csrc/speculative.hip) and the engine are held to these integers."""
import numpy as np


def ngram_propose(history, k, n_max, n_min, remaining):
    """history: the sequence's tokens (prompt + emitted; the last one is the next forward's first row).  For n = n_max .. n_min the
    suffix history[L - n:] is looked up among the starts i with history[i:i + n] == suffix and i + n <= L - 1 (overlap with the suffix
    allowed); the largest i of the first n that matches gives the draft history[i + n:min(i + n + k, L)], capped at remaining - 1
    tokens.  Returns the draft as a list (empty: no match, or no room)."""
    h = [int(t) for t in history]
    L = len(h)
    cap = min(k, remaining - 1)
    if cap <= 0:
        return []
    for n in range(n_max, n_min - 1, -1):
        if n > L - 1:
            continue
        suffix = h[L - n:]
        for i in range(L - 1 - n, -1, -1):
            if h[i:i + n] == suffix:
                return h[i + n:min(i + n + k, L)][:cap]
    return []


def accept(ids, draft, n_draft, remaining):
    """ids[j]: the greedy token behind input row j (row 0 = the last emitted token, row j = draft[j - 1]).  a = the longest prefix of
    the n_draft drafts with ids[j] == draft[j]; ids[0 .. a] are emitted, cut at `remaining`.  Returns the emitted tokens."""
    if remaining <= 0:
        return []
    a = 0
    while a < n_draft and int(ids[a]) == int(draft[a]):
        a += 1
    return [int(t) for t in ids[:a + 1]][:remaining]


def simulate(next_token, prompt, first_token, max_new, k, n_max, n_min, max_steps=10 ** 6):
    """A speculative run of one sequence over `next_token(history) -> token` (the model's greedy choice behind the history).
    first_token: the prefill's token (emitted before the first step).  Returns (emitted tokens, per-step emitted counts,
    per-step draft lengths); the tokens equal the plain greedy run's whatever the drafts were."""
    hist = [int(t) for t in prompt] + [int(first_token)]
    out, per_step, drafted = [int(first_token)], [], []
    for _ in range(max_steps):
        remaining = max_new - len(out)
        if remaining <= 0:
            break
        draft = ngram_propose(hist, k, n_max, n_min, remaining)
        ids, h = [], list(hist)
        for j in range(len(draft) + 1):          # the verify forward: row j sees the history + draft[:j]
            ids.append(int(next_token(h)))
            if j < len(draft):
                h.append(draft[j])
        new = accept(ids, draft, len(draft), remaining)
        hist += new
        out += new
        per_step.append(len(new))
        drafted.append(len(draft))
    return out, per_step, drafted


def propose_batch(hist, hist_len, emitted, max_new, k, n_max, n_min):
    """the proposer over a padded batch: (drafts [B, k] zero-padded, n_draft [B])"""
    B = len(hist_len)
    drafts, nd = np.zeros((B, k), np.int32), np.zeros(B, np.int32)
    for b in range(B):
        d = ngram_propose(hist[b][:hist_len[b]], k, n_max, n_min, max(max_new - int(emitted[b]), 0))
        drafts[b, :len(d)] = d
        nd[b] = len(d)
    return drafts, nd
