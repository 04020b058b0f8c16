"""Plain-Python restatement of the speculative greedy step of csrc/speculate.hip (llark_spec_verify_rows, llark_spec_draft_rows), as
include/llark_hip.h states it, and of the two decode loops it must make equal: the plain greedy loop and the block loop.  A plain
module: tests/test_spec_ref_cpu.py proves the loop property on it, tests/test_spec_kernels_gpu.py holds the kernels to it exactly."""
import math

IDLE, ACTIVE, FINISHED = 0, 1, 2          # LLARK_ROW_*
MAX_BLOCK = 8


def better(v, i, bv, bi):
    """llark_decode_advance_rows' order: first maximal index, a NaN counts as the maximum"""
    vn, bn = v != v, bv != bv
    if vn or bn:
        return vn and (not bn or i < bi)
    return v > bv or (v == bv and i < bi)


def argmax(row):
    bv, bi = -math.inf, 0x7FFFFFFF
    for j, v in enumerate(row):
        if better(v, j, bv, bi):
            bv, bi = v, j
    return bi


def verify(greedy, ids, blk, state, pos, budget, eos, pad, hist=None, ld_hist=None):
    """One slot of llark_spec_verify_rows.  ``greedy``: g_i of the block's rows (only the first ``blk`` are read), ``ids``: the block's
    input tokens.  Returns (out_tokens[8], n_out, state, pos, budget, next_id or None when untouched); ``hist`` (a list) is appended to
    in place, up to ``ld_hist`` tokens."""
    if state != ACTIVE or blk <= 0 or budget <= 0:
        return [pad] * MAX_BLOCK, 0, state, pos, budget, None
    a = 0
    while a < blk - 1 and ids[a + 1] == greedy[a]:
        a += 1
    n = min(a + 1, budget)
    fin = False
    for i in range(n):
        if eos >= 0 and greedy[i] == eos:
            n, fin = i + 1, True
            break
    toks = list(greedy[:n])
    if hist is not None:
        for t in toks:
            if ld_hist is None or len(hist) < ld_hist:
                hist.append(t)
    return toks + [pad] * (MAX_BLOCK - n), n, FINISHED if fin else state, pos + n, budget - n, toks[-1]


def lookup(hist, k_max, g_max):
    """prompt lookup: for g = g_max .. 1 the last g tokens of ``hist`` at the largest earlier start s <= len - g - 1; the tokens that
    follow that occurrence, at most k_max"""
    n = len(hist)
    for g in range(g_max, 0, -1):
        if n < g + 1:
            continue
        suf = hist[n - g:]
        for s in range(n - g - 1, -1, -1):
            if hist[s:s + g] == suf:
                return list(hist[s + g:n][:k_max])
    return []


def draft(next_id, state, pos, budget, stride, k_max, smax, pad, drafts=None, hist=None, g_max=2):
    """One slot of llark_spec_draft_rows: (ids[stride], blk).  ``drafts``: the caller's form (a list), else the lookup over ``hist``."""
    cap = min(stride, budget, smax - pos)
    if state != ACTIVE or pos < 0 or cap <= 0:
        return [pad] * stride, 0
    d = list(drafts) if drafts is not None else lookup(hist, k_max, g_max)
    d = d[:max(0, min(k_max, cap - 1))]
    return [next_id] + d + [pad] * (stride - 1 - len(d)), 1 + len(d)


# ---- the two loops ---------------------------------------------------------------------------------------------------
def plain_loop(next_token, prompt, max_new, eos, smax):
    """greedy decoding, one token per step: ``next_token(seq)`` is the model (deterministic).  Stops after eos, after max_new
    tokens, or when the cache (smax positions) is full: the step that feeds position p needs p < smax."""
    seq, out = list(prompt), []
    while len(out) < max_new and len(seq) - 1 < smax:        # the step feeds token seq[-1] at position len(seq) - 1
        t = next_token(seq)
        seq.append(t)
        out.append(t)
        if eos >= 0 and t == eos:
            break
    return out


def block_loop(next_token, prompt, max_new, eos, smax, stride, k_max, drafter, pad=0, g_max=2):
    """the speculative loop over verify() / draft().  ``drafter(hist)`` returns the caller's drafts, or None for the prompt lookup.
    The model sees a block as the plain loop would see each of its prefixes: g_i = next_token(history + ids[1 .. i]).
    Returns (tokens, steps)."""
    hist = list(prompt)                                       # the history holds the prompt and every emitted token
    state, pos, budget = ACTIVE, len(prompt) - 1, max_new     # the last prompt token is the first block's row 0
    next_id = prompt[-1]
    out, steps = [], 0
    while True:
        ids, blk = draft(next_id, state, pos, budget, stride, k_max, smax, pad, drafts=drafter(hist), hist=hist, g_max=g_max)
        if blk == 0:
            break
        assert ids[0] == hist[-1]
        greedy = [next_token(hist + ids[1:i + 1]) for i in range(blk)]
        toks, n, state, pos, budget, next_id = verify(greedy, ids, blk, state, pos, budget, eos, pad, hist)
        assert n >= 1
        out += toks[:n]
        steps += 1
    return out, steps
