"""Numpy float64 restatement of ``llark_token_logprob_rows`` (csrc/logprob.hip; contract in include/llark_hip.h) for the
log-probability tests: the values, the skip rules, the per-slot history, and the tolerance of the kernel's fp32 arithmetic."""
import numpy as np

ROW_IDLE, ROW_ACTIVE, ROW_FINISHED = 0, 1, 2
THREADS, LANE_STEPS, WAVES = 1024, 6, 16


def depth(vocab: int) -> int:
    """D: the additions on the longest path of the kernel's sum of exponentials, counted from csrc/logprob.hip: a thread adds its
    ceil(vocab / 1024) columns one by one (the first onto 0), the butterfly over the 64 lanes takes 6 steps, and the 16 wave sums are
    added in a chain of 15: ceil(vocab / 1024) + 21; 71 at vocab 50 435, 53 at 32 003."""
    return -(-int(vocab) // THREADS) + LANE_STEPS + (WAVES - 1)


def row_logprob(row, t: int):
    """One evaluated row in float64: (logprob, rank, E) with E = sum_i p_i (M - l_i), the rounding of the exponent arguments weighted
    by the row's own distribution.  A NaN in the row or a maximum of +-inf: (NaN, -1, 0)."""
    l = np.asarray(row, dtype=np.float64)
    if np.isnan(l).any() or np.isinf(l.max()):
        return float("nan"), -1, 0.0
    M = l.max()
    with np.errstate(all="ignore"):
        d = l - M                                              # -inf for a -inf logit: exp gives exactly 0
        e = np.exp(d)
        S = e.sum()
        lp = float((l[t] - M) - np.log(S))
        E = float(np.where(e > 0, e * -d, 0.0).sum() / S)
    return lp, int((l > l[t]).sum()), E


def tol_of(row, t: int) -> float:
    """2^-24 (2 |l_t - M| + |lp| + D + E + 4): the two subtractions (l_t - M, and the final one, each half an ulp of a number no
    larger than |l_t - M| + |lp|), logf (1 ulp of |log S| <= |l_t - M| + |lp|), D additions of positive terms (relative 2^-24 each, so D
    2^-24 on log S), the exponent arguments (E), expf (1 ulp) and slack; infinite where the reference itself is not finite."""
    lp, _, E = row_logprob(row, t)
    if not np.isfinite(lp):
        return float("inf")
    l = np.asarray(row, dtype=np.float64)
    return 2.0 ** -24 * (2.0 * abs(l[t] - l.max()) + abs(lp) + depth(l.size) + E + 4.0)


def token_logprob_rows(logits, vocab, tokens, slots, state=None, slot_of_row=None, logprob=None, rank=None, hist=None, count=None,
                       total=None):
    """The whole launch on numpy arrays; ``logprob`` / ``rank`` / ``hist`` / ``count`` / ``total`` are updated in place (float64 /
    int) exactly where the kernel writes, everything else keeps what it held.  Returns the list of evaluated rows."""
    logits = np.asarray(logits)
    rows = logits.shape[0]
    if hist is not None and count is None:
        raise ValueError("hist requires count")
    done = []
    for r in range(rows):
        slot = int(slot_of_row[r]) if slot_of_row is not None else r
        if not 0 <= slot < slots:
            continue
        if state is not None and state[slot] != ROW_ACTIVE:
            continue
        t = int(tokens[r])
        if not 0 <= t < vocab:
            continue
        lp, rk, _ = row_logprob(logits[r, :vocab], t)
        if logprob is not None:
            logprob[r] = lp
        if rank is not None:
            rank[r] = rk
        if count is not None:
            if hist is not None and count[slot] < hist.shape[1]:
                hist[slot, count[slot]] = lp
        if total is not None:
            total[slot] += lp
        if count is not None:
            count[slot] += 1
        done.append(r)
    return done


def make_rows(vocab: int, rows: int, seed: int = 0) -> np.ndarray:
    """3 * randn logits with up to five tokens raised by 6 .. 10 (the family of the sampling tests): peaked like a model's."""
    rng = np.random.default_rng(1000 * seed + vocab + 7)
    logits = (3.0 * rng.standard_normal((rows, vocab))).astype(np.float32)
    n_up = min(5, vocab)
    for r in range(rows):
        up = rng.choice(vocab, size=n_up, replace=False)
        logits[r, up] += rng.uniform(6.0, 10.0, size=n_up).astype(np.float32)
    return logits
