"""Plain Python / numpy restatement of the constrained-decoding rules (csrc/constrain.hip; contract in include/llark_hip.h:
llark_constrain_rows, llark_beam_topk_rows_banned), for the constraint tests: HF 4.29.2's NoRepeatNGram, NoBadWords (``_tokens_match``),
MinLength and MinNewTokensLength processors over ONE row's history h[0 .. L) -- its own prompt, then what it generated."""
import numpy as np

from beam_ref import BeamRef, row_candidates


def words_of(bad_words_ids=(), suppress_tokens=(), eos=-1):
    """The word table: bad words, then suppress_tokens as one-token words; a word equal to [eos] is dropped."""
    table = [list(w) for w in bad_words_ids] + [[int(t)] for t in suppress_tokens]
    return [w for w in table if not (eos is not None and eos >= 0 and w == [eos])]


def banned_set(hist, vocab, n=0, words=(), eos=-1, prompt_len=0, min_new=0, min_len=0):
    """The tokens in [0, vocab) banned for the next choice after the history ``hist``."""
    h = [int(t) for t in hist]
    L = len(h)
    out = set()
    if n and n > 0 and L + 1 >= n:
        tail = h[L - n + 1:] if n > 1 else []
        for i in range(0, L - n + 1):
            if h[i:i + n - 1] == tail:
                out.add(h[i + n - 1])
    for w in words:
        k = len(w)
        if k - 1 <= L and (k == 1 or h[L - k + 1:] == list(w[:-1])):
            out.add(int(w[-1]))
    if eos is not None and eos >= 0 and (L - prompt_len < min_new or L < min_len):
        out.add(int(eos))
    return {t for t in out if 0 <= t < vocab}


def processed_row(row, banned):
    """The row's own bits, -inf at the banned columns."""
    out = np.array(row, dtype=np.float32, copy=True)
    if banned:
        out[sorted(banned)] = -np.inf
    return out


def bitmap(banned, vocab):
    words = np.zeros((vocab + 31) // 32, dtype=np.uint32)
    for t in banned:
        words[t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return words.view(np.int32)


def update_history(hists, parent=None, last=None, active=None, width=None):
    """One launch's history update over all slots, in place semantics restated on copies: slot s takes hists[parent[s]] when parent[s]
    is another valid slot, then appends last[s].  Returns (new histories, full: whether some row was full).  Skipped slots (``active``
    False) keep theirs."""
    n = len(hists)
    old = [list(h) for h in hists]
    new, full = [], False
    for s in range(n):
        if active is not None and not active[s]:
            new.append(old[s])
            continue
        p = s if parent is None else int(parent[s])
        if p < 0 or p >= n:
            p = s
        h = list(old[p][: len(old[s])]) if p != s else list(old[s])
        if last is not None:
            if width is not None and len(h) >= width:
                full = True
            else:
                h.append(int(last[s]))
        new.append(h)
    return new, full


def banned_candidates(row, score, beams, banned):
    """row_candidates over the unbanned columns of the row's FULL-row values: a banned token counts in the log-softmax and is left out
    of the selection; (cand, token, lp) [2B], padded with (-inf, -1, -inf)."""
    K = 2 * beams
    c, t, lp = row_candidates(row, score, beams, count=len(row))
    keep = [i for i in range(len(t)) if t[i] >= 0 and int(t[i]) not in banned][:K]
    pad = K - len(keep)
    return (np.concatenate((c[keep], np.full(pad, -np.inf))), np.concatenate((t[keep], np.full(pad, -1, dtype=np.int64))),
            np.concatenate((lp[keep], np.full(pad, -np.inf))))


class ConstrainedBeamRef:
    """BeamRef driven with candidates from the unbanned columns; the slots' histories follow the beams."""

    def __init__(self, prompts, beams, vocab, eos=-1, pad=0, length_penalty=1.0, early_stopping=False, n=0, words=(), min_new=0, min_len=0):
        self.ref = BeamRef([len(p) for p in prompts], beams, eos, pad, length_penalty, early_stopping)
        self.B, self.vocab, self.eos = beams, vocab, eos
        self.kw = dict(n=n, words=words, eos=eos, min_new=min_new, min_len=min_len)
        self.hists = [[int(t) for t in prompts[s // beams]] for s in range(len(prompts) * beams)]
        self.plens = [len(prompts[s // beams]) for s in range(len(prompts) * beams)]
        self.last = None

    def step(self, logits):
        ref, B = self.ref, self.B
        slots = ref.N * B
        active = [not ref.done[s // B] for s in range(slots)]
        if self.last is not None:
            self.hists, _ = update_history(self.hists, ref.trellis[-1][0], self.last, active)
        cs, ct, cl = np.zeros((slots, 2 * B), dtype=np.float32), np.zeros((slots, 2 * B), dtype=np.int64), np.zeros((slots, 2 * B))
        for s in range(slots):
            if not active[s]:
                continue
            ban = banned_set(self.hists[s], self.vocab, prompt_len=self.plens[s], **self.kw)
            c, t, lp = banned_candidates(logits[s], ref.score[s], B, ban)
            cs[s], ct[s], cl[s] = c.astype(np.float32), t, lp
        nxt, pairs = ref.step(cands=(cs, ct, cl))
        self.last = nxt
        return nxt, pairs
