"""Numpy float64 restatement of the beam-search step (csrc/beam.hip; contract in include/llark_hip.h: llark_beam_topk_rows,
llark_beam_advance) and of ``llark_amd.m2t.beam.BeamSearch``'s finalize, for the beam tests: HF 4.29.2's ``beam_search`` +
``BeamSearchScorer`` with one beam group, with this project's tie rules.

Example e of N owns the B global slots e * B .. e * B + B - 1.  A beam's rank and its slot are different things.  Log-softmax rows come
from ``logprob_ref``; a candidate is fp32(score + lp) with lp in float64, the merge and the heap work on fp32 values exactly as given."""
import numpy as np

from logprob_ref import row_logprob, tol_of  # noqa: F401  (tol_of: the tolerance of one lp, used by the tests)

ROW_IDLE, ROW_ACTIVE, ROW_FINISHED = 0, 1, 2
NEG = -1e9


def row_candidates(row, score, beams: int, count=None):
    """(cand float64 [2B] = score + lp unrounded, token [2B], lp float64 [2B]) of one row, ordered by fp32(cand) descending, then token
    ascending (``count``: that many instead of 2B).  A NaN in the row or a maximum of +-inf: all (-inf, -1, -inf)."""
    K = 2 * beams if count is None else int(count)
    l = np.asarray(row, dtype=np.float64)
    if np.isnan(l).any() or np.isinf(l.max()):
        return np.full(K, -np.inf), np.full(K, -1, dtype=np.int64), np.full(K, -np.inf)
    M = l.max()
    with np.errstate(all="ignore"):
        lp = (l - M) - np.log(np.exp(l - M).sum())
        cand = np.float64(score) + lp
        c32 = cand.astype(np.float32)
    order = np.lexsort((np.arange(l.size), -c32.astype(np.float64)))[:K]
    return cand[order], order.astype(np.int64), lp[order]


def cand_tols(row, score, tokens, cands):
    """Tolerance of the kernel's fp32(score + lp) for each of ``tokens``: logprob_ref.tol_of for lp -- 2^-24 (2 |l_t - M| + |lp| + D + E
    + 4), with the row's E computed once -- plus half an ulp of the candidate (the one rounding of the addition: 2^-24 |cand| bounds it)."""
    l = np.asarray(row, dtype=np.float64)
    _, _, E = row_logprob(l, int(tokens[0]))
    M = l.max()
    lt = l[np.asarray(tokens)]
    lps = np.asarray(cands, dtype=np.float64) - np.float64(score)
    from logprob_ref import depth
    return 2.0 ** -24 * (2.0 * np.abs(lt - M) + np.abs(lps) + depth(l.size) + E + 4.0) + 2.0 ** -24 * np.abs(cands)


def near_ties(row, score, beams: int) -> int:
    """Adjacent candidates among the reference's best 2B + 1 (the first one left out included) that differ, but by no more than their two
    tolerances: there the kernel's fp32 order may legitimately differ from the float64 order."""
    c, t, _ = row_candidates(row, score, beams, 2 * beams + 1)
    if t[0] < 0:
        return 0
    tol = cand_tols(row, score, t, c)
    d = np.abs(np.diff(c))
    return int(((d > 0) & (d <= tol[:-1] + tol[1:])).sum())


def make_rows(vocab: int, rows: int, seed: int = 0) -> np.ndarray:
    """logprob_ref.make_rows; every row but rows 1, 9, 17, ... is rounded to multiples of 1/32, so that its candidates either tie exactly
    (equal logits: equal lp bits, the tie rule decides) or differ by about 1/32, far above any tolerance; the others are kept as drawn
    and their seeds are chosen (near_ties) so that no two of their candidates come closer than the tolerances."""
    from logprob_ref import make_rows as base
    x = base(vocab, rows, seed).copy()
    q = np.round(x * 32.0) / 32.0
    keep = (np.arange(rows) % 8) == 1
    x[~keep] = q[~keep]
    return x.astype(np.float32)


def hyp_score(total, length: int, length_penalty: float) -> np.float32:
    return np.float32(np.float64(np.float32(total)) / np.float64(length) ** np.float64(length_penalty))


class BeamRef:
    def __init__(self, prompt_lens, beams: int, eos: int = -1, pad: int = 0, length_penalty: float = 1.0, early_stopping: bool = False):
        self.N, self.B = len(prompt_lens), int(beams)
        self.eos, self.pad, self.length_penalty, self.early_stopping = int(eos), int(pad), float(length_penalty), bool(early_stopping)
        n = self.N * self.B
        self.score = np.full(n, NEG, dtype=np.float32)
        self.score[:: self.B] = 0.0
        self.rank_of_slot = np.tile(np.arange(self.B), self.N)
        self.heaps = [[] for _ in range(self.N)]              # dicts: score, sum, length, end_step, end_slot, arrival, eos_lp
        self.arrivals = [0] * self.N
        self.done = [False] * self.N
        self.cur_len = [int(x) for x in prompt_lens]
        self.state = np.full(n, ROW_ACTIVE)
        self.trellis = []                                      # per step: (parent global slot [n], token [n], lp [n])
        self.steps = 0

    # ---- the heap (BeamHypotheses) ---------------------------------------------------------------------------------------------
    def worst(self, e: int) -> np.float32:
        return np.float32(min((h["score"] for h in self.heaps[e]), default=1e9))

    def add(self, e: int, total, length: int, end_step: int, end_slot: int, eos_lp) -> None:
        sc = hyp_score(total, length, self.length_penalty)
        heap, arrival = self.heaps[e], self.arrivals[e]
        self.arrivals[e] += 1
        entry = dict(score=sc, sum=np.float32(total), length=int(length), end_step=int(end_step), end_slot=int(end_slot), arrival=arrival,
                     eos_lp=float(eos_lp))
        if len(heap) < self.B:
            heap.append(entry)
        elif sc > self.worst(e):
            at = min(range(len(heap)), key=lambda i: (heap[i]["score"], heap[i]["arrival"]))
            heap[at] = entry

    # ---- one step ----------------------------------------------------------------------------------------------------------------
    def candidates(self, logits):
        """cand fp32 / token / lp of every slot from logits [slots][V] (row = slot)."""
        n, K = self.N * self.B, 2 * self.B
        cs, ct, cl = np.zeros((n, K), dtype=np.float32), np.zeros((n, K), dtype=np.int64), np.zeros((n, K))
        for s in range(n):
            c, t, lp = row_candidates(logits[s], self.score[s], self.B)
            cs[s], ct[s], cl[s] = c.astype(np.float32), t, lp
        return cs, ct, cl

    def step(self, logits=None, cands=None, advance: bool = True):
        """Steps 2 to 5 of every example from ``cands`` = (cand fp32, token, lp), each [slots][2B] (or from ``logits``).  Returns
        (next_ids [slots], pairs: per example the list of (src, dst) global slots)."""
        B, K, n = self.B, 2 * self.B, self.N * self.B
        cs, ct, cl = self.candidates(logits) if cands is None else cands
        parent_row, token_row, lp_row = np.full(n, -1), np.full(n, -1), np.full(n, np.nan)
        next_ids, all_pairs = np.full(n, self.pad, dtype=np.int64), []
        for e in range(self.N):
            base = e * B
            if self.done[e]:
                all_pairs.append([])
                continue
            slot_of_rank = np.zeros(B, dtype=np.int64)
            slot_of_rank[self.rank_of_slot[base:base + B]] = np.arange(B)
            merged = sorted(((-np.float64(np.float32(cs[base + slot_of_rank[r], k])), r, int(ct[base + slot_of_rank[r], k]), k)
                             for r in range(B) for k in range(K)), key=lambda x: (x[0], x[1], x[3]))[:K]
            live, cur = [], self.cur_len[e]
            for place, (negc, r, t, k) in enumerate(merged):
                slot = int(slot_of_rank[r])
                c, lp = np.float32(-negc), cl[base + slot, k]
                if t < 0:
                    continue
                if self.eos >= 0 and t == self.eos:
                    if place < B:
                        self.add(e, c, cur, self.steps, base + slot, lp)
                    continue
                live.append((slot, t, c, lp))
                if len(live) == B:
                    break
            done = len(live) < B
            if not done and len(self.heaps[e]) >= B:
                done = self.early_stopping or self.worst(e) >= hyp_score(-merged[0][0], cur, self.length_penalty)
            has_child = [False] * B
            first = []
            for (p, _, _, _) in live:
                first.append(not has_child[p])
                has_child[p] = True
            free = [s for s in range(B) if not has_child[s]]
            pairs = []
            for q, (p, t, c, lp) in enumerate(live):
                slot = p if first[q] else free.pop(0)
                if slot != p and not done:
                    pairs.append((base + p, base + slot))
                g = base + slot
                self.score[g], self.rank_of_slot[g] = c, q
                next_ids[g] = self.pad if done else t
                parent_row[g], token_row[g], lp_row[g] = base + p, t, lp
            for q in range(len(live), B):
                g = base + free.pop(0)
                self.score[g], self.rank_of_slot[g] = -np.inf, q
            all_pairs.append(pairs)
            self.cur_len[e] = cur + 1
            if done:
                self.done[e] = True
                self.state[base:base + B] = ROW_FINISHED
        self.trellis.append((parent_row, token_row, lp_row))
        self.steps += 1
        return next_ids, all_pairs

    # ---- the end -----------------------------------------------------------------------------------------------------------------
    def backtrack(self, end_step: int, end_slot: int):
        toks, lps, slot = [], [], end_slot
        for s in range(end_step - 1, -1, -1):
            p, t, lp = (a[slot] for a in self.trellis[s])
            toks.append(int(t)), lps.append(float(lp))
            slot = int(p)
        return toks[::-1], lps[::-1]

    def tokens_of_slot(self, slot: int):
        return self.backtrack(self.steps, slot)[0]

    def finalize(self, num_return_sequences: int = 1):
        """Per example the R best hypotheses (score descending, earlier arrival first): dicts with tokens, logprobs (the closing eos'
        included when there was one), score, sum, length, eos (did it end on eos)."""
        out = []
        for e in range(self.N):
            base = e * self.B
            if not self.done[e]:
                for r in range(self.B):
                    slot = base + int(np.nonzero(self.rank_of_slot[base:base + self.B] == r)[0][0])
                    self.add(e, self.score[slot], self.cur_len[e], self.steps, slot, np.nan)
            best = sorted(self.heaps[e], key=lambda h: (-np.float64(h["score"]), h["arrival"]))[:num_return_sequences]
            hyps = []
            for h in best:
                toks, lps = self.backtrack(h["end_step"], h["end_slot"])
                ended = not np.isnan(h["eos_lp"])
                hyps.append(dict(tokens=toks, logprobs=lps + ([h["eos_lp"]] if ended else []), score=h["score"], sum=h["sum"],
                                 length=h["length"], eos=ended))
            out.append(hyps)
        return out


def layout(prompts, hyps, eos, pad, max_new_tokens: int):
    """HF's output: ``prompts`` int [N][S] as given, every hypothesis after its example's prompt; width = min(longest + 1, S +
    max_new_tokens); a row shorter than the width gets eos right after its last token (when there is an eos), the rest is pad.
    Returns (ids [N * R][width], logprobs [N * R][width - S], NaN where nothing was chosen)."""
    prompts = np.asarray(prompts)
    S = prompts.shape[1]
    rows = [(e, h) for e, hs in enumerate(hyps) for h in hs]
    width = min(S + max(len(h["tokens"]) for _, h in rows) + 1, S + max_new_tokens)
    ids = np.full((len(rows), width), pad, dtype=np.int64)
    lps = np.full((len(rows), width - S), np.nan)
    for i, (e, h) in enumerate(rows):
        n = len(h["tokens"])
        ids[i, :S] = prompts[e]
        ids[i, S:S + n] = h["tokens"]
        lps[i, :n] = h["logprobs"][:n]
        if S + n < width and eos is not None and eos >= 0:
            ids[i, S + n] = eos
            if h["eos"]:
                lps[i, n] = h["logprobs"][n]
    return ids, lps


def beam_search(row_of, prompt_lens, beams, max_new_tokens, eos=-1, pad=0, length_penalty=1.0, early_stopping=False, num_return_sequences=1):
    """The whole loop on a model given as ``row_of(example, generated tokens) -> logits row``.  Returns (BeamRef, hypotheses)."""
    ref = BeamRef(prompt_lens, beams, eos, pad, length_penalty, early_stopping)
    for _ in range(max_new_tokens):
        logits = np.stack([row_of(s // beams, ref.tokens_of_slot(s) if ref.steps else []) for s in range(ref.N * beams)])
        ref.step(logits)
        if all(ref.done):
            break
    return ref, ref.finalize(num_return_sequences)
