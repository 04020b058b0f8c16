"""Beam search on the device: HF 4.29.2's ``beam_search`` + ``BeamSearchScorer`` with one beam group on the ragged slot mode.

:class:`BeamSearch` owns the device state of N examples x B beams -- example e lives in the engine slots e * B .. e * B + B - 1 -- and
runs a step as three launches after the logits (``ops.beam_topk_rows``, ``ops.beam_advance``, ``ops.kv_copy_slots``; contracts in
include/llark_hip.h).  Nothing but the next ids and the done flags comes back to the host during the loop; the hypotheses' tokens and
per-token log-probabilities are found at the end by walking the trellis that the steps wrote.

Semantics: beam scores start at (0, -1e9, ...); a candidate is fp32(score + log-softmax of the RAW logits); the top 2B candidates are
ordered by value descending, then rank, then token ascending (torch.topk has no tie rule; this is ours); an eos among the first B places
closes a hypothesis of score sum / length ** length_penalty, where the length counts the example's own prompt (without padding); an
example is done when its heap is full and (``early_stopping`` or its worst hypothesis is at least the best candidate / cur_len **
length_penalty).  Ties between hypotheses go to the one that arrived first."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import ops

MAX_SLOTS = 64


def check_beam_args(num_beams, num_return_sequences=1, length_penalty=1.0, n_examples: int = 1) -> Tuple[int, int, float]:
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= ops.BEAM_MAX:
        raise ValueError(f"num_beams must be an integer in 1 .. {ops.BEAM_MAX}, got {num_beams!r}")
    r = 1 if num_return_sequences is None else num_return_sequences
    if isinstance(r, bool) or not isinstance(r, int) or not 1 <= r <= num_beams:
        raise ValueError(f"num_return_sequences must be an integer in 1 .. num_beams = {num_beams}, got {num_return_sequences!r}")
    lp = float(length_penalty)
    if not np.isfinite(lp):
        raise ValueError(f"length_penalty must be finite, got {length_penalty!r}")
    if n_examples * num_beams > MAX_SLOTS:
        raise ValueError(f"{n_examples} examples x {num_beams} beams need {n_examples * num_beams} slots; the slot mode has {MAX_SLOTS}")
    return num_beams, r, lp


class BeamSearch:
    def __init__(self, n_examples: int, beams: int, vocab: int, max_steps: int, device, eos: Optional[int] = None, pad: int = 0,
                 length_penalty: float = 1.0, early_stopping: bool = False):
        self.beams, _, self.length_penalty = check_beam_args(beams, 1, length_penalty, n_examples)
        if max_steps < 1:
            raise ValueError(f"max_steps must be >= 1, got {max_steps}")
        self.n, self.vocab, self.max_steps, self.device = int(n_examples), int(vocab), int(max_steps), torch.device(device)
        self.eos = -1 if eos is None or eos < 0 else int(eos)
        self.pad, self.early_stopping = int(pad), bool(early_stopping)
        N, B, dev = self.n, self.beams, self.device
        slots = self.slots = N * B
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.score = torch.full((slots,), -1e9, **f32)
        self.score[::B] = 0.0
        self.rank_of_slot = torch.arange(B, **i32).repeat(N)
        self.cand_score = torch.zeros((slots, 2 * B), **f32)
        self.cand_token = torch.zeros((slots, 2 * B), **i32)
        self.cand_logprob = torch.zeros((slots, 2 * B), **f32)
        self.next_ids = torch.zeros((slots,), dtype=torch.int64, device=dev)
        self.heap = torch.zeros((N, B, ops.BEAM_HEAP_STRIDE), **i32)
        self.heap_meta = torch.zeros((N, ops.BEAM_META_STRIDE), **i32)
        self.heap_meta[:, 1] = torch.tensor([1e9], **f32).view(torch.int32)
        self.done = torch.zeros((N,), **i32)
        self.cur_len = torch.zeros((N,), **i32)
        self.p0 = torch.zeros((slots,), **i32)
        self.trellis = torch.zeros((self.max_steps, slots, 3), **i32)
        self.pairs = torch.zeros((N, max(B - 1, 1), 2), **i32)
        self.pair_count = torch.zeros((N,), **i32)
        self.fallbacks = torch.zeros((1,), **i32)
        self.steps = 0
        self.done_host: List[bool] = [False] * N
        self.len_host: List[int] = [0] * N
        self.p0_host: List[int] = [0] * N
        # test hooks: observe_logits(step, logits) before the step's launches, observe_move(step, "before" / "after") around the K/V move
        self.observe_logits = self.observe_move = None
        # a llark_amd.m2t.constraints.DeviceConstraints over the same slots (admitted by the caller): banned tokens are left out of the
        # candidates; None: the unconstrained launch
        self.constraints = None
        # a llark_amd.m2t.guide.DeviceGuide over the same slots (admitted by the caller): tokens outside a slot's choice set are left
        # out of the candidates too -- its bitmap is OR-ed into the constraints' when both are on; None: no such launch.  Inside a closed
        # set an example soon has fewer continuations than beams: with a guide the step is ops.beam_advance(open=True), which goes on
        # while ANY beam lives; a slot without a beam has the score -inf, is fed pad and is taken again when a later step forks into it
        self.guide = None

    def admit(self, prompt_lens: Sequence[int]) -> None:
        """The examples' prompt lengths: cur_len, and the first position a K/V move has to copy (the slots of an example are clones of
        its prompt, so everything below the last multiple of 8 of its length is the same in all of them, for good)."""
        lens = [int(x) for x in prompt_lens]
        if len(lens) != self.n or min(lens) < 1:
            raise ValueError(f"BeamSearch.admit: {self.n} positive prompt lengths expected, got {lens}")
        self.len_host, self.p0_host = lens, [x // 8 * 8 for x in lens]
        self.cur_len.copy_(torch.tensor(lens, dtype=torch.int32))
        self.p0.copy_(torch.tensor(self.p0_host, dtype=torch.int32).repeat_interleave(self.beams))

    def step(self, logits: torch.Tensor, state: torch.Tensor, pos_rows: Optional[torch.Tensor] = None, kv=None,
             last: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, List[bool]]:
        """One step from fp32 ``logits`` [slots, >= vocab] (row = slot).  ``state``: the slots' ROW_* states; ``pos_rows``: their cache
        lengths, advanced by one for the rows of examples that are not done (None: nothing advances); ``kv`` = (k_cache, vt_cache,
        k_cache_lo, vt_cache_lo): the caches in which forked beams receive their parent's positions (None: no move).  ``last`` (with
        ``constraints``): the ids the logits were computed from, None on the prompts' logits; a slot's history then follows its beam --
        the parent column of the previous trellis row says whose history it continues.  Returns (next ids [slots] on the device, the
        examples' done flags on the host)."""
        if self.steps >= self.max_steps:
            raise RuntimeError(f"BeamSearch.step: all {self.max_steps} steps are used")
        assert logits.shape[0] == self.slots and logits.shape[1] >= self.vocab
        N, B = self.n, self.beams
        if self.observe_logits is not None:
            self.observe_logits(self.steps, logits)
        ban = None
        if self.constraints is not None or self.guide is not None:
            if (last is None) != (self.steps == 0):
                raise ValueError("BeamSearch.step: constraints and a guide need `last` on every step but the first")
            parent = None if last is None else self.trellis[self.steps - 1, :, 0]
            if self.constraints is not None:
                ban = self.constraints.process(logits, state=state, last=last, parent=parent, bitmap=True)
            if self.guide is not None:
                ban = self.guide.process(logits, state=state, last=last, parent=parent, bitmap=True, ban=ban)
        ops.beam_topk_rows(logits, self.score, B, self.cand_score, self.cand_token, self.cand_logprob, vocab=self.vocab, state=state,
                           fallbacks=self.fallbacks, **({} if ban is None else dict(ban=ban)))
        ops.beam_advance(self.cand_score, self.cand_token, self.cand_logprob, N, B, self.steps, self.eos, self.pad, self.length_penalty,
                         self.early_stopping, self.score, self.rank_of_slot, state, pos_rows, self.cur_len, self.next_ids, self.heap,
                         self.heap_meta, self.done, self.trellis, self.pairs, self.pair_count,
                         **({} if self.guide is None else dict(open=True)))
        for e in range(N):
            if not self.done_host[e]:
                self.len_host[e] += 1
        if kv is not None and B > 1 and pos_rows is not None:
            if self.observe_move is not None:
                self.observe_move(self.steps, "before")
            span = max(self.len_host[e] - 1 - self.p0_host[e] for e in range(N))
            ops.kv_copy_slots(kv[0], kv[1], self.pairs, self.pair_count, self.p0, pos_rows, max(1, span), kv[2], kv[3])
            if self.observe_move is not None:
                self.observe_move(self.steps, "after")
        self.steps += 1
        host = torch.cat((self.next_ids, self.done.to(torch.int64))).cpu()
        self.done_host = [bool(x) for x in host[self.slots:].tolist()]
        return self.next_ids, self.done_host

    # ---- the end -----------------------------------------------------------------------------------------------------------------
    def hypotheses(self, num_return_sequences: int = 1) -> List[List[dict]]:
        """Per example its ``num_return_sequences`` best hypotheses, best first: the live beams of an example that is not done are
        added in rank order first (length = its current length).  Each: tokens, logprobs (one per token, the closing eos' included
        when it ended on one), score, sum, length, eos.  One transfer of the state; the trellis is walked on the host."""
        N, B, T = self.n, self.beams, self.steps
        _, R, _ = check_beam_args(B, num_return_sequences, self.length_penalty)
        score, rank, done, cur = (t.cpu().numpy() for t in (self.score, self.rank_of_slot, self.done, self.cur_len))
        heap, meta = self.heap.cpu().numpy(), self.heap_meta.cpu().numpy()
        tr = self.trellis[:T].cpu().numpy()
        tr_lp = np.ascontiguousarray(tr[:, :, 2]).view(np.float32)
        hf = heap.view(np.float32)
        out = []
        for e in range(N):
            entries = [dict(score=hf[e, i, 0], sum=hf[e, i, 1], length=int(heap[e, i, 2]), end_step=int(heap[e, i, 3]),
                            end_slot=int(heap[e, i, 4]), arrival=int(heap[e, i, 5]), eos_lp=float(hf[e, i, 6])) for i in range(int(meta[e, 0]))]
            arrivals = int(meta[e, 2])
            if not done[e]:
                for r in range(B):
                    slot = e * B + int(np.nonzero(rank[e * B:e * B + B] == r)[0][0])
                    if np.isneginf(score[slot]):                   # a slot without a beam (the open step)
                        continue
                    sc = np.float32(np.float64(score[slot]) / np.float64(int(cur[e])) ** np.float64(self.length_penalty))
                    new = dict(score=sc, sum=score[slot], length=int(cur[e]), end_step=T, end_slot=slot, arrival=arrivals, eos_lp=float("nan"))
                    arrivals += 1
                    if len(entries) < B:
                        entries.append(new)
                    elif sc > min(h["score"] for h in entries):
                        entries[min(range(B), key=lambda i: (entries[i]["score"], entries[i]["arrival"]))] = new
            hyps = []
            for h in sorted(entries, key=lambda h: (-float(h["score"]), h["arrival"]))[:R]:
                toks, lps, slot = [], [], h["end_slot"]
                for s in range(h["end_step"] - 1, -1, -1):
                    toks.append(int(tr[s, slot, 1])), lps.append(float(tr_lp[s, slot]))
                    slot = int(tr[s, slot, 0])
                ended = not np.isnan(h["eos_lp"])
                hyps.append(dict(tokens=toks[::-1], logprobs=lps[::-1] + ([h["eos_lp"]] if ended else []), score=float(h["score"]),
                                 sum=float(h["sum"]), length=h["length"], eos=ended))
            if len(hyps) < R:
                raise RuntimeError(f"beam search: example {e} has {len(hyps)} hypotheses, {R} asked for")
            out.append(hyps)
        return out

    def finalize(self, prompts: torch.Tensor, max_new_tokens: int, num_return_sequences: int = 1):
        """HF's layout: (ids int64 [N * R, width], logprobs fp32 [N * R, width - S], scores fp32 [N * R]) on the device.  ``prompts``
        [N, S] as given (padding included); width = min(longest + 1, S + max_new_tokens); a row shorter than the width gets eos right
        after its last token whether or not it ended on eos (HF does this), the rest is pad.  logprobs: NaN where nothing was chosen."""
        hyps = self.hypotheses(num_return_sequences)
        S = prompts.shape[1]
        rows = [(e, h) for e, hs in enumerate(hyps) for h in hs]
        width = min(S + max(len(h["tokens"]) for _, h in rows) + 1, S + max_new_tokens)
        ids = torch.full((len(rows), width), self.pad, dtype=torch.int64)
        lps = torch.full((len(rows), width - S), float("nan"), dtype=torch.float32)
        pc = prompts.detach().cpu()
        for i, (e, h) in enumerate(rows):
            n = len(h["tokens"])
            ids[i, :S] = pc[e]
            ids[i, S:S + n] = torch.tensor(h["tokens"], dtype=torch.int64)
            lps[i, :n] = torch.tensor(h["logprobs"][:n], dtype=torch.float32)
            if S + n < width and self.eos >= 0:
                ids[i, S + n] = self.eos
                if h["eos"]:
                    lps[i, n] = h["logprobs"][n]
        scores = torch.tensor([h["score"] for _, h in rows], dtype=torch.float32)
        return ids.to(self.device), lps.to(self.device), scores.to(self.device)

    # ---- what a stopping criterion sees (only kept when there is one) ---------------------------------------------------------------
    def extend_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """``ids`` [slots, len] in SLOT order as they were before the last step -> [slots, len + 1] after it: every slot takes its
        parent's row and its new token (pad for a done example).  Device tensors only, nothing is read back."""
        parent = self.trellis[self.steps - 1, :, 0].to(torch.int64)
        own = torch.arange(self.slots, dtype=torch.int64, device=self.device)
        return torch.cat((ids.index_select(0, torch.where(parent < 0, own, parent)), self.next_ids[:, None]), dim=1)

    def by_rank(self, ids: torch.Tensor) -> torch.Tensor:
        """Rows in slot order -> HF's order: example by example, its beams by rank."""
        own = torch.arange(self.slots, dtype=torch.int64, device=self.device)
        return ids.index_select(0, torch.argsort(own // self.beams * self.beams + self.rank_of_slot.to(torch.int64)))
