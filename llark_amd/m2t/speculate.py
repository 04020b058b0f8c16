"""Speculative greedy decoding by prompt lookup (HF's later ``prompt_lookup_num_tokens`` / ``max_matching_ngram_size``): every decode
step feeds a block of up to K drafted tokens behind the token the plain step would feed, and keeps the drafts that equal the model's own
greedy choice (``HipLlamaEngine.decode_block``: ``llark_attn_decode_rope_bf16_block``, ``llark_spec_verify_rows``,
``llark_spec_draft_rows``).  The drafts come from the row's own history: the longest suffix of G .. 1 tokens that occurs earlier, and the
tokens that followed its most recent occurrence.  No draft model.  Greedy verification reproduces the block step's own greedy decoding
whatever was drafted; it equals the plain loop's token for token where the decode Linears give a row the same bits at n_slots and at
n_slots * (K + 1) rows.  Off by default."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch

from .. import ops

MAX_ROWS = 16                 # rows of a block step: the m <= 16 decode Linears


@dataclass(frozen=True)
class SpeculationParams:
    """``num_tokens`` K drafted tokens per step (1 .. 7), suffixes of up to ``max_ngram`` G tokens (1 .. 64)."""
    num_tokens: int
    max_ngram: int = 2

    def __post_init__(self):
        for name, v, lo, hi in (("prompt_lookup_num_tokens", self.num_tokens, 1, ops.SPEC_MAX_BLOCK - 1), ("max_matching_ngram_size", self.max_ngram, 1, 64)):
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"{name} must be an integer in {lo} .. {hi}, got {v!r}")

    @property
    def stride(self) -> int:
        return self.num_tokens + 1

    def check_batch(self, batch: int) -> None:
        if batch * self.stride > MAX_ROWS:
            raise ValueError(f"prompt_lookup_num_tokens={self.num_tokens}: B * (K + 1) = {batch} * {self.stride} rows per step exceed {MAX_ROWS}")

    @staticmethod
    def from_generate(prompt_lookup_num_tokens, max_matching_ngram_size=None, **others) -> Optional["SpeculationParams"]:
        """``None`` / 0: speculation is off and nothing else is looked at.  Otherwise every argument of ``generate`` that speculative
        greedy decoding does not cover is refused by name (``others``: name -> whether it was given)."""
        if prompt_lookup_num_tokens is None or (prompt_lookup_num_tokens == 0 and not isinstance(prompt_lookup_num_tokens, bool)):
            return None
        p = SpeculationParams(prompt_lookup_num_tokens, 2 if max_matching_ngram_size is None else max_matching_ngram_size)
        for name, given in others.items():
            if given:
                raise NotImplementedError(f"prompt_lookup_num_tokens with {name} is not implemented: speculative decoding verifies plain greedy choices only")
        return p


class PromptLookup:
    """The host restatement of the device lookup (``llark_spec_draft_rows``): ``PromptLookup(K, G)(history) -> drafts``."""

    def __init__(self, num_tokens: int, max_ngram: int = 2):
        self.params = SpeculationParams(num_tokens, max_ngram)

    def __call__(self, hist: Sequence[int]) -> List[int]:
        hist = list(hist)
        n = len(hist)
        for g in range(self.params.max_ngram, 0, -1):
            if n < g + 1:
                continue
            for s in range(n - g - 1, -1, -1):
                if hist[s:s + g] == hist[n - g:]:
                    return hist[s + g:n][: self.params.num_tokens]
        return []


def generate_speculative(eng, rows, segs, input_ids, eos_k: int, pad_k: int, max_new_tokens: int, params: SpeculationParams,
                         stopping_criteria=None, drafter: Optional[Callable[[int, List[int]], Sequence[int]]] = None, stats: Optional[dict] = None):
    """``generate`` on the slot mode with block steps: row b (``rows[b]``, choice.unpack_prompts) in slot b.  Returns the HF layout of
    choice.generate_padded.  ``stopping_criteria`` see the tokens one step at a time -- ``c(ids with n new tokens, the [B, V] logits
    those tokens were chosen from)`` -- as the plain loop shows them; when one fires inside an accepted run the rest is dropped and the
    slots are truncated to the state the plain loop leaves (prompt + kept tokens - 1 positions: the last token is not fed yet).
    ``drafter(b, new tokens of row b so far) -> drafts`` replaces the lookup (the caller-tensor form of the kernel); ``stats`` receives
    ``steps``, ``drafted`` and ``accepted``."""
    B, S = input_ids.shape
    K = params.num_tokens
    params.check_batch(B)
    dev = eng.device
    total = S + max(max_new_tokens, 0)
    out = torch.full((B, total), pad_k, dtype=torch.int64, device=dev)
    out[:, :S] = input_ids.to(dev)
    if max_new_tokens <= 0:
        return out
    eng.init_slots(B)
    scores = eng.prefill_slots([r.to(dev) for r in rows], segs, range(B))
    _, first = eng.advance_slots(scores, eos_k, pad_k, out[:, S], None, advance=False)
    new: List[List[int]] = [[int(first[b])] for b in range(B)]           # the new tokens of every row
    lens0 = [int(r.numel()) for r in rows]
    watch = stopping_criteria is not None and len(stopping_criteria) > 0
    seen: List[List[torch.Tensor]] = [[scores[b].clone()] for b in range(B)] if watch else []
    st = dict(steps=0, drafted=0, accepted=0)
    shown = 0                                                            # steps the criteria have seen

    def done(b):
        return eng.slot_state_host[b] != ops.ROW_ACTIVE or len(new[b]) >= max_new_tokens

    def show() -> bool:
        """hand the criteria every step that all unfinished rows have reached; True: one fired at step `shown`"""
        nonlocal shown
        while True:
            reach = min([len(new[b]) for b in range(B) if not done(b)] or [max(len(x) for x in new)])
            if shown >= reach:
                return False
            shown += 1
            ids = out[:, : S + shown].clone()
            sc = torch.stack([seen[b][min(shown, len(seen[b])) - 1] for b in range(B)])
            for b in range(B):
                k = min(shown, len(new[b]))
                ids[b, S:S + k] = torch.tensor(new[b][:k], dtype=torch.int64, device=dev)
            if any(bool(c(ids, sc)) for c in stopping_criteria):
                return True

    stopped = watch and show()
    if not stopped and not all(done(b) for b in range(B)):
        eng.init_block_decode(params.stride)
        eng.start_block_decode([torch.cat((rows[b].reshape(-1).cpu(), torch.tensor(new[b], dtype=torch.int64))) for b in range(B)],
                               [max_new_tokens - 1] * B)
        while not all(done(b) for b in range(B)):
            kw = {}
            if drafter is not None:
                d = [list(drafter(b, list(new[b])))[:K] for b in range(B)]
                dt = torch.zeros((B, K), dtype=torch.int64)
                for b, x in enumerate(d):
                    dt[b, : len(x)] = torch.tensor(x, dtype=torch.int64)
                kw = dict(drafts=dt.to(dev), n_drafts=torch.tensor([len(x) for x in d], dtype=torch.int32, device=dev))
            emitted, ids_blk, logits = eng.decode_block(eos_k, pad_k, K, params.max_ngram, **kw)
            st["steps"] += 1
            if stats is not None or watch:
                blk = eng._block_ws["blk"].cpu().tolist()
            for b in range(B):
                if done(b) and not emitted[b]:
                    continue
                if not emitted[b]:
                    raise ValueError(f"slot {b} reached the engine's max_seq {eng.smax}")
                if stats is not None:
                    st["drafted"] += max(blk[b] - 1, 0)
                    st["accepted"] += len(emitted[b]) - 1
                if watch:
                    seen[b] += [logits[b * params.stride + i].clone() for i in range(len(emitted[b]))]
                new[b] += emitted[b]
            if watch and show():
                stopped = True
                break
    n = shown if stopped else max(len(x) for x in new)
    if stopped:                                                          # drop what lies behind the stop, in the output and in the slots
        cut = [b for b in range(B) if len(new[b]) > n]
        for b in cut:
            new[b] = new[b][:n]
        if cut:
            eng.truncate_slots(cut, [lens0[b] + n - 1 for b in cut])
    for b in range(B):
        out[b, S:S + len(new[b])] = torch.tensor(new[b], dtype=torch.int64, device=dev)
    if stats is not None:
        stats.update(st)
    return out[:, : S + n]
