"""Token log-probabilities on the device: the per-slot history that ``ops.token_logprob_rows`` appends to, one launch per step.

The values are log-probabilities of the MODEL's distribution -- log-softmax of the raw logits.  Repetition penalty, temperature, top-k
and top-p are not applied, for sampled tokens too: the number says how probable the model found the token, not how probable the
sampler's reshaped distribution made it.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from .. import ops


class LogprobTracker:
    """``tracker(logits, tokens, state=None, slot_of_row=None) -> fp32 log-probabilities``, one ``ops.token_logprob_rows`` launch that
    also appends each evaluated row's value to its slot's history (``hist`` fp32 [n_slots, width], ``count``, ``total``).

    ``admit(slots)`` before a slot's first token zeroes its ``count`` and ``total``; ``take(slots)`` hands a finished example's
    whole history back in ONE device-to-host transfer, so a decode step keeps its single transfer.  ``width`` is the engine's
    ``max_seq``: a slot cannot generate more tokens than that.  The values are log-softmax of the raw logits (module docstring)."""

    def __init__(self, n_slots: int, vocab: int, device, width: int):
        if n_slots < 1 or vocab < 1 or width < 1:
            raise ValueError(f"LogprobTracker: need n_slots, vocab and width >= 1, got {n_slots}, {vocab}, {width}")
        self.n_slots, self.vocab, self.width, self.device = n_slots, vocab, width, torch.device(device)
        self.hist = torch.zeros((n_slots, width), dtype=torch.float32, device=self.device)
        self.count = torch.zeros((n_slots,), dtype=torch.int32, device=self.device)
        self.total = torch.zeros((n_slots,), dtype=torch.float32, device=self.device)

    def _index(self, slots: Sequence[int], what: str) -> torch.Tensor:
        slots = [int(b) for b in slots]
        if any(not 0 <= b < self.n_slots for b in slots) or len(set(slots)) != len(slots):
            raise ValueError(f"LogprobTracker.{what}: bad slot list {slots}")
        return torch.tensor(slots, dtype=torch.long, device=self.device)

    def admit(self, slots: Sequence[int]) -> None:
        idx = self._index(slots, "admit")
        self.count[idx] = 0
        self.total[idx] = 0

    def __call__(self, logits: torch.Tensor, tokens: torch.Tensor, state: Optional[torch.Tensor] = None,
                 slot_of_row: Optional[torch.Tensor] = None) -> torch.Tensor:
        if logits.dim() == 3 and logits.shape[1] == 1:
            logits = logits[:, 0]
        out = torch.full((logits.shape[0],), float("nan"), dtype=torch.float32, device=self.device)
        if slot_of_row is not None:
            slot_of_row = torch.as_tensor(slot_of_row, dtype=torch.int32, device=self.device)
        tokens = torch.as_tensor(tokens, dtype=torch.int64, device=self.device).reshape(-1)
        return ops.token_logprob_rows(logits, tokens, out, vocab=self.vocab, state=state, slot_of_row=slot_of_row, hist=self.hist,
                                      count=self.count, total=self.total, slots=self.n_slots)

    def take(self, slots: Sequence[int]) -> List[torch.Tensor]:
        """Per slot, its history so far: a 1-D fp32 CPU tensor of length ``count`` (capped at ``width``).  One transfer for all."""
        idx = self._index(slots, "take")
        if idx.numel() == 0:
            return []
        packed = torch.cat((self.hist[idx], self.count[idx].to(torch.float32)[:, None]), dim=1).cpu()      # counts <= 2^24: exact in fp32
        return [packed[i, : min(int(packed[i, -1]), self.width)].clone() for i in range(len(idx))]
