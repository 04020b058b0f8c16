"""Sampling on the device: the callable that ``decode_slots(sample=...)`` / ``advance_slots(choice=...)`` of both engines accept.

:class:`SamplingParams` are the generation arguments of HF 4.29.2 that this project honours (``do_sample``, ``temperature``,
``top_k``, ``top_p``, ``repetition_penalty``) plus a ``seed``; :class:`DeviceSampler` owns the per-slot state of
``ops.sample_rows`` -- the bitmaps of the tokens each slot has seen (its prompt and what it generated), the draw counters and
the stream ids.  A draw is Philox4x32-10 under (seed; draw number, stream id): it depends on the example (its stream id) and
on how many tokens the example has drawn, never on the slot it landed in, on the slot count or on any host generator.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from .. import ops


@dataclass(frozen=True)
class SamplingParams:
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0                      # 0: off (HF's default of 50 is the caller's to pass)
    top_p: float = 1.0
    repetition_penalty: float = 1.0
    seed: int = 0

    def __post_init__(self):
        def number(name, v):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            return v
        if number("temperature", self.temperature) <= 0:
            raise ValueError(f"temperature must be > 0, got {self.temperature!r}")
        if isinstance(self.top_k, bool) or not isinstance(self.top_k, int) or self.top_k < 0:
            raise ValueError(f"top_k must be an integer >= 0 (0: off), got {self.top_k!r}")
        if not 0 < number("top_p", self.top_p) <= 1:
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p!r}")
        if number("repetition_penalty", self.repetition_penalty) <= 0:
            raise ValueError(f"repetition_penalty must be > 0, got {self.repetition_penalty!r}")
        if isinstance(self.seed, bool) or not isinstance(self.seed, int) or not -2 ** 63 <= self.seed < 2 ** 64:
            raise ValueError(f"seed must be an integer that fits 64 bits, got {self.seed!r}")

    @property
    def active(self) -> bool:
        """False when these parameters ask for nothing but the plain greedy token."""
        return bool(self.do_sample) or self.repetition_penalty != 1.0


def params_from_generate(do_sample, temperature, top_k, top_p, repetition_penalty, seed, always: bool = False) -> Optional[SamplingParams]:
    """The device sampler's parameters for a ``generate`` call, or None when the call does not ask for it: none of ``top_k`` /
    ``top_p`` / ``repetition_penalty`` / ``seed`` given (and not ``always``), or nothing but the plain greedy token asked for.
    Bad values raise whether or not the sampler ends up being used."""
    if not always and all(x is None for x in (top_k, top_p, repetition_penalty, seed)):
        return None
    params = SamplingParams(do_sample=bool(do_sample), temperature=temperature, top_k=0 if top_k is None else top_k,
                            top_p=1.0 if top_p is None else top_p,
                            repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty, seed=0 if seed is None else seed)
    return params if params.active else None


class DeviceSampler:
    """``sampler(logits, state=None, slot_of_row=None) -> int64 tokens``, one ``ops.sample_rows`` launch.

    ``admit(slots, prompts, stream_ids)`` before a slot's first token: clears its bitmap, marks its prompt, zeroes its draw
    counter and records its stream id (the example's index); ``release(slots)`` when its example is done."""

    def __init__(self, params: SamplingParams, n_slots: int, vocab: int, device):
        if n_slots < 1 or not 1 <= vocab <= 65536:
            raise ValueError(f"DeviceSampler: need n_slots >= 1 and 1 <= vocab <= 65536, got {n_slots}, {vocab}")
        self.params, self.n_slots, self.vocab, self.device = params, n_slots, vocab, torch.device(device)
        self.seen = torch.zeros((n_slots, (vocab + 31) // 32), dtype=torch.int32, device=self.device)
        self.draws = torch.zeros((n_slots,), dtype=torch.int32, device=self.device)
        self.stream_id = torch.arange(n_slots, dtype=torch.int64, device=self.device)
        self.fallbacks = torch.zeros((1,), dtype=torch.int32, device=self.device)
        seed = params.seed
        self._seed = seed - 2 ** 64 if seed >= 2 ** 63 else seed          # the 64 key bits, as the C ABI's long long

    def admit(self, slots: Sequence[int], prompts: Sequence[torch.Tensor], stream_ids: Sequence[int]) -> None:
        slots = [int(b) for b in slots]
        if len(prompts) != len(slots) or len(stream_ids) != len(slots):
            raise ValueError("DeviceSampler.admit: slots, prompts and stream_ids differ in length")
        if any(not 0 <= b < self.n_slots for b in slots) or len(set(slots)) != len(slots):
            raise ValueError(f"DeviceSampler.admit: bad slot list {slots}")
        idx = torch.tensor(slots, dtype=torch.long, device=self.device)
        self.seen[idx] = 0
        self.draws[idx] = 0
        self.stream_id[idx] = torch.tensor([int(s) for s in stream_ids], dtype=torch.int64, device=self.device)
        flat = [torch.as_tensor(p, dtype=torch.int64).reshape(-1) for p in prompts]
        lens = [p.numel() for p in flat]
        if sum(lens) == 0:
            return
        offs = [0]
        for n in lens[:-1]:
            offs.append(offs[-1] + n)
        i32 = dict(dtype=torch.int32, device=self.device)
        ops.seen_mark_rows(torch.cat([p.to(self.device) for p in flat]).contiguous(), torch.tensor(offs, **i32), torch.tensor(lens, **i32),
                           self.seen, self.vocab, slot_of_row=torch.tensor(slots, **i32))

    def release(self, slots: Sequence[int]) -> None:
        idx = torch.tensor([int(b) for b in slots], dtype=torch.long, device=self.device)
        self.seen[idx] = 0
        self.draws[idx] = 0

    def __call__(self, logits: torch.Tensor, state: Optional[torch.Tensor] = None, slot_of_row: Optional[torch.Tensor] = None) -> torch.Tensor:
        p = self.params
        if logits.dim() == 3 and logits.shape[1] == 1:
            logits = logits[:, 0]
        choice = torch.zeros((logits.shape[0],), dtype=torch.int64, device=self.device)
        if slot_of_row is not None:
            slot_of_row = torch.as_tensor(slot_of_row, dtype=torch.int32, device=self.device)
        return ops.sample_rows(logits, choice, vocab=self.vocab, state=state, slot_of_row=slot_of_row, seen=self.seen, do_sample=p.do_sample,
                               temperature=p.temperature, top_k=p.top_k, top_p=p.top_p, repetition_penalty=p.repetition_penalty,
                               seed=self._seed, draws=self.draws, stream_id=self.stream_id, fallbacks=self.fallbacks, slots=self.n_slots)

    def fallback_count(self) -> int:
        """Rows so far whose logits were degenerate (NaN, infinite maximum) and took the greedy token; a device-to-host read."""
        return int(self.fallbacks.item())
