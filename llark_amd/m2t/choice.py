"""The token choice of every generate path, and the padded-batch loop both wrappers share.

One step's choice is a composition of up to four stages, each with per-slot state on the device (:mod:`.constraints`, :mod:`.guide`,
:mod:`.sampling`, :mod:`.logprob`).  :class:`TokenChooser` owns the four parts and is the single home of their ORDER:

1. constraints: ``DeviceConstraints.process`` turns the raw logits into the rows with -inf at the banned tokens.  The ban comes before
   the repetition penalty.  The history it bans from is the row's own prompt (what :meth:`TokenChooser.admit` copied in), then the
   tokens this chooser handed that slot: a call that directly follows an ``admit`` sees prefill rows and appends nothing, every other
   call first appends the tokens of the call before it;
2. guide: ``DeviceGuide.process`` sets -inf at every token with which the row would leave its choice set (a slot without a set passes
   through bit for bit), on the rows stage 1 produced.  Its node steps by the same per-slot token stage 1 appends, under the same
   prefill rule.  A caller that passes no ``state`` (the uniform loops) gets the EOS rule from the chooser itself: a row that was
   handed ``eos`` is finished, is skipped by every stage from then on and keeps emitting ``eos``;
3. the choice, on the processed rows (the raw rows without stages 1 and 2): the ``DeviceSampler``, else the caller's ``choose(rows)``
   (the uniform loops' ``argmax`` / ``torch.multinomial``), else the advance kernel's own first-maximum rule;
4. log-probabilities: ``LogprobTracker`` on the RAW logits and the chosen tokens -- the model's own distribution, whatever stages 1 to 3
   did to the row;
5. the tokens are kept per slot for the next call's stages 1 and 2.

With every stage off there is no chooser (:meth:`TokenChooser.build` returns None): callers keep their plain calls, and nothing is
launched or allocated.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import ops
from .constraints import DeviceConstraints
from .guide import DeviceGuide
from .logprob import LogprobTracker
from .sampling import DeviceSampler


def first_maximum(rows: torch.Tensor, vocab: int, n_slots: int, state=None, slot_of_row=None) -> torch.Tensor:
    """The greedy token of every row by the rule of ``decode_advance_rows``: the first maximal index (one ``ops.sample_rows`` launch)."""
    return ops.sample_rows(rows, torch.zeros((rows.shape[0],), dtype=torch.int64, device=rows.device), vocab=vocab, state=state,
                           slot_of_row=slot_of_row, do_sample=False, repetition_penalty=1.0, slots=n_slots)


class TokenChooser:
    """``chooser(logits, state=None, slot_of_row=None) -> int64 tokens [rows]`` in the order of the module docstring; ``state`` and
    ``slot_of_row`` as the three parts take them (only ROW_ACTIVE slots are touched; row r belongs to slot ``slot_of_row[r]``).

    ``sampling`` (SamplingParams), ``constraints`` (TokenConstraints), ``guide`` (ChoiceSets), ``logprobs``: the stages that are on,
    None / False: off.  ``history_len``: the longest history a slot may reach (prompt + new tokens); ``logprob_width``: the most tokens
    a slot may generate; ``eos``: the token ``min_new_tokens`` / ``min_length`` ban and a whole sequence of a choice set allows (a
    guide needs one).  The parts are the attributes ``cons``, ``guide``, ``sampler``, ``tracker``."""

    def __init__(self, n_slots: int, vocab: int, device, *, sampling=None, constraints=None, guide=None, logprobs: bool = False,
                 history_len: Optional[int] = None, logprob_width: Optional[int] = None, eos: Optional[int] = None, choose=None):
        self.n_slots, self.vocab, self.device, self.choose = n_slots, vocab, torch.device(device), choose
        self.cons = None if constraints is None else DeviceConstraints(constraints, n_slots, vocab, history_len, device, eos)
        self.guide = None if guide is None else DeviceGuide(guide, n_slots, vocab, device, eos)
        self.alive = None                                          # int32 [n_slots] ROW_* states of a guided caller that passes no state
        self.sampler = None if sampling is None else DeviceSampler(sampling, n_slots, vocab, device)
        self.tracker = LogprobTracker(n_slots, vocab, device, logprob_width) if logprobs else None
        self.last = None                                           # int64 [n_slots]: the token each slot was handed last (stage 4)
        self._admitted = False

    @classmethod
    def build(cls, n_slots: int, vocab: int, device, *, sampling=None, constraints=None, guide=None, logprobs: bool = False, **kw):
        """The chooser, or None when no stage is on (a ``choose`` alone is the caller's plain call)."""
        if sampling is None and constraints is None and guide is None and not logprobs:
            return None
        return cls(n_slots, vocab, device, sampling=sampling, constraints=constraints, guide=guide, logprobs=logprobs, **kw)

    def admit(self, slots: Sequence[int], prompts: Sequence[torch.Tensor], stream_ids: Optional[Sequence[int]] = None,
              choice: Optional[Sequence[Optional[int]]] = None) -> None:
        """Before the slots' first token: ``prompts`` are the rows' own whole prompts (the history, the seen tokens); ``stream_ids``
        the examples' random streams (default: the slots); ``choice`` the index of each slot's choice set, None for an unconstrained
        slot (default: all unconstrained).  The next call is these slots' prefill call."""
        if self.cons is not None:
            self.cons.admit(slots, prompts)
        if self.guide is not None:
            slots = list(slots)
            self.guide.admit(slots, [None] * len(slots) if choice is None else choice)
            if self.alive is None:
                self.alive = torch.full((self.n_slots,), ops.ROW_IDLE, dtype=torch.int32, device=self.device)
            self.alive[torch.tensor([int(b) for b in slots], dtype=torch.long, device=self.device)] = ops.ROW_ACTIVE
        if self.sampler is not None:
            self.sampler.admit(slots, prompts, slots if stream_ids is None else stream_ids)
        if self.tracker is not None:
            self.tracker.admit(slots)
        self._admitted = True

    def release(self, slots: Sequence[int]) -> None:
        if self.sampler is not None:
            self.sampler.release(slots)
        if self.cons is not None:
            self.cons.release(slots)
        if self.guide is not None:
            self.guide.release(slots)

    def __call__(self, logits: torch.Tensor, state=None, slot_of_row=None) -> torch.Tensor:
        if logits.dim() == 3 and logits.shape[1] == 1:
            logits = logits[:, 0]
        if slot_of_row is not None:
            slot_of_row = torch.as_tensor(slot_of_row, dtype=torch.int32, device=self.device)
        prefill, self._admitted = self._admitted, False
        own_state = self.guide is not None and state is None and slot_of_row is None and logits.shape[0] == self.n_slots
        if own_state:
            state = self.alive
        rows = logits
        if self.cons is not None:
            rows = self.cons.process(logits, state=state, slot_of_row=slot_of_row, last=None if prefill else self.last)
        if self.guide is not None:
            rows = self.guide.process(rows, state=state, slot_of_row=slot_of_row, last=None if prefill else self.last)
        if self.sampler is not None:
            tokens = self.sampler(rows, state=state, slot_of_row=slot_of_row)
        elif self.choose is not None:
            tokens = self.choose(rows).reshape(-1)
        else:
            tokens = first_maximum(rows, self.vocab, self.n_slots, state, slot_of_row)
        if own_state:                                              # the EOS rule of a caller without states
            eos = torch.full_like(tokens, self.guide.eos)
            tokens = torch.where(state == ops.ROW_ACTIVE, tokens, eos)
            self.alive = torch.where(tokens == eos, torch.full_like(state, ops.ROW_FINISHED), state)
        if self.tracker is not None:
            self.tracker(logits, tokens, state=state, slot_of_row=slot_of_row)
        if self.cons is not None or self.guide is not None:
            if self.last is None:
                self.last = torch.zeros((self.n_slots,), dtype=torch.int64, device=self.device)
            if slot_of_row is None:
                self.last[: tokens.numel()] = tokens
            else:
                self.last[slot_of_row.long()] = tokens
        return tokens

    def take_logprobs(self, slots: Sequence[int]):
        """``LogprobTracker.take``: per slot its history so far, one transfer for all."""
        return self.tracker.take(slots)

    def logprob_matrix(self, n: int) -> torch.Tensor:
        """fp32 [n_slots, n] on the device: each slot's history, NaN from its ``count`` on (where a finished row emitted padding)."""
        t = self.tracker
        cols = torch.arange(n, device=t.device)[None, :]
        return torch.where(cols < t.count[:, None], t.hist[:, :n], torch.full((), float("nan"), device=t.device))

    def finish(self) -> None:
        """Raises when a history row was full, so that bans were computed from a history that lacks tokens, and when a guided row had no
        allowed token left."""
        if self.cons is not None:
            self.cons.check()
        if self.guide is not None:
            self.guide.check()


def unpack_prompts(input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor]):
    """A padded batch -> ``(rows, lens, packed)``: row b is ``input_ids[b][mask[b]]`` (all of it without a mask; 1-D int64, CPU), its
    length, and the rows left-aligned in one zero-padded tensor for the splice plan."""
    B, S = input_ids.shape
    am = torch.ones((B, S), dtype=torch.bool) if attention_mask is None else attention_mask.to(device="cpu", dtype=torch.bool)
    if am.shape != (B, S):
        raise ValueError(f"attention_mask shape {tuple(am.shape)} does not match input_ids {(B, S)}")
    lens = am.sum(1)
    if bool((lens == 0).any()):
        raise ValueError("attention_mask selects no token in some row")
    ids_cpu = input_ids.detach().cpu()
    rows = [ids_cpu[b][am[b]] for b in range(B)]
    packed = torch.zeros((B, int(lens.max())), dtype=torch.int64)
    for b, r in enumerate(rows):
        packed[b, : r.numel()] = r
    return rows, [int(n) for n in lens], packed


def generate_padded(eng, rows, segs, input_ids, eos_k: int, pad_k: int, max_new_tokens: int, stopping_criteria=None, *, sampling=None,
                    constraints=None, return_logprobs: bool = False, choose=None, guide=None, choice=None):
    """``generate`` over a padded batch on either engine: row b (``rows[b]``, :func:`unpack_prompts`) runs at positions 0 .. len_b - 1
    (HF's position_ids = cumsum(mask) - 1) in engine slot b (``prefill_slots`` / ``decode_slots``); ``segs``: the audio splice plan of the
    packed rows.  ``eos_k`` < 0: no EOS.  Returns the HF layout -- ``input_ids`` as given followed by the new tokens; a row that emitted
    EOS continues with ``pad_k`` -- and with ``return_logprobs`` the pair ``(ids, logprobs [B, new tokens])``.  ``stopping_criteria`` are
    called as ``c(ids so far, the step's raw logits)``.  ``guide`` (ChoiceSets) with ``choice`` (a set index or None per row): stage 2 of
    the chooser."""
    B, S = input_ids.shape
    out = torch.empty((B, S + max(max_new_tokens, 0)), dtype=torch.int64, device=eng.device)
    out[:, :S] = input_ids.to(eng.device)
    if max_new_tokens <= 0:
        return (out, torch.empty((B, 0), dtype=torch.float32, device=eng.device)) if return_logprobs else out
    eng.init_slots(B)
    scores = eng.prefill_slots([r.to(eng.device) for r in rows], segs, range(B))
    chooser = TokenChooser.build(B, scores.shape[-1], eng.device, sampling=sampling, constraints=constraints, logprobs=return_logprobs,
                                 history_len=max(r.numel() for r in rows) + max_new_tokens, logprob_width=max_new_tokens, eos=eos_k,
                                 choose=choose, **({} if guide is None else dict(guide=guide)))
    sample = None
    if chooser is not None:
        chooser.admit(range(B), rows, **({} if guide is None else dict(choice=choice)))

        def sample(scores):
            return chooser(scores, state=eng.slot_state)
    elif choose is not None:
        sample = choose
    nxt, _ = eng.advance_slots(scores, eos_k, pad_k, out[:, S], None if sample is None else sample(scores), advance=False)
    n = 1
    while True:
        if eos_k >= 0 and all(st != ops.ROW_ACTIVE for st in eng.slot_state_host):
            break
        if stopping_criteria is not None and any(bool(c(out[:, : S + n], scores)) for c in stopping_criteria):
            break
        if n == max_new_tokens:
            break
        nxt, _, scores = eng.decode_slots(nxt, eos_k, pad_k, out[:, S + n], sample)
        n += 1
    if chooser is None:
        return out[:, : S + n]
    chooser.finish()
    return (out[:, : S + n], chooser.logprob_matrix(n)) if return_logprobs else out[:, : S + n]
