"""Constrained decoding on the device: ``no_repeat_ngram_size``, ``bad_words_ids`` / ``suppress_tokens`` and ``min_new_tokens`` /
``min_length`` of HF 4.29.2's ``generate``, for every token-choice path of both engines.

:class:`TokenConstraints` are the arguments; :class:`DeviceConstraints` owns the per-slot state of ``ops.constrain_rows`` -- each
slot's token history (its own prompt, never the batch's padding, then what it generated), the word table, the processed-logits buffer
and the ban bitmap -- and turns a step's logits into the same logits with -inf at the banned tokens, in ONE launch per step and
without a transfer.  With no constraint asked for nothing of this is built and no launch is added.

Order: the ban is applied to the RAW logits, before the sampler's repetition penalty; HF applies the penalty first.  A -inf stays -inf
under the penalty (and under temperature, top-k, top-p) and the penalty of a token does not depend on the others, so ban-first gives
the same distribution.  Under beams HF applies its processors after the log-softmax: a banned token still counts in the normaliser and
is only left out of the selection, which is what ``ops.beam_topk_rows(ban=...)`` does with the bitmap.  ``min_length`` counts the
row's own length, without the batch's padding (the project's rule for padded batches; HF counts the padded width).
Log-probabilities (``return_logprobs``) stay those of the model's own distribution over the raw logits; with a constraint on, the
``rank`` of a greedy token may therefore be above 0.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch

from .. import ops


def _integer(name, v, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer in {lo} .. {hi if hi is not None else ''}, got {v!r}")
    return v


@dataclass(frozen=True)
class TokenConstraints:
    no_repeat_ngram_size: int = 0       # 0 (or None): off
    bad_words_ids: Tuple[Tuple[int, ...], ...] = ()
    suppress_tokens: Tuple[int, ...] = ()
    min_new_tokens: int = 0
    min_length: int = 0

    def __post_init__(self):
        def put(name, v):
            object.__setattr__(self, name, v)
        put("no_repeat_ngram_size", _integer("no_repeat_ngram_size", 0 if self.no_repeat_ngram_size is None else self.no_repeat_ngram_size,
                                             0, ops.CONSTRAIN_MAX_NGRAM))
        put("min_new_tokens", _integer("min_new_tokens", 0 if self.min_new_tokens is None else self.min_new_tokens, 0, 2 ** 31 - 1))
        put("min_length", _integer("min_length", 0 if self.min_length is None else self.min_length, 0, 2 ** 31 - 1))
        words = () if self.bad_words_ids is None else self.bad_words_ids
        if isinstance(words, (str, bytes)) or not isinstance(words, (list, tuple)):
            raise ValueError(f"bad_words_ids must be a list of non-empty lists of token ids, got {words!r}")
        out = []
        for w in words:
            if isinstance(w, (str, bytes)) or not isinstance(w, (list, tuple)) or len(w) == 0:
                raise ValueError(f"bad_words_ids must be a list of non-empty lists of token ids, got the word {w!r}")
            out.append(tuple(_integer("bad_words_ids: a token id", t, 0, 2 ** 31 - 1) for t in w))
        if len(out) > ops.CONSTRAIN_MAX_WORDS or sum(len(w) for w in out) > ops.CONSTRAIN_MAX_WORD_TOKENS:
            raise ValueError(f"bad_words_ids: {len(out)} words / {sum(len(w) for w in out)} tokens exceed the table's "
                             f"{ops.CONSTRAIN_MAX_WORDS} words / {ops.CONSTRAIN_MAX_WORD_TOKENS} tokens")
        put("bad_words_ids", tuple(out))
        sup = () if self.suppress_tokens is None else self.suppress_tokens
        if isinstance(sup, (str, bytes)) or not isinstance(sup, (list, tuple)):
            raise ValueError(f"suppress_tokens must be a list of token ids, got {sup!r}")
        put("suppress_tokens", tuple(_integer("suppress_tokens: a token id", t, 0, 2 ** 31 - 1) for t in sup))
        if len(self.bad_words_ids) + len(self.suppress_tokens) > ops.CONSTRAIN_MAX_WORDS:
            raise ValueError(f"bad_words_ids and suppress_tokens together exceed the table's {ops.CONSTRAIN_MAX_WORDS} words")

    @property
    def active(self) -> bool:
        """False when these parameters ban nothing, whatever the history."""
        return bool(self.no_repeat_ngram_size or self.bad_words_ids or self.suppress_tokens or self.min_new_tokens or self.min_length)

    def words(self, eos: Optional[int] = None) -> Tuple[Tuple[int, ...], ...]:
        """The word table: the bad words, then ``suppress_tokens`` as one-token words; a word equal to ``[eos]`` is dropped, as HF does."""
        table = self.bad_words_ids + tuple((t,) for t in self.suppress_tokens)
        return tuple(w for w in table if eos is None or eos < 0 or w != (eos,))


def constraints_from_generate(no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None, min_new_tokens=None,
                              min_length=None) -> Optional[TokenConstraints]:
    """The constraints of a ``generate`` call, or None when it asks for none (``None``, ``0``, empty).  Bad values raise either way."""
    c = TokenConstraints(no_repeat_ngram_size, bad_words_ids, suppress_tokens, min_new_tokens, min_length)
    return c if c.active else None


class DeviceConstraints:
    """``process(logits, ...)`` -> the rows with -inf at the banned tokens (or the ban bitmap, for beams), one ``ops.constrain_rows``
    launch that also brings the slots' histories up to date.

    ``admit(slots, prompts)`` before a slot's first token copies its prompt into its history row and sets both lengths;
    ``release(slots)`` when its example is done.  ``max_len``: the longest history a slot may reach, prompt + new tokens."""

    def __init__(self, params: TokenConstraints, n_slots: int, vocab: int, max_len: int, device, eos: Optional[int] = None):
        if n_slots < 1 or not 1 <= vocab <= ops.CONSTRAIN_MAX_VOCAB or max_len < 1:
            raise ValueError(f"DeviceConstraints: need n_slots >= 1, 1 <= vocab <= {ops.CONSTRAIN_MAX_VOCAB} and max_len >= 1, got "
                             f"{n_slots}, {vocab}, {max_len}")
        self.params, self.n_slots, self.vocab, self.max_len, self.device = params, n_slots, vocab, int(max_len), torch.device(device)
        self.eos = -1 if eos is None or eos < 0 else int(eos)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.hist = torch.zeros((n_slots, self.max_len), **i32)
        self.hist_len = torch.zeros((n_slots,), **i32)
        self.prompt_len = torch.zeros((n_slots,), **i32)
        words = params.words(self.eos)
        offs = [0]
        for w in words:
            offs.append(offs[-1] + len(w))
        self.bw_tokens = torch.tensor([t for w in words for t in w], **i32) if words else None
        self.bw_off = torch.tensor(offs, **i32) if words else None
        self.out = torch.zeros((n_slots, vocab), dtype=torch.float32, device=self.device)    # zeros: a skipped row stays a valid row
        self.ban = None                                            # beams only: built at the first process(bitmap=True)
        self.status = torch.zeros((1,), **i32)

    def _slots(self, slots: Sequence[int], what: str):
        slots = [int(b) for b in slots]
        if any(not 0 <= b < self.n_slots for b in slots) or len(set(slots)) != len(slots):
            raise ValueError(f"DeviceConstraints.{what}: bad slot list {slots}")
        return slots

    def admit(self, slots: Sequence[int], prompts: Sequence[torch.Tensor]) -> None:
        slots = self._slots(slots, "admit")
        if len(prompts) != len(slots):
            raise ValueError("DeviceConstraints.admit: slots and prompts differ in length")
        if not slots:
            return
        flat = [torch.as_tensor(p).detach().reshape(-1).to(device="cpu", dtype=torch.int32) for p in prompts]
        lens = [p.numel() for p in flat]
        if max(lens) > self.max_len:
            raise ValueError(f"DeviceConstraints.admit: a prompt of {max(lens)} tokens does not fit the history's {self.max_len}")
        rows = torch.zeros((len(slots), max(max(lens), 1)), dtype=torch.int32)
        for i, p in enumerate(flat):
            rows[i, : p.numel()] = p
        idx = torch.tensor(slots, dtype=torch.long, device=self.device)
        self.hist[idx, : rows.shape[1]] = rows.to(self.device)
        n = torch.tensor(lens, dtype=torch.int32, device=self.device)
        self.hist_len[idx] = n
        self.prompt_len[idx] = n

    def release(self, slots: Sequence[int]) -> None:
        slots = self._slots(slots, "release")
        idx = torch.tensor(slots, dtype=torch.long, device=self.device)
        self.hist_len[idx] = 0
        self.prompt_len[idx] = 0

    def process(self, logits: torch.Tensor, state: Optional[torch.Tensor] = None, slot_of_row=None, last: Optional[torch.Tensor] = None,
                parent: Optional[torch.Tensor] = None, bitmap: bool = False) -> torch.Tensor:
        """fp32 ``logits`` [rows, >= vocab] -> the rows with -inf at the banned tokens and the raw bits elsewhere (a buffer the next
        call overwrites; rows of slots that are not ROW_ACTIVE keep what it held), or with ``bitmap`` the ban bitmap int32 [n_slots,
        ceil(vocab / 32)] for ``ops.beam_topk_rows(ban=...)``.  ``last`` (int64 [n_slots]): the token each slot's logits were computed
        from, appended to its history first; None appends nothing -- the rows are prefill rows, whose history is the prompt that
        :meth:`admit` copied in.  ``parent`` (int32 [n_slots], any stride): beams, the slot whose history each slot continues."""
        if logits.dim() == 3 and logits.shape[1] == 1:
            logits = logits[:, 0]
        rows = logits.shape[0]
        sor = None
        if slot_of_row is not None:
            sor = torch.as_tensor(slot_of_row, dtype=torch.int32, device=self.device)
        if last is not None:
            last = last.reshape(-1).to(torch.int64).contiguous()
        p = self.params
        kw = dict(vocab=self.vocab, state=state, slot_of_row=sor, hist=self.hist, hist_len=self.hist_len, prompt_len=self.prompt_len,
                  parent=parent, last_token=last, no_repeat_ngram_size=p.no_repeat_ngram_size, bw_tokens=self.bw_tokens, bw_off=self.bw_off,
                  eos=self.eos, min_new_tokens=p.min_new_tokens, min_length=p.min_length, status=self.status, slots=self.n_slots)
        if bitmap:
            if self.ban is None:
                self.ban = torch.zeros((self.n_slots, (self.vocab + 31) // 32), dtype=torch.int32, device=self.device)
            ops.constrain_rows(logits, ban=self.ban, **kw)
            return self.ban
        out = self.out[:rows]
        ops.constrain_rows(logits, out=out, **kw)
        return out

    def check(self) -> None:
        """Raises when a history row was full (:meth:`full`): from then on the bans were computed from a history that lacks tokens."""
        if self.full():
            raise RuntimeError(f"DeviceConstraints: a slot's history outgrew its {self.max_len} positions; tokens were not appended")

    def full(self) -> bool:
        """Whether a history row ever was full, so that a token was not appended (``max_len`` too small); a device-to-host read."""
        return bool(int(self.status.item()) & ops.CONSTRAIN_STATUS_FULL)
