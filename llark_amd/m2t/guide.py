"""Guided choice on the device: generation restricted to a closed set of token sequences -- HF 4.29.2's ``prefix_allowed_tokens_fn`` /
``PrefixConstrainedLogitsProcessor`` with the set given as data -- for every token-choice path of both engines.

A *choice set* is a non-empty list of non-empty token-id sequences (the labels of a closed question, several surface forms per label
being several sequences).  A row that has generated ``g`` may choose ``x`` iff some sequence starts with ``g + [x]``; when ``g`` is a
whole sequence ``eos`` is allowed (and, if that sequence is a proper prefix of another, the other's next tokens too); after ``eos``
the row is finished by the existing EOS rule.  Everything else gets -inf, allowed columns keep their raw bits.  The host callback
itself cannot be used: it would need the row's ids on the host every step.  So :class:`ChoiceSets` are the arguments, turned into ONE
prefix tree for all sets of a call (CSR), and :class:`DeviceGuide` owns that table and the per-slot node that ``ops.guide_rows``
advances -- one launch per step, no transfer.  With no choice set given nothing of this is built and no launch is added.

Under beams a token that is not allowed still counts in the log-softmax and is only left out of the candidates (the bitmap route of
``ops.beam_topk_rows(ban=...)``, as for :mod:`.constraints`): guided beam search with at least as many beams as sequences returns the
sequence with the highest summed log-probability, the one ``score_continuations(...).sum()`` ranks first, after one prompt prefill.
Log-probabilities (``return_logprobs``) stay those of the model's own distribution over the raw logits, not renormalised inside the set.
"""
from __future__ import annotations

import json
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from .. import ops


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _listy(v) -> bool:
    return isinstance(v, (list, tuple)) and not isinstance(v, (str, bytes))


def _one_set(s, what: str) -> Tuple[Tuple[int, ...], ...]:
    if isinstance(s, torch.Tensor):
        s = s.tolist()
    if not _listy(s) or len(s) == 0:
        raise ValueError(f"{what}: a choice set must be a non-empty list of non-empty token-id sequences, got {s!r}")
    seqs = set()
    for q in s:
        if isinstance(q, torch.Tensor):
            q = q.reshape(-1).tolist()
        if not _listy(q) or len(q) == 0:
            raise ValueError(f"{what}: a choice set must be a non-empty list of non-empty token-id sequences, got the sequence {q!r}")
        for t in q:
            if not _is_int(t) or not 0 <= t <= 2 ** 31 - 1:
                raise ValueError(f"{what}: a token id must be an integer in 0 .. {2 ** 31 - 1}, got {t!r}")
        seqs.add(tuple(q))
    return tuple(sorted(seqs))                                    # duplicates collapse


@dataclass(frozen=True, init=False)
class ChoiceSets:
    """The choice sets of one call, validated and frozen: ``sets[i]`` is set i, its sequences sorted and without duplicates."""
    sets: Tuple[Tuple[Tuple[int, ...], ...], ...]

    def __init__(self, sets, what: str = "choice_sets"):
        if not _listy(sets) or len(sets) == 0:
            raise ValueError(f"{what} must be a non-empty list of choice sets, got {sets!r}")
        object.__setattr__(self, "sets", tuple(_one_set(s, what) for s in sets))

    def table(self, vocab: int):
        """The prefix tree of all sets in CSR form, CPU int32: ``(child_off [nodes + 1], child_tok [edges], child_node [edges], terminal
        [nodes], roots)`` -- ``roots[i]`` is the node a row of set i starts at; children ascend by token.  A token id outside
        [0, vocab) and a table above the kernel's caps are refused here."""
        for i, s in enumerate(self.sets):
            for q in s:
                bad = [t for t in q if t >= vocab]
                if bad:
                    raise ValueError(f"choice set {i}: token id {bad[0]} outside [0, vocab = {vocab})")
        kids: List[dict] = []                                     # node -> {token: node}
        term: List[int] = []
        roots = []
        for s in self.sets:
            roots.append(len(kids))
            kids.append({}), term.append(0)
            for q in s:
                n = roots[-1]
                for t in q:
                    if t not in kids[n]:
                        kids[n][t] = len(kids)
                        kids.append({}), term.append(0)
                    n = kids[n][t]
                term[n] = 1
        off, tok, node = [0], [], []
        for k in kids:
            for t in sorted(k):
                tok.append(t), node.append(k[t])
            off.append(len(tok))
        if len(kids) > ops.GUIDE_MAX_NODES or len(tok) > ops.GUIDE_MAX_EDGES:
            raise ValueError(f"choice sets: {len(kids)} nodes / {len(tok)} edges exceed the table's {ops.GUIDE_MAX_NODES} nodes / "
                             f"{ops.GUIDE_MAX_EDGES} edges")
        i32 = torch.int32
        return (torch.tensor(off, dtype=i32), torch.tensor(tok, dtype=i32), torch.tensor(node, dtype=i32), torch.tensor(term, dtype=i32),
                roots)


def require_eos(eos, name: str = "eos_token_id") -> int:
    """A choice set needs an eos: a leaf would otherwise allow nothing."""
    if eos is None or isinstance(eos, bool) or not isinstance(eos, int) or eos < 0:
        raise ValueError(f"a choice set needs {name} >= 0 (the token that ends a whole sequence), got {eos!r}")
    return int(eos)


def guide_from_generate(allowed_continuations, n_rows: int):
    """The ``allowed_continuations`` of a ``generate`` call over ``n_rows`` rows -> ``(ChoiceSets, set index or None per row)``, or
    ``(None, None)`` when the argument is None.  One set (a list of sequences) is for every row; a list of sets is one per row, None
    for an unconstrained row."""
    a = allowed_continuations
    if a is None:
        return None, None
    what = "allowed_continuations"
    if not _listy(a) or len(a) == 0:
        raise ValueError(f"{what} must be one choice set (a non-empty list of token-id sequences) or a list with one set or None per row, "
                         f"got {a!r}")

    def is_seq(q):
        if isinstance(q, torch.Tensor):
            return q.dim() <= 1
        return _listy(q) and (len(q) == 0 or not (_listy(q[0]) or isinstance(q[0], torch.Tensor)))
    if all(q is not None and is_seq(q) for q in a):              # one set for every row
        return ChoiceSets([a], what), [0] * n_rows
    if len(a) != n_rows:
        raise ValueError(f"{what}: a per-row list needs one choice set (or None) per row: {n_rows} rows, got {len(a)} entries")
    given = [s for s in a if s is not None]
    if not given:
        return None, None
    index, k = [], 0
    for s in a:
        index.append(None if s is None else k)
        k += s is not None
    return ChoiceSets(given, what), index


def choices_from_strings(tokenizer, strings: Sequence[str], lead: str = " ") -> List[List[int]]:
    """One choice set from label strings: each is tokenised as ``lead + s`` without special tokens (a label follows the prompt's last
    token after a space, by default).  Several surface forms of a label are just several strings."""
    if not _listy(strings) or len(strings) == 0 or not all(isinstance(s, str) and s for s in strings):
        raise ValueError(f"choices must be a non-empty list of non-empty strings, got {strings!r}")
    out = []
    for s in strings:
        ids = list(tokenizer(lead + s, add_special_tokens=False).input_ids)
        if not ids:
            raise ValueError(f"the choice {s!r} tokenises to nothing")
        out.append([int(t) for t in ids])
    return out


def choices_from_json(text: str) -> List[str]:
    """The content of a ``--choices-json`` file: a JSON list of non-empty strings, one set for every example."""
    try:
        v = json.loads(text)
    except ValueError as e:
        raise ValueError(f"--choices-json: not JSON ({e})") from e
    if not isinstance(v, list) or len(v) == 0 or not all(isinstance(s, str) and s for s in v):
        raise ValueError(f"--choices-json: a non-empty JSON list of non-empty strings is expected, got {v!r}")
    return v


class DeviceGuide:
    """``process(logits, ...)`` -> the rows with -inf at every token that is not allowed (or the bitmap of those tokens, for beams),
    one ``ops.guide_rows`` launch that also advances the slots' nodes.

    ``admit(slots, set_index)`` before a slot's first token puts it at the root of its set (None: unconstrained);
    ``release(slots)`` when its example is done.  A slot that was never admitted is unconstrained."""

    def __init__(self, sets: ChoiceSets, n_slots: int, vocab: int, device, eos: Optional[int], eos_name: str = "eos_token_id"):
        if n_slots < 1 or not 1 <= vocab <= ops.GUIDE_MAX_VOCAB:
            raise ValueError(f"DeviceGuide: need n_slots >= 1 and 1 <= vocab <= {ops.GUIDE_MAX_VOCAB}, got {n_slots}, {vocab}")
        self.eos = require_eos(eos, eos_name)
        if self.eos >= vocab:
            raise ValueError(f"DeviceGuide: {eos_name} = {self.eos} outside [0, vocab = {vocab})")
        self.sets, self.n_slots, self.vocab, self.device = sets, n_slots, vocab, torch.device(device)
        off, tok, node, term, self.roots = sets.table(vocab)
        self.child_off, self.child_tok, self.child_node, self.terminal = (t.to(self.device) for t in (off, tok, node, term))
        i32 = dict(dtype=torch.int32, device=self.device)
        self.node = torch.full((n_slots,), ops.GUIDE_FREE, **i32)             # read by the next launch
        self.node_next = torch.full((n_slots,), ops.GUIDE_FREE, **i32)        # written by it; then the two swap
        self.out = None                                            # the processed rows: built at the first process without bitmap
        self.n_open = torch.ones((n_slots,), **i32)
        self.ban = None                                            # beams without constraints: built at the first process(bitmap=True)
        self.status = torch.zeros((1,), **i32)

    def _slots(self, slots: Sequence[int], what: str):
        slots = [int(b) for b in slots]
        if any(not 0 <= b < self.n_slots for b in slots) or len(set(slots)) != len(slots):
            raise ValueError(f"DeviceGuide.{what}: bad slot list {slots}")
        return slots

    def _put(self, slots, values) -> None:
        if slots:
            idx = torch.tensor(slots, dtype=torch.long, device=self.device)
            v = torch.tensor(values, dtype=torch.int32, device=self.device)
            self.node[idx] = v
            self.node_next[idx] = v

    def admit(self, slots: Sequence[int], set_index: Sequence[Optional[int]]) -> None:
        slots = self._slots(slots, "admit")
        set_index = list(set_index)
        if len(set_index) != len(slots):
            raise ValueError("DeviceGuide.admit: slots and set_index differ in length")
        for i in set_index:
            if i is not None and (isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < len(self.roots)):
                raise ValueError(f"DeviceGuide.admit: a set index must be None or an integer in 0 .. {len(self.roots) - 1}, got {i!r}")
        self._put(slots, [ops.GUIDE_FREE if i is None else self.roots[i] for i in set_index])

    def release(self, slots: Sequence[int]) -> None:
        slots = self._slots(slots, "release")
        self._put(slots, [ops.GUIDE_FREE] * len(slots))

    def process(self, logits: torch.Tensor, state: Optional[torch.Tensor] = None, slot_of_row=None, last: Optional[torch.Tensor] = None,
                parent: Optional[torch.Tensor] = None, bitmap: bool = False, ban: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 ``logits`` [rows, >= vocab] -> the rows with -inf at the tokens that are not allowed and the raw bits elsewhere (a buffer
        the next call overwrites; rows of slots that are not ROW_ACTIVE keep what it held), or with ``bitmap`` the bitmap int32
        [n_slots, ceil(vocab / 32)] of those tokens for ``ops.beam_topk_rows(ban=...)`` -- OR-ed into ``ban`` when one is given (the
        bitmap :class:`DeviceConstraints` just wrote), else stored into an own one.  ``last`` (int64 [n_slots]): the token each slot's
        logits were computed from, by which its node steps first; None: prefill rows, whose node is where :meth:`admit` put it.
        ``parent`` (int32 [n_slots], any stride): beams, the slot whose node each slot continues from.  The buffer the launch writes
        starts as a copy of the one it reads, so a slot that the launch skips (not among its rows, or not ROW_ACTIVE) keeps its node."""
        if logits.dim() == 3 and logits.shape[1] == 1:
            logits = logits[:, 0]
        rows = logits.shape[0]
        sor = None
        if slot_of_row is not None:
            sor = torch.as_tensor(slot_of_row, dtype=torch.int32, device=self.device)
        if last is not None:
            last = last.reshape(-1).to(torch.int64).contiguous()
        self.node_next.copy_(self.node)                           # a slot the launch skips (not in it, not active) keeps its node through the swap
        kw = dict(eos=self.eos, vocab=self.vocab, state=state, slot_of_row=sor, parent=parent, last_token=last, status=self.status)
        tab = (self.child_off, self.child_tok, self.child_node, self.terminal, self.node, self.node_next)
        if bitmap:
            if ban is None:
                if self.ban is None:
                    self.ban = torch.zeros((self.n_slots, (self.vocab + 31) // 32), dtype=torch.int32, device=self.device)
                ops.guide_rows(logits, *tab, ban=self.ban, **kw)
                res = self.ban
            else:
                ops.guide_rows(logits, *tab, ban=ban, ban_accumulate=True, **kw)
                res = ban
        else:
            if self.out is None:                                   # zeros: a skipped row stays a valid row
                self.out = torch.zeros((self.n_slots, self.vocab), dtype=torch.float32, device=self.device)
            res = self.out[:rows]
            ops.guide_rows(logits, *tab, out=res, n_open=self.n_open[:rows], **kw)
        self.node, self.node_next = self.node_next, self.node
        return res

    def check(self, off_set: bool = True) -> None:
        """Raises when a row had no allowed token left with a finite logit (other constraints banned them all: nothing valid could be
        chosen), or when a slot was handed a token outside its set; a device-to-host read.  ``off_set=False`` (beams): a slot that
        holds no beam is fed the pad token, which is no fault."""
        st = int(self.status.item())
        if st & ops.GUIDE_STATUS_EMPTY:
            raise RuntimeError("DeviceGuide: a row had no allowed token left (every continuation inside its choice set was banned)")
        if off_set and st & ops.GUIDE_STATUS_OFF_SET:
            raise RuntimeError("DeviceGuide: a slot was handed a token outside its choice set")
