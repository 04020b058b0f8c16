"""Batched inference drivers.

The reference's ``scripts/inference/infer_from_encodings.py:47-116`` walks a directory of ``<id>.npy`` Jukebox
representations (the files ``jukebox/main.py:254`` writes: float32, C-order, ``(frames, 4800)``) ONE example at a time
through ``infer_with_prompt`` and writes a CSV with the columns ``example_id, prompt_text, model_completion_text``.
Here the same contract is served in batches on the HIP engine:

* :func:`infer_from_encodings` -- same inputs / same CSV, ``batch_size`` examples per ``generate`` call;
* :func:`infer_from_audio`     -- audio clips -> ``WrappedAudioEncoder`` -> LLM in ONE process: the ``(B, frames, 4800)``
  embeddings never leave HBM (no ``.npy`` round trip);
* :func:`infer_from_shards`    -- the contract of ``scripts/inference/infer_from_webdataset.py:51-151`` (local tar shards, one
  example per question, per-example prompts) through :func:`generate_inflight`: ragged prompts share the engine's batch slots
  and a finished row's slot is refilled with the next example while the other slots keep decoding.

Batched greedy decoding is token-for-token the per-example loop of the reference: every kernel on the path is
row-independent and accumulates each output element in the same k order whatever the batch size, and stopping is
tracked per sequence (``KeywordsStoppingCriteria`` semantics of ``m2t/generate.py:31-44`` applied row by row).
"""
from __future__ import annotations

import glob
import os
import random
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .generate import KeywordsStoppingCriteria
from .prompting import (DEFAULT_CONVERSATION_HEADER, concat_audio_token_and_prompt, extract_prompt_tokens,
                        extract_response_tokens, preprocess_for_lm_mappable, preprocess_multimodal_mappable)

EMBED_DIM = 4800


def load_encoding(path: str, embed_dim: int = EMBED_DIM) -> np.ndarray:
    """One ``.npy`` representation under the contract of ``jukebox/main.py:254`` / ``m2t/gcs_utils.py:175-248``:
    float32, C-order, ``(frames, embed_dim)`` (or ``(embed_dim,)`` for the frame-rate-0 pooling -> one frame)."""
    a = np.load(path, allow_pickle=False)
    if a.dtype != np.float32:
        raise ValueError(f"{path}: expected float32 encodings, got {a.dtype}")
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != embed_dim:
        raise ValueError(f"{path}: expected shape (frames, {embed_dim}), got {a.shape}")
    return np.ascontiguousarray(a)


def build_prompt_ids(prompt: str, frames: int, tokenizer, multimodal_cfg: Dict[str, Any], end_seq: Sequence[int],
                     audio_first: bool = True, header: str = DEFAULT_CONVERSATION_HEADER) -> torch.Tensor:
    """Token ids of header + human turn (with the audio placeholder expanded to ``frames`` patches) up to and including
    "### Assistant:" -- exactly what ``infer_with_prompt`` (m2t/infer.py:99-145) feeds to ``generate``."""
    text = concat_audio_token_and_prompt(prompt, audio_first)
    elem = {"audio_encoding": np.zeros((frames, 1), dtype=np.float32), "audio_encoding_shape": [frames, 1], "id": None,
            "conversations": [{"from": "human", "value": text}, {"from": "gpt", "value": "<empty>"}]}
    elem = preprocess_for_lm_mappable(preprocess_multimodal_mappable(elem, multimodal_cfg), tokenizer=tokenizer, header=header)
    return extract_prompt_tokens(elem["input_ids"], end_seq)


@torch.no_grad()
def generate_batch(model, input_ids: torch.Tensor, encodings: torch.Tensor, tokenizer, max_new_tokens: int = 512,
                   keywords: Sequence[str] = ("###",), **generate_kwargs) -> List[torch.Tensor]:
    """Greedy generation for B examples sharing one prompt length.  Returns, per example, prompt + continuation ids cut
    where the reference's loop would have stopped for that example (keyword hit, EOS, or ``max_new_tokens``).  ``generate_kwargs``
    (``no_repeat_ngram_size``, ``min_new_tokens``, ...) go to ``model.generate``.  EOS is handled per row here and ``generate`` runs
    without one -- except under ``min_new_tokens`` / ``min_length``, which ban the EOS and so need ``generate`` to know it: a row that
    ended then emits padding behind its cut, nothing else changes."""
    B = input_ids.shape[0]
    dev = model.engine.device if getattr(model, "_engine", None) is not None else torch.device("cuda")
    ids = input_ids.to(dev)
    stops = [KeywordsStoppingCriteria(keywords=list(keywords), tokenizer=tokenizer, input_ids=input_ids[b: b + 1]) for b in range(B)]
    eos = getattr(getattr(model, "generation_config", None), "eos_token_id", None)
    done_at: List[Optional[int]] = [None] * B
    needs_eos = eos is not None and bool(generate_kwargs.get("min_new_tokens") or generate_kwargs.get("min_length"))

    class _AllDone:                                        # plugs the per-row bookkeeping into model.generate's loop
        def __call__(self, out_ids, scores=None, **kw):
            n = out_ids.shape[1]
            rows = out_ids.cpu()
            for b in range(B):
                if done_at[b] is None and (stops[b](rows[b: b + 1], None) or (eos is not None and int(rows[b, -1]) == eos)):
                    done_at[b] = n
            return all(d is not None for d in done_at)

    out = model.generate(input_ids=ids, audio_encodings=encodings, max_new_tokens=max_new_tokens, stopping_criteria=[_AllDone()],
                         eos_token_id=eos if needs_eos else -1, **generate_kwargs)     # EOS is handled per row above
    out = out.cpu()
    return [out[b, : (done_at[b] if done_at[b] is not None else out.shape[1])] for b in range(B)]


@torch.no_grad()
def generate_beam(model, input_ids: torch.Tensor, encodings: torch.Tensor, tokenizer, max_new_tokens: int = 512, num_beams: int = 4,
                  length_penalty: float = 1.0, keywords: Sequence[str] = ("###",), **generate_kwargs) -> List[torch.Tensor]:
    """Beam search, one example per ``model.generate(num_beams=...)`` call under the keyword stopping criterion (HF's criterion sees
    the best live beam first, as the reference's loop would).  Returns, per example, prompt + the best hypothesis' ids: the eos that
    generate puts behind a short row, and the padding, are cut.  ``generate_kwargs`` (``no_repeat_ngram_size``, ``min_new_tokens``, ...) go to
    ``model.generate``."""
    eos = getattr(getattr(model, "generation_config", None), "eos_token_id", None)
    S, outs = input_ids.shape[1], []
    for b in range(input_ids.shape[0]):
        stop = KeywordsStoppingCriteria(keywords=list(keywords), tokenizer=tokenizer, input_ids=input_ids[b: b + 1])
        row = model.generate(input_ids=input_ids[b: b + 1], audio_encodings=encodings[b: b + 1], max_new_tokens=max_new_tokens,
                             stopping_criteria=[stop], num_beams=num_beams, length_penalty=length_penalty, **generate_kwargs)[0].cpu()
        hit = (row[S:] == eos).nonzero() if eos is not None and eos >= 0 else torch.empty((0, 1))
        outs.append(row[: S + int(hit[0])] if hit.numel() else row)
    return outs


def refuse_beams(where: str, num_beams) -> None:
    """Beam search runs through WrappedLlamav2ForCausalLM.generate only: everywhere else the argument is refused, not ignored."""
    if num_beams is not None and num_beams != 1:
        raise NotImplementedError(f"{where}: num_beams={num_beams!r} is not implemented here (beam search: WrappedLlamav2ForCausalLM.generate)")


MIN_SHARED = 64      # fewest common leading tokens worth a fork; the engine's own (untuned) default, HipLlamaEngine.MIN_SHARED


class InflightScheduler:
    """Slot table of :func:`generate_inflight`, free of any GPU code so that it can run against a fake backend.

    ``backend`` is the narrow model interface:
      * ``prefill(slots, prompts, encodings) -> first tokens``: new examples (1-D int64 prompt ids, encoding or None) into the
        given slots; returns the greedy token after each prompt, in the order of ``slots``;
      * ``decode() -> tokens``: one decode step of every slot; returns a token per slot (entries of free slots are ignored);
      * ``release(slots)``: the slots' examples are done.
    Free slots are refilled in ascending slot order with examples in input order; a row stops on a keyword (``stop_fn``), on
    ``eos`` or at its budget, exactly as :func:`generate_batch` decides per row.  ``trace`` records ``("prefill", slots, indices)``
    and ``("done", slot, index)`` events.

    ``share_prefix``: an example may carry a ``prefix_key`` (equal keys promise equal audio encodings: the questions of one clip).
    When one is admitted while a slot of the same key is active -- or is being prefilled in the same round -- and the two prompts
    have at least ``min_shared`` leading tokens in common (capped at the new prompt's length - 1, the rest free of the backend's
    ``audio_token_ids``), the backend copies those positions (``fork(src, dsts, n)``) and prefills only the rest
    (``prefill(slots, suffixes, [None, ...], past=[n, ...])``); the trace gains ``("fork", src, dst, n)``.  The examples that need a full
    prefill go first, in one call as ever; a backend without ``fork`` gets nothing but full prefills.  Off (the default), calls and
    trace are exactly what they were.

    ``sampling``: the backend draws its tokens (:class:`llark_amd.m2t.sampling.DeviceSampler`) and every ``prefill`` call also gets
    ``indices=`` (the examples' input indices: their random streams) and ``whole=`` (their full prompts -- what a forked slot has seen
    although only its suffix is prefilled).  Off (the default), the backend's signature is what it was.

    ``logprobs``: the backend records the log-probability of every token it hands out -- log-softmax of the model's raw logits; no
    repetition penalty, temperature, top-k or top-p is applied, for sampled tokens too -- and ``run`` yields ``(index, ids, logprobs)``
    with one entry per generated token, the EOS or keyword token included.  ``backend.take_logprobs(finished)`` (a list of 1-D
    tensors in the order of ``finished``) is called just before ``backend.release(finished)``.  Off (the default), the backend sees
    no new call and ``run`` yields pairs.

    ``choices``: an example may carry a fifth element, the index of its choice set (None: unconstrained), and every ``prefill`` call
    also gets ``choice=`` (the indices of its examples).  Off (the default), a fifth element is refused."""

    def __init__(self, backend, n_slots: int, max_new_tokens: int = 512, eos: Optional[int] = None, stop_fn=None,
                 share_prefix: bool = False, min_shared: int = MIN_SHARED, sampling: bool = False, logprobs: bool = False,
                 choices: bool = False):
        if n_slots < 1:
            raise ValueError(f"n_slots must be >= 1, got {n_slots}")
        self.backend, self.n_slots, self.max_new_tokens = backend, n_slots, max_new_tokens
        self.share_prefix = bool(share_prefix) and hasattr(backend, "fork")
        self.min_shared = min_shared
        self.sampling = bool(sampling)
        self.logprobs = bool(logprobs)
        self.choices = bool(choices)
        self.eos = eos if eos is not None and eos >= 0 else None
        self.stop_fn = stop_fn                    # (prompt ids, generated ids) -> bool: keyword stop; may keep state per row
        self.trace: List[Tuple] = []

    def run(self, examples: Iterable[Sequence[Any]]) -> Iterator[Tuple[int, torch.Tensor]]:
        """examples: (prompt_ids, encoding[, max_new_tokens[, prefix_key[, choice set index]]]).  Yields (input index, prompt + generated ids) as rows finish; rows
        finishing in the same step come out in input order.  With ``logprobs``: (input index, ids, log-probabilities of the generated
        tokens under the model's raw logits)."""
        it = enumerate(examples)
        exhausted = False
        table: List[Optional[Dict[str, Any]]] = [None] * self.n_slots
        while True:
            free = [b for b in range(self.n_slots) if table[b] is None]
            new: List[int] = []
            while free and not exhausted:
                try:
                    idx, ex = next(it)
                except StopIteration:
                    exhausted = True
                    break
                prompt = torch.as_tensor(ex[0], dtype=torch.int64).reshape(-1).cpu()
                budget = int(ex[2]) if len(ex) > 2 and ex[2] is not None else self.max_new_tokens
                if len(ex) > 4 and ex[4] is not None and not self.choices:
                    raise ValueError(f"example {idx} names the choice set {ex[4]!r}, but no choice_sets were given")
                b = free.pop(0)
                table[b] = {"index": idx, "prompt": prompt, "enc": ex[1], "budget": budget, "out": [], "stop": None,
                            "key": ex[3] if len(ex) > 3 else None, "choice": ex[4] if len(ex) > 4 else None}
                new.append(b)
            if new:
                done = self._take(table, self._admit(table, new))
                yield from done
                if done and not exhausted:
                    continue                       # refill the slots that finished at once before the next decode step
            if all(r is None for r in table):
                if exhausted:
                    return
                continue
            toks = self.backend.decode()
            yield from self._take(table, {b: toks[b] for b in range(self.n_slots) if table[b] is not None})

    def _admit(self, table, new: List[int]) -> Dict[int, int]:
        """Prefill the examples just placed in the slots ``new``; returns slot -> first token."""
        forks = self._plan_forks(table, new) if self.share_prefix else {}
        full = [b for b in new if b not in forks]
        toks: Dict[int, int] = {}

        def extra(slots):
            kw = dict(indices=[table[b]["index"] for b in slots], whole=[table[b]["prompt"] for b in slots]) if self.sampling else {}
            if self.choices:
                kw["choice"] = [table[b]["choice"] for b in slots]
            return kw
        if full:
            self.trace.append(("prefill", tuple(full), tuple(table[b]["index"] for b in full)))
            toks.update(zip(full, self.backend.prefill(full, [table[b]["prompt"] for b in full], [table[b]["enc"] for b in full],
                                                       **extra(full))))
        if forks:
            calls: Dict[Tuple[int, int], List[int]] = {}
            for b in sorted(forks):
                calls.setdefault(forks[b], []).append(b)
            for (src, n), dsts in calls.items():
                for b in dsts:
                    self.trace.append(("fork", src, b, n))
                self.backend.fork(src, dsts, n)
            forked = sorted(forks)
            self.trace.append(("prefill", tuple(forked), tuple(table[b]["index"] for b in forked)))
            firsts = self.backend.prefill(forked, [table[b]["prompt"][forks[b][1]:] for b in forked], [None] * len(forked),
                                          past=[forks[b][1] for b in forked], **extra(forked))
            toks.update(zip(forked, firsts))
        return toks

    def _plan_forks(self, table, new: List[int]) -> Dict[int, Tuple[int, int]]:
        """slot -> (source slot, n) for the new examples that start like a slot of their key which is active, or which gets its
        full prefill in this round (the first of several new siblings).  The longest common prefix wins, then the lowest slot."""
        audio = set(getattr(self.backend, "audio_token_ids", ()))
        forks: Dict[int, Tuple[int, int]] = {}
        sources = [b for b in range(self.n_slots) if table[b] is not None and b not in new]
        for b in new:
            row = table[b]
            best = None
            for src in sources if row["key"] is not None else ():
                if table[src]["key"] != row["key"]:
                    continue
                a, p = table[src]["prompt"], row["prompt"]
                m = min(a.numel(), p.numel())
                diff = (a[:m] != p[:m]).nonzero()
                n = min(int(diff[0]) if diff.numel() else m, p.numel() - 1)
                if n >= self.min_shared and not any(int(t) in audio for t in p[n:]) and (best is None or n > best[1]):
                    best = (src, n)
            if best is not None:
                forks[b] = best
            else:
                sources.append(b)                     # prefilled in full first: later siblings of this round fork from it
        return forks

    def _take(self, table, toks: Dict[int, int]) -> List[Tuple[int, torch.Tensor]]:
        finished = []
        for b in sorted(toks):
            row = table[b]
            t = int(toks[b])
            row["out"].append(t)
            if (len(row["out"]) >= row["budget"] or (self.eos is not None and t == self.eos)
                    or (self.stop_fn is not None and self.stop_fn(row, torch.tensor(row["out"], dtype=torch.int64)))):
                finished.append(b)
        if not finished:
            return []
        lps = self.backend.take_logprobs(finished) if self.logprobs else None
        self.backend.release(finished)
        outs = []
        for i, b in enumerate(finished):
            row = table[b]
            table[b] = None
            self.trace.append(("done", b, row["index"]))
            ids = torch.cat((row["prompt"], torch.tensor(row["out"], dtype=torch.int64)))
            if lps is None:
                outs.append((row["index"], ids))
            else:
                lp = torch.as_tensor(lps[i], dtype=torch.float32).reshape(-1)
                if lp.numel() != len(row["out"]):
                    raise RuntimeError(f"slot {b}: {lp.numel()} log-probabilities for {len(row['out'])} generated tokens")
                outs.append((row["index"], ids, lp))
        return sorted(outs, key=lambda o: o[0])


class EngineSlots:
    """:class:`InflightScheduler` backend on the HIP engine's ragged slot mode (``init_slots`` / ``prefill_slots`` / ``decode_slots`` /
    ``release_slots`` of ``HipLlamaEngine`` or ``HipMptEngine``) of a ``WrappedLlamav2ForCausalLM`` or ``WrappedMPTForCausalLM``.  The
    MPT wrapper splices audio by its patch tokens (``audio_patch_branch``) and its engine has no shared-prefix form (``init_slots``
    raises ``NotImplementedError``).  ``sampling`` (a :class:`llark_amd.m2t.sampling.SamplingParams`): tokens come from the device
    sampler, whose stream id is the example's input index.  ``logprobs``: every token handed out -- the first one from the refill's
    prefill logits, the others from the decode step's -- gets its log-probability under the model's raw logits (log-softmax; no
    repetition penalty, temperature, top-k or top-p, for sampled tokens too) appended to its slot's history on the device
    (:class:`llark_amd.m2t.logprob.LogprobTracker`, one launch per step); ``take_logprobs(slots)`` reads finished slots' histories.
    ``constraints`` (a :class:`llark_amd.m2t.constraints.TokenConstraints`): every choice, greedy or sampled, is made on the logits with
    -inf at the tokens its example's history bans (one more launch per step, no transfer); the EOS of ``min_new_tokens`` /
    ``min_length`` is the model's ``generation_config.eos_token_id``.  ``choice_sets`` (a :class:`llark_amd.m2t.guide.ChoiceSets`):
    an example that names one of the sets only continues inside it (one more launch per step, no transfer); the EOS a whole sequence
    allows is the same ``eos_token_id``, which must exist.  The stages that are on run in the order of one
    :class:`llark_amd.m2t.choice.TokenChooser`."""

    def __init__(self, model, n_slots: int, share_prefix: bool = False, sampling=None, logprobs: bool = False, constraints=None,
                 choice_sets=None):
        from .llamav2 import plan_audio_splice

        self._plan = plan_audio_splice
        self._plan_kw = dict(patch_branch=True) if getattr(model, "audio_patch_branch", False) else {}
        self.model = model
        self.eng = model.engine
        if share_prefix:
            self.eng.init_slots(n_slots, share_prefix=True)
        else:
            self.eng.init_slots(n_slots)
        self.n_slots = n_slots
        self.ids = torch.zeros((n_slots,), dtype=torch.int64, device=self.eng.device)
        stages = dict(sampling=sampling if sampling is not None and sampling.active else None,
                      constraints=constraints if constraints is not None and constraints.active else None, logprobs=bool(logprobs))
        if choice_sets is not None:
            from .guide import require_eos

            require_eos(getattr(getattr(model, "generation_config", None), "eos_token_id", None), "generation_config.eos_token_id")
            stages["guide"] = choice_sets
        self.stages = stages if any(stages.values()) else None    # None: plain greedy calls, nothing launched or allocated
        self.chooser = None                                       # built at the first prefill, which tells the logits' width
        self.index_of_slot = {}                                   # slot -> its example's input index (when the scheduler hands them on)
        cfg = model.get_model().audio_encoder_config
        self.audio_token_ids = tuple(int(t) for t in (getattr(cfg, name, None) for name in ("audio_start_token", "audio_end_token", "audio_patch_token"))
                                     if t is not None)

    def fork(self, src, dsts, n):
        self.eng.fork_slots(src, dsts, n)

    def prefill(self, slots, prompts, encodings, past=None, indices=None, whole=None, choice=None):
        eng = self.eng
        cfg = self.model.get_model().audio_encoder_config
        segs = []
        for i, (p, enc) in enumerate(zip(prompts, encodings)):
            if enc is not None:
                feats = torch.as_tensor(enc).to(device=eng.device, dtype=torch.float32)
                segs += [(i, start, f) for (_, start, f) in self._plan(p[None], [feats], cfg, False, **self._plan_kw)]
        if past is None:
            logits = eng.prefill_slots([p.to(eng.device) for p in prompts], segs, slots)
        else:
            logits = eng.prefill_slots([p.to(eng.device) for p in prompts], segs, slots, past=past)
        if self.stages is None:
            first = logits.argmax(-1)                              # what generate() picks after the prompt
        else:
            if self.chooser is None:
                from .choice import TokenChooser

                # a history is at most the cache's smax positions plus the token just chosen: the engine refuses a slot beyond smax first
                self.chooser = TokenChooser(self.n_slots, logits.shape[-1], eng.device, history_len=eng.smax + 1, logprob_width=eng.smax,
                                            eos=getattr(getattr(self.model, "generation_config", None), "eos_token_id", None), **self.stages)
            self.chooser.admit(slots, prompts if whole is None else whole, indices, **({} if choice is None else dict(choice=choice)))
            if indices is not None:
                self.index_of_slot.update(zip(slots, indices))
            first = self.chooser(logits, state=eng.slot_state, slot_of_row=list(slots))
        self.ids[torch.tensor(slots, dtype=torch.long, device=eng.device)] = first
        return first.cpu().tolist()

    def decode(self):
        if self.chooser is not None:
            self.ids, host, _ = self.eng.decode_slots(self.ids, sample=lambda lg: self.chooser(lg, state=self.eng.slot_state))
        else:
            self.ids, host, _ = self.eng.decode_slots(self.ids)
        return host.tolist()

    def take_logprobs(self, slots):
        if self.stages is None or not self.stages["logprobs"]:
            raise RuntimeError("EngineSlots: built without logprobs=True")
        return self.chooser.take_logprobs(slots)

    def release(self, slots):
        self.check_guide(slots)
        self.eng.release_slots(slots)
        if self.chooser is not None:
            self.chooser.release(slots)

    def check_guide(self, slots=()):
        """Raises when a guided row had no allowed token left (every continuation inside its choice set was banned by the constraints)
        or was handed a token outside its set: the guide's status word, read when examples are released -- before their completions
        are handed out, so the example it happened to is never yielded -- and once more at the end of the run."""
        if self.chooser is None or self.chooser.guide is None:
            return
        from .. import ops

        try:
            self.chooser.guide.check()
        except RuntimeError as e:
            now = [self.index_of_slot.get(b, f"slot {b}") for b in slots]
            live = [i for b, i in sorted(self.index_of_slot.items()) if self.eng.slot_state_host[b] == ops.ROW_ACTIVE and b not in slots]
            raise RuntimeError(f"generate_inflight: {e}; noticed at the release of example(s) {now}, examples still decoding: {live}") from e


@torch.no_grad()
def generate_inflight(model, examples: Iterable[Sequence[Any]], slots: int = 8, max_new_tokens: int = 512,
                      keywords: Sequence[str] = ("###",), tokenizer=None, trace: Optional[list] = None,
                      share_prefix: bool = False, sampling=None, return_logprobs: bool = False,
                      num_beams: Optional[int] = None, constraints=None, choice_sets=None) -> Iterator[Tuple[int, torch.Tensor]]:
    """Generation (greedy unless ``sampling``) with in-flight slot refill.  ``examples`` yields ``(prompt_ids, encoding[, max_new_tokens[, prefix_key[, choice]]])`` with prompts
    of any length; up to ``slots`` of them decode together, each at its own KV-cache length, and a finished row's slot is refilled
    from the iterable (contiguous free slots prefilled as one batch) while the others keep decoding.  Stops per row as in
    :func:`generate_batch` (keyword -- needs ``tokenizer`` --, EOS or budget).  Yields ``(index, prompt + continuation ids)`` as
    examples complete.  ``model`` may provide ``slot_backend(n_slots)`` (any :class:`InflightScheduler` backend); otherwise its
    engine's ragged slot mode serves it.  ``trace``: a list that receives the scheduler's events.  ``share_prefix``: examples with
    equal ``prefix_key`` (the questions of one clip) share the K/V of their common leading tokens -- prefilled once, copied to the
    siblings' slots, and read once per group by the decode step (:class:`InflightScheduler`, ``HipLlamaEngine.fork_slots``).
    ``sampling``: a :class:`llark_amd.m2t.sampling.SamplingParams`; tokens are then chosen by the device sampler with the example's
    index as its random stream, so a completion depends neither on the slot the example landed in nor on ``slots`` (a model's own
    ``slot_backend`` is greedy: sampling with one is refused).  ``return_logprobs``: yields ``(index, ids, logprobs)`` instead;
    ``logprobs`` (1-D fp32, CPU) has one entry per generated token, ``ids.numel() - prompt.numel()`` of them, the EOS or keyword token
    included.  They are log-probabilities of the MODEL's distribution: log-softmax of the raw logits, computed on the device in the
    step's own launch sequence (``llark_token_logprob_rows``); repetition penalty, temperature, top-k and top-p are not applied, for
    sampled tokens too.  Refused with a model's own ``slot_backend`` as sampling is.  ``constraints``: a
    :class:`llark_amd.m2t.constraints.TokenConstraints` (``no_repeat_ngram_size``, ``bad_words_ids``, ``suppress_tokens``,
    ``min_new_tokens``, ``min_length``), applied on the device to every choice from the example's own history -- its whole prompt under
    ``share_prefix`` too -- so a completion does not depend on ``slots``; an example's own ``max_new_tokens`` below ``min_new_tokens``
    wins: the row stops at its budget.  Refused with a model's own ``slot_backend`` as sampling is.  ``choice_sets``: a list of choice
    sets (each a non-empty list of non-empty token-id sequences; :mod:`llark_amd.m2t.guide`); an example's fifth element is the index
    of its set, or None for an unconstrained example.  A guided example's new tokens are one of its set's sequences followed by the
    model's ``generation_config.eos_token_id`` (required), whatever ``slots`` is -- unless a keyword or its budget stops it first.  When
    ``constraints`` ban every continuation of a guided example the run raises a RuntimeError at the next release of examples, before
    that example is yielded (``EngineSlots.check_guide``).
    Refused with a model's own ``slot_backend`` as sampling is."""
    refuse_beams("generate_inflight", num_beams)
    if keywords and tokenizer is None:
        raise ValueError("generate_inflight: keyword stopping needs the tokenizer")
    make = getattr(model, "slot_backend", None)
    sampling = sampling if sampling is not None and sampling.active else None
    if sampling is not None and make is not None:
        raise ValueError("generate_inflight: sampling needs the engine's own slot backend; this model provides slot_backend()")
    if return_logprobs and make is not None:
        raise ValueError("generate_inflight: return_logprobs needs the engine's own slot backend; this model provides slot_backend()")
    constraints = constraints if constraints is not None and constraints.active else None
    if constraints is not None and make is not None:
        raise ValueError("generate_inflight: constraints need the engine's own slot backend; this model provides slot_backend()")
    more = {} if constraints is None else dict(constraints=constraints)
    if choice_sets is not None:
        from .guide import ChoiceSets

        if make is not None:
            raise ValueError("generate_inflight: choice_sets need the engine's own slot backend; this model provides slot_backend()")
        more["choice_sets"] = choice_sets if isinstance(choice_sets, ChoiceSets) else ChoiceSets(choice_sets)
    if make is not None:
        backend = make(slots)
    elif return_logprobs:
        backend = EngineSlots(model, slots, share_prefix, sampling, logprobs=True, **more)
    else:
        backend = EngineSlots(model, slots, share_prefix, sampling, **more)
    eos = getattr(getattr(model, "generation_config", None), "eos_token_id", None)
    stop_fn = None
    if keywords:
        def stop_fn(row, gen):
            if row["stop"] is None:
                row["stop"] = KeywordsStoppingCriteria(keywords=list(keywords), tokenizer=tokenizer, input_ids=row["prompt"][None])
            return bool(row["stop"](torch.cat((row["prompt"], gen))[None], None))
    sched = InflightScheduler(backend, slots, max_new_tokens, eos, stop_fn, share_prefix=share_prefix,
                              sampling=sampling is not None or constraints is not None or choice_sets is not None,
                              **(dict(logprobs=True) if return_logprobs else {}), **(dict(choices=True) if choice_sets is not None else {}))
    if trace is not None:
        sched.trace = trace
    yield from sched.run(examples)
    if choice_sets is not None:
        backend.check_guide()


@torch.no_grad()
def score_continuations(model, prompt_ids, encoding, continuations: Sequence[Any], logits_sink: Optional[list] = None) -> List[torch.Tensor]:
    """Teacher-forced scoring of candidate answers after one prompt: per candidate (a 1-D sequence of token ids, not empty), the
    log-probability of each of its tokens given the prompt (with ``encoding`` spliced in, or None) and the candidate's earlier
    tokens -- a 1-D fp32 CPU tensor of the candidate's length; its ``sum()`` ranks the candidates of a closed answer set
    (giantsteps key / tempo, gtzan genre), its ``mean()`` is the length-normalised score.

    They are log-probabilities of the MODEL's distribution: log-softmax of the raw logits; no repetition penalty, temperature, top-k
    or top-p exists on this path.  Each candidate is one row ``prompt + continuation`` through ``engine.forward_tokens`` with full
    logits; then ONE ``ops.token_logprob_rows`` launch over all B * S rows of the call, whose ``tokens`` are the ids shifted by one and
    -1 everywhere outside a candidate's own span (its first scored row is the prompt's last position), so prompt rows and pad rows are
    skipped.  Llama runs the candidates as right-padded batches of up to the engine's ``max_batch`` (causal attention never lets a
    valid position see a pad); MPT's forward takes no padded batch, so candidates of equal length share a batch and the rest run
    singly.  ``logits_sink``: a list that receives ``(logits [B * S, V], tokens [B * S])`` of every call (device tensors)."""
    from .. import ops
    from .llamav2 import plan_audio_splice

    eng = model.engine
    dev = eng.device
    prompt = torch.as_tensor(prompt_ids, dtype=torch.int64).reshape(-1).to(dev)
    P = int(prompt.numel())
    conts = [torch.as_tensor(c, dtype=torch.int64).reshape(-1).to(dev) for c in continuations]
    if P < 1 or any(c.numel() < 1 for c in conts):
        raise ValueError("score_continuations: the prompt and every continuation need at least one token")
    patch = bool(getattr(model, "audio_patch_branch", False))              # the MPT wrapper
    plan_kw = dict(patch_branch=True) if patch else {}
    cfg = model.get_model().audio_encoder_config
    feats = None if encoding is None else torch.as_tensor(encoding).to(device=dev, dtype=torch.float32)
    order = sorted(range(len(conts)), key=lambda i: conts[i].numel()) if patch else list(range(len(conts)))
    batches: List[List[int]] = []
    for i in order:
        if batches and len(batches[-1]) < eng.max_batch and (not patch or conts[batches[-1][0]].numel() == conts[i].numel()):
            batches[-1].append(i)
        else:
            batches.append([i])
    pending = []
    for batch in batches:
        B, S = len(batch), P + max(conts[i].numel() for i in batch)
        ids = torch.zeros((B, S), dtype=torch.int64, device=dev)
        tokens = torch.full((B, S), -1, dtype=torch.int64, device=dev)
        for b, i in enumerate(batch):
            n = conts[i].numel()
            ids[b, :P] = prompt
            ids[b, P: P + n] = conts[i]
            tokens[b, P - 1: P - 1 + n] = conts[i]
        segs = [] if feats is None else list(plan_audio_splice(ids, [feats] * B, cfg, False, **plan_kw))
        logits = eng.forward_tokens(ids, segs).reshape(B * S, -1)
        tokens = tokens.view(-1)
        if logits_sink is not None:
            logits_sink.append((logits, tokens))
        lp = torch.full((B * S,), float("nan"), dtype=torch.float32, device=dev)
        ops.token_logprob_rows(logits, tokens, lp)
        pending.append((batch, lp.view(B, S)))
    out: List[Optional[torch.Tensor]] = [None] * len(conts)
    for batch, lp in pending:
        host = lp.cpu()
        for b, i in enumerate(batch):
            out[i] = host[b, P - 1: P - 1 + conts[i].numel()].clone()
    return out


def _rows_to_records(example_ids, prompt, outs, end_seq, tokenizer) -> List[Dict[str, str]]:
    recs = []
    for ex, ids in zip(example_ids, outs):
        completion = tokenizer.decode(extract_response_tokens(ids, end_seq))
        recs.append({"example_id": ex, "prompt_text": prompt, "model_completion_text": completion})
    return recs


def _write_csv(records: List[Dict[str, str]], outfile: Optional[str]) -> None:
    if not outfile:
        return
    import pandas as pd

    d = os.path.dirname(outfile)
    if d and not os.path.exists(d):
        os.makedirs(d)
    pd.DataFrame(records, columns=["example_id", "prompt_text", "model_completion_text"]).to_csv(outfile, index=False)


def infer_from_encodings(model, tokenizer, audio_encodings_dir: str, prompt: str, multimodal_cfg: Dict[str, Any],
                         end_seq: Sequence[int], outfile: Optional[str] = None, batch_size: int = 8,
                         max_samples: Optional[int] = None, max_new_tokens: int = 512, audio_first: bool = True,
                         embed_dim: Optional[int] = None, num_beams: int = 1, length_penalty: float = 1.0,
                         no_repeat_ngram_size: Optional[int] = None, min_new_tokens: Optional[int] = None,
                         prompt_lookup_num_tokens: Optional[int] = None) -> List[Dict[str, str]]:
    """Directory of ``*.npy`` -> CSV, like ``scripts/inference/infer_from_encodings.py:main`` (same record fields; files
    in sorted order; ``example_id`` = path without ``.npy``).  Examples are grouped by frame count so that every batch
    shares one prompt length.  ``num_beams`` > 1: beam search with ``length_penalty``, one example per call (:func:`generate_beam`).
    ``no_repeat_ngram_size`` / ``min_new_tokens`` go to ``model.generate`` on both paths (:mod:`llark_amd.m2t.constraints`).
    ``prompt_lookup_num_tokens`` K (1 .. 7; None or 0: off): speculative greedy decoding by prompt lookup
    (:mod:`llark_amd.m2t.speculate`), ``batch_size * (K + 1) <= 16``; refused by ``generate`` next to beams or constraints."""
    from .constraints import constraints_from_generate

    constraints_from_generate(no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens)      # bad values raise here, by name
    more = {k: v for k, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens),
                              ("prompt_lookup_num_tokens", prompt_lookup_num_tokens)) if v}
    if embed_dim is None:                                  # 4800 for Jukebox, 512 for CLAP (ModelArguments.mm_hidden_size)
        embed_dim = int(getattr(getattr(model, "config", None), "mm_hidden_size", EMBED_DIM))
    paths = sorted(glob.glob(os.path.join(audio_encodings_dir, "*.npy")))
    if max_samples:
        paths = paths[:max_samples]
    by_frames: Dict[int, List[Tuple[str, np.ndarray]]] = {}
    for p in paths:
        a = load_encoding(p, embed_dim)
        by_frames.setdefault(a.shape[0], []).append((p, a))
    records: Dict[str, Dict[str, str]] = {}
    for frames, items in by_frames.items():
        prompt_ids = build_prompt_ids(prompt, frames, tokenizer, multimodal_cfg, end_seq, audio_first)
        for i in range(0, len(items), batch_size):
            chunk = items[i: i + batch_size]
            enc = torch.from_numpy(np.stack([a for _, a in chunk])).cuda()
            ids = prompt_ids.unsqueeze(0).repeat(len(chunk), 1)
            if num_beams is not None and num_beams != 1:
                outs = generate_beam(model, ids, enc, tokenizer, max_new_tokens, num_beams, length_penalty, **more)
            else:
                outs = generate_batch(model, ids, enc, tokenizer, max_new_tokens, **more)
            for rec in _rows_to_records([p[: -len(".npy")] for p, _ in chunk], prompt, outs, end_seq, tokenizer):
                records[rec["example_id"]] = rec
    ordered = [records[p[: -len(".npy")]] for p in paths]
    _write_csv(ordered, outfile)
    return ordered


def infer_from_audio(encoder, model, tokenizer, clips: Iterable[Tuple[str, np.ndarray]], prompt: str,
                     multimodal_cfg: Dict[str, Any], end_seq: Sequence[int], outfile: Optional[str] = None, batch_size: int = 8,
                     max_new_tokens: int = 512, audio_first: bool = True) -> List[Dict[str, str]]:
    """Fused driver: ``clips`` yields ``(example_id, mono float32 audio @44.1 kHz)``; ``encoder`` is a
    ``llark_amd.jukebox.extract.WrappedAudioEncoder``.  Audio is normalised / padded / truncated exactly as
    ``jukebox/main.py:29-59`` does, encoded in batches on the GPU, short clips keep only the frames of their own audio
    (``jukebox/main.py:147``), and the ``(B, frames, 4800)`` tensor is handed to ``generate`` without leaving device memory."""
    from ..jukebox import extract as E

    records: List[Dict[str, str]] = []
    buf: List[Tuple[str, np.ndarray]] = []
    prompt_cache: Dict[int, torch.Tensor] = {}

    def flush():
        if not buf:
            return
        from math import floor

        hps = encoder.hps
        n = hps.sample_length
        norm = [E._normalize(a) for _, a in buf]
        audio = np.stack([E.maybe_pad_audio_to_max_len(a, n)[:n].astype(np.float32) for a in norm])
        emb = encoder(torch.from_numpy(audio).to(encoder.vqvae.device))                  # (B, frames, 4800) fp32, on device
        # jukebox/main.py:147: activations are truncated to latent_audio_len = floor(T * len / expected) BEFORE pooling, so a clip
        # shorter than 23.8 s yields fewer frames (no embeddings of the zero padding).  Group the batch by frame count so that
        # every generate call shares one prompt length, exactly as the .npy pipeline (infer_from_encodings) does.
        fl = encoder.frame_len
        frames = [min(floor(hps.n_ctx * len(a) / n), hps.n_ctx) // fl for a in norm]
        recs: Dict[int, Dict[str, str]] = {}
        for f in sorted(set(frames)):
            if f == 0:
                raise ValueError("infer_from_audio: a clip is shorter than one pooled frame (%d samples)" % (fl * hps.raw_to_tokens))
            rows = [i for i, fi in enumerate(frames) if fi == f]
            if f not in prompt_cache:
                prompt_cache[f] = build_prompt_ids(prompt, f, tokenizer, multimodal_cfg, end_seq, audio_first)
            ids = prompt_cache[f].unsqueeze(0).repeat(len(rows), 1)
            sub = emb[torch.tensor(rows, device=emb.device), :f].contiguous()
            outs = generate_batch(model, ids, sub, tokenizer, max_new_tokens)
            for i, rec in zip(rows, _rows_to_records([buf[i][0] for i in rows], prompt, outs, end_seq, tokenizer)):
                recs[i] = rec
        records.extend(recs[i] for i in range(len(buf)))
        buf.clear()

    for item in clips:
        buf.append(item)
        if len(buf) == batch_size:
            flush()
    flush()
    _write_csv(records, outfile)
    return records


SHARD_COLUMNS = ["example_id", "prompt_text", "original_completion_text", "model_completion_text"]
LOGPROB_COLUMNS = ["sum_logprob", "mean_logprob", "n_tokens"]


def infer_from_shards(model, tokenizer, shards: str, multimodal_cfg: Dict[str, Any], end_seq: Sequence[int], outfile: Optional[str] = None,
                      slots: int = 8, max_samples: Optional[int] = None, max_new_tokens: int = 512, prompt: Optional[str] = None,
                      seed: int = 0, allow_pickle: bool = False, header: str = DEFAULT_CONVERSATION_HEADER,
                      share_prefix: bool = False, sampling=None, logprobs: bool = False,
                      num_beams: Optional[int] = None, constraints=None, choice_sets=None, choice_of=None) -> List[Dict[str, str]]:
    """Local tar shards -> CSV under the contract of ``scripts/inference/infer_from_webdataset.py:51-151``: every (question,
    answer) pair of a sample is one example whose prompt is its own human turn up to "### Assistant:" (audio placeholder first
    or last by a draw seeded with ``seed``); ``prompt`` overrides every question (the reference's ``--prompt``: audio first).
    Records ``example_id`` (the sample's tar key, repeated across its questions), ``prompt_text``, ``original_completion_text``
    (the pair's answer) and ``model_completion_text``, in input order.  ``max_samples`` caps the number of examples.  All
    generation runs through :func:`generate_inflight` with ``slots`` batch slots.  ``share_prefix``: the questions of one sample
    (its tar key is their ``prefix_key``) share the K/V of their common leading tokens when the audio placeholder comes first.
    ``sampling``: a :class:`llark_amd.m2t.sampling.SamplingParams` (its ``seed`` is the draws'; ``seed`` here shuffles the questions).
    ``logprobs``: every record also gets ``sum_logprob``, ``mean_logprob`` and ``n_tokens`` over ALL generated tokens (the stop keyword or
    EOS included, although the completion text drops it): log-probabilities of the model's distribution -- log-softmax of the raw
    logits; repetition penalty, temperature, top-k and top-p are not applied, for sampled tokens too.  ``constraints``: a
    :class:`llark_amd.m2t.constraints.TokenConstraints`, as in :func:`generate_inflight`.  ``choice_sets``: the closed answer sets, as in
    :func:`generate_inflight`; ``choice_of(conversation)`` -- the example's record, whose ``id`` is the sample's tar key -- returns the
    index of its set or None for a free answer (default with ONE set: every example takes it)."""
    from .data import element_to_conversations, expand_urls, iter_tar_samples

    refuse_beams("infer_from_shards", num_beams)
    if choice_of is not None and choice_sets is None:
        raise ValueError("infer_from_shards: choice_of without choice_sets")
    if choice_sets is not None and choice_of is None:
        if len(choice_sets.sets if hasattr(choice_sets, "sets") else choice_sets) != 1:
            raise ValueError("infer_from_shards: several choice_sets need choice_of, which names each example's set")

        def choice_of(conv):
            return 0
    rng = random.Random(seed)
    meta: List[Dict[str, str]] = []

    def examples():
        for elem in iter_tar_samples(expand_urls(shards), allow_pickle):
            for conv in element_to_conversations(elem, rng):
                if max_samples and len(meta) >= max_samples:
                    return
                ex = preprocess_for_lm_mappable(preprocess_multimodal_mappable(conv, multimodal_cfg), tokenizer=tokenizer, header=header)
                enc = ex["audio_encoding"].float()
                if prompt is None:
                    ids = extract_prompt_tokens(ex["input_ids"], end_seq)
                    prompt_text = tokenizer.decode(ids)
                else:
                    ids = build_prompt_ids(prompt, enc.shape[0], tokenizer, multimodal_cfg, end_seq, True, header)
                    prompt_text = prompt
                meta.append({"example_id": conv["id"], "prompt_text": prompt_text,
                             "original_completion_text": tokenizer.decode(extract_response_tokens(ex["input_ids"], end_seq))})
                if choice_sets is None:
                    yield ids, enc, None, conv["id"]
                else:
                    yield ids, enc, None, conv["id"], choice_of(conv)

    outs: Dict[int, torch.Tensor] = {}
    lps: Dict[int, torch.Tensor] = {}
    for item in generate_inflight(model, examples(), slots=slots, max_new_tokens=max_new_tokens, tokenizer=tokenizer,
                                  share_prefix=share_prefix, sampling=sampling, **(dict(return_logprobs=True) if logprobs else {}),
                                  **({} if constraints is None else dict(constraints=constraints)),
                                  **({} if choice_sets is None else dict(choice_sets=choice_sets))):
        outs[item[0]] = item[1]
        if logprobs:
            lps[item[0]] = item[2]
    records = []
    for i, m in enumerate(meta):
        rec = dict(m, model_completion_text=tokenizer.decode(extract_response_tokens(outs[i], end_seq)))
        if logprobs:
            lp = lps[i].double()
            rec.update(sum_logprob=float(lp.sum()), mean_logprob=float(lp.mean()), n_tokens=int(lp.numel()))
        records.append(rec)
    if outfile:
        import pandas as pd

        d = os.path.dirname(outfile)
        if d and not os.path.exists(d):
            os.makedirs(d)
        pd.DataFrame(records, columns=SHARD_COLUMNS + (LOGPROB_COLUMNS if logprobs else [])).to_csv(outfile, index=False)
    return records


def get_prompt_end_token_sequence(tokenizer, model_name: str, prompt_end_string: str = "\n### Assistant:") -> List[int]:
    """m2t/tokenizer.py:33-52: the token ids that mark the end of the prompt; the Llama-2 SentencePiece tokenizer prepends a
    piece to a string that starts with a newline, which is dropped."""
    end_seq = tokenizer([prompt_end_string], add_special_tokens=False).input_ids[0]
    if "meta-llama/Llama-2" in model_name:
        end_seq = end_seq[1:]
    return list(end_seq)


def main(argv=None):
    """CLI with the flags of the reference's ``scripts/inference/infer_from_encodings.py:120-156`` (+ ``--batch-size``):
    python -m llark_amd.m2t.infer_driver --model_name_or_path <dir> --audio-encodings-dir reps/ --prompt "What genre is this song?" \
        --outfile results/infer.csv [--max-samples N] [--max_new_tokens 512] [--batch-size 8] [--mm_hidden_size 4800]"""
    import argparse

    ap = argparse.ArgumentParser(description="LLark inference over a directory of audio encodings on the HIP engine")
    ap.add_argument("--model_name_or_path", required=True)
    ap.add_argument("--audio-encodings-dir", required=True)
    ap.add_argument("--prompt", required=True)
    ap.add_argument("--outfile", default="infer_results.csv")
    ap.add_argument("--max-samples", type=int, default=None)
    ap.add_argument("--max_new_tokens", type=int, default=512)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--mm_hidden_size", type=int, default=None)
    ap.add_argument("--model_max_length", type=int, default=2048)
    ap.add_argument("--llm-precision", default="split", choices=["split", "bf16"])
    ap.add_argument("--num_beams", type=int, default=1, help="beam search with this many beams (1 .. 16), one example per call; 1: greedy")
    ap.add_argument("--length_penalty", type=float, default=1.0, help="hypothesis score = sum of log-probabilities / length ** this")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0, help="no n-gram of this size occurs twice in prompt + completion; 0: off")
    ap.add_argument("--min_new_tokens", type=int, default=0, help="the EOS token is banned for this many new tokens; 0: off")
    ap.add_argument("--prompt_lookup_num_tokens", type=int, default=0,
                    help="speculative greedy decoding: verify this many tokens (1 .. 7) looked up in the row's own history per step; 0: off")
    for ignored in ("--ckpt-num", "--report_to", "--bf16", "--tf32", "--output_dir"):
        ap.add_argument(ignored, default=None, help="accepted for script compatibility")
    args = ap.parse_args(argv)
    from .constraints import constraints_from_generate

    try:                                                   # before the model is loaded
        constraints_from_generate(no_repeat_ngram_size=args.no_repeat_ngram_size, min_new_tokens=args.min_new_tokens)
        from .speculate import SpeculationParams
        spec = SpeculationParams.from_generate(args.prompt_lookup_num_tokens)
        if spec is not None:
            spec.check_batch(args.batch_size)
    except ValueError as e:
        ap.error(str(e))
    model, tok, end_seq, mm_cfg = _load_for_inference(args, max(args.batch_size, args.num_beams))
    recs = infer_from_encodings(model, tok, args.audio_encodings_dir, args.prompt, mm_cfg, end_seq, outfile=args.outfile,
                                batch_size=args.batch_size, max_samples=args.max_samples, max_new_tokens=args.max_new_tokens,
                                num_beams=args.num_beams, length_penalty=args.length_penalty,
                                **{k: v for k, v in (("no_repeat_ngram_size", args.no_repeat_ngram_size), ("min_new_tokens", args.min_new_tokens),
                                                     ("prompt_lookup_num_tokens", args.prompt_lookup_num_tokens)) if v})
    print(f"writing {len(recs)} results to {args.outfile}")
    return recs


def _load_tokenizer(args):
    """The tokenizer of either backbone, loaded as llark_amd/m2t/train.py:main does."""
    from transformers import AutoTokenizer

    return AutoTokenizer.from_pretrained(args.model_name_or_path, model_max_length=args.model_max_length, padding_side="right", use_fast=False)


def _load_for_inference(args, max_batch: int):
    """Tokenizer + model of ``args.model_name_or_path`` set up for generation (audio tokens, engine) -> (model, tokenizer, end_seq,
    multimodal config)."""
    from .special_tokens import DEFAULT_AUDIO_END_TOKEN, DEFAULT_AUDIO_PATCH_TOKEN, DEFAULT_AUDIO_START_TOKEN
    from .train import backbone_of

    tok = _load_tokenizer(args)
    if backbone_of(args.model_name_or_path) == "mpt":          # the reference's rule (m2t/train.py:62), as in this project's train.main
        from .mpt import WrappedMPTForCausalLM

        model = WrappedMPTForCausalLM.from_pretrained(args.model_name_or_path, torch_dtype=torch.bfloat16, mm_hidden_size=args.mm_hidden_size)
    else:
        from .llamav2 import WrappedLlamav2ForCausalLM

        model = WrappedLlamav2ForCausalLM.from_pretrained(args.model_name_or_path, torch_dtype=torch.bfloat16)
    if args.mm_hidden_size:
        model.config.mm_hidden_size = args.mm_hidden_size
    if tok.pad_token is None:                                           # m2t/train.py:110-124 adds it at training time
        tok.add_special_tokens(dict(pad_token="[PAD]"))
        model.resize_token_embeddings(len(tok))
    if not hasattr(model.get_model(), "mm_projector"):
        model.get_model().initialize_adapter_modules()
    known = set(tok.get_vocab())
    if {DEFAULT_AUDIO_PATCH_TOKEN, DEFAULT_AUDIO_START_TOKEN, DEFAULT_AUDIO_END_TOKEN} <= known and model.get_input_embeddings().weight.shape[0] >= len(tok):
        ac = model.get_model().audio_encoder_config                      # a trained checkpoint: the tokens are already in place
        ac.use_audio_start_end = True
        ac.audio_patch_token, ac.audio_start_token, ac.audio_end_token = tok.convert_tokens_to_ids(
            [DEFAULT_AUDIO_PATCH_TOKEN, DEFAULT_AUDIO_START_TOKEN, DEFAULT_AUDIO_END_TOKEN])
    else:
        model.initialize_audio_tokenizer(mm_use_audio_start_end=True, tokenizer=tok, device="cpu")
    model.cuda().eval()
    model.configure_engine(max_batch=max_batch, max_seq=args.model_max_length, precision=args.llm_precision)
    end_seq = get_prompt_end_token_sequence(tok, args.model_name_or_path)
    mm_cfg = dict(is_multimodal=True, sep_audio_conv_front=False, use_audio_start_end=True)
    return model, tok, end_seq, mm_cfg


def main_shards(argv=None):
    """``shards`` mode, with the flags of the reference's ``scripts/inference/infer_from_webdataset.py:154-190`` (+ ``--slots``):
    python -m llark_amd.m2t.infer_driver shards --model_name_or_path <dir> --eval_data_path "shards-{000000..000021}.tar" \
        --outfile results/infer.csv [--prompt "Describe ..."] [--max-samples N] [--max_new_tokens 2048] [--slots 8] [--allow-pickle]
        [--share-prefix] [--do-sample --temperature 0.8 --top-k 50 --top-p 0.9 --sample-seed 0] [--repetition-penalty 1.3] [--logprobs]
        [--no-repeat-ngram-size 3] [--min-new-tokens 8] [--choices-json labels.json]
    ``--allow-pickle``: read ``.pyd`` (pickled) encodings -- unpickling runs code, pass it only for shards you trust."""
    import argparse

    ap = argparse.ArgumentParser(description="LLark inference over local webdataset shards on the HIP engine (in-flight batching)")
    ap.add_argument("--model_name_or_path", required=True)
    ap.add_argument("--eval_data_path", required=True)
    ap.add_argument("--prompt", default=None)
    ap.add_argument("--outfile", default="infer_results.csv")
    ap.add_argument("--max-samples", type=int, default=None)
    ap.add_argument("--max_new_tokens", type=int, default=2048)
    ap.add_argument("--slots", type=int, default=8, help="examples that decode together, 1 .. 64 (each slot holds a KV cache of "
                    "--model_max_length positions: about 1 GiB per slot at 7B, 1024 positions, split precision)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--allow-pickle", action="store_true")
    ap.add_argument("--share-prefix", action="store_true", help="the questions of one sample share the K/V of their common leading "
                    "tokens (audio placeholder first): prefilled once, read once per group in the decode step")
    ap.add_argument("--do-sample", action="store_true", help="draw the tokens on the device instead of taking the greedy one "
                    "(scripts/inference/infer_from_webdataset.py:102-103 keeps do_sample / temperature commented out)")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0, help="0: off")
    ap.add_argument("--top-p", type=float, default=1.0, help="1: off")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="1: off; applies to greedy decoding too")
    ap.add_argument("--sample-seed", type=int, default=0, help="seed of the draws (--seed is the question shuffle's); a completion "
                    "depends on it and on the example's index, not on --slots")
    ap.add_argument("--num_beams", type=int, default=1, help="refused above 1: beam search is not scheduled in flight")
    ap.add_argument("--logprobs", action="store_true", help="add the columns sum_logprob, mean_logprob and n_tokens: log-probabilities of the "
                    "generated tokens under the model's raw logits (no penalty, temperature, top-k or top-p applied), computed on the device")
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0, help="no n-gram of this size occurs twice in prompt + completion "
                    "(1 .. 64; 0: off); the bans are computed on the device from the example's own history")
    ap.add_argument("--min-new-tokens", type=int, default=0, help="the EOS token is banned for this many new tokens (0: off); an example's "
                    "own budget below it wins")
    ap.add_argument("--choices-json", default=None, help="a file holding a JSON list of strings: the closed answer set of every example "
                    "(each tokenised after a space, without special tokens); every completion is then one of them, chosen on the device")
    ap.add_argument("--mm_hidden_size", type=int, default=None)
    ap.add_argument("--model_max_length", type=int, default=2048)
    ap.add_argument("--llm-precision", default="split", choices=["split", "bf16"])
    for ignored in ("--ckpt-num", "--report_to", "--bf16", "--tf32", "--output_dir"):
        ap.add_argument(ignored, default=None, help="accepted for script compatibility")
    args = ap.parse_args(argv)
    from .constraints import constraints_from_generate
    from .guide import choices_from_json, choices_from_strings
    from .sampling import SamplingParams

    try:
        choices = None
        if args.choices_json is not None:
            with open(args.choices_json) as f:
                choices = choices_from_json(f.read())
        sampling = SamplingParams(do_sample=args.do_sample, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                  repetition_penalty=args.repetition_penalty, seed=args.sample_seed)
        constraints = constraints_from_generate(no_repeat_ngram_size=args.no_repeat_ngram_size, min_new_tokens=args.min_new_tokens)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    if not 1 <= args.slots <= 64:
        ap.error(f"--slots must be in 1 .. 64, got {args.slots}")
    refuse_beams("shards", args.num_beams)
    from .train import backbone_of

    if args.share_prefix and backbone_of(args.model_name_or_path) == "mpt":
        ap.error("--share-prefix is not available for an MPT model: the shared-prefix decode attention takes no ALiBi bias")
    model, tok, end_seq, mm_cfg = _load_for_inference(args, args.slots)
    recs = infer_from_shards(model, tok, args.eval_data_path, mm_cfg, end_seq, outfile=args.outfile, slots=args.slots,
                             max_samples=args.max_samples, max_new_tokens=args.max_new_tokens, prompt=args.prompt, seed=args.seed,
                             allow_pickle=args.allow_pickle, share_prefix=args.share_prefix, sampling=sampling if sampling.active else None,
                             **(dict(logprobs=True) if args.logprobs else {}),
                             **({} if constraints is None else dict(constraints=constraints)),
                             **({} if choices is None else dict(choice_sets=[choices_from_strings(tok, choices)])))
    print(f"writing {len(recs)} results to {args.outfile}")
    return recs


if __name__ == "__main__":
    import sys

    if len(sys.argv) > 1 and sys.argv[1] == "shards":
        main_shards(sys.argv[2:])
    else:
        main()
