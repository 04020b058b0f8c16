"""Training data path of the native loop: reads the reference's shard format without the ``webdataset`` dependency.

The reference streams tar shards (``m2t/data_modules.py:466-520`` ``read_webdataset``): every sample is a group of tar
members sharing a key -- ``<key>.json`` (``{"response": [{"question": ..., "answer": ...}, ...]}``) and
``<key>.audio_encoding.pyd`` (a pickled array) -- which ``webdataset_element_to_conversation`` (:295-340) unpacks into one
conversation per question/answer pair with the ``<audio>`` placeholder randomly first or last; the conversations then go
through ``preprocess_multimodal_mappable`` / ``preprocess_for_lm_mappable`` and the collator (llark_amd.m2t.prompting).

Here: a pure-``tarfile`` reader for local shards (``.npy`` members are read natively; ``.pyd`` pickles only with
``allow_pickle=True`` -- unpickling is code execution, the caller must trust the shards), brace expansion of
``name-{000..127}.tar`` lists (:436-438), the per-rank shard split of ``wds.split_by_node``, and a micro-batch generator
for ``llark_amd.m2t.train.train``; with ``task_sample_probs`` the shard order of an epoch is drawn WITH replacement, each shard
weighted by the probability of the task whose name its path contains (``repeat_shards``, :441-463; off unless
``--apply_task_sample_probs``, as in m2t/arguments.py:61-68).  GCS URLs and the HF ``IterableDataset`` wrapper are not built
(I/O glue outside the hot path).
"""
from __future__ import annotations

import io
import json
import pickle
import random
import re
import tarfile
from dataclasses import dataclass
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .prompting import (DataCollatorForSupervisedDataset, concat_audio_token_and_prompt, preprocess_for_lm_mappable,
                        preprocess_multimodal_mappable)

_RANGE = re.compile(r"\{(\d+)\.\.(\d+)\}")


def expand_urls(url: str) -> List[str]:
    """``"a-{000..002}.tar,b.tar"`` -> ``[a-000.tar, a-001.tar, a-002.tar, b.tar]`` (numeric ranges, zero padding kept)."""
    out: List[str] = []
    for part in url.split(","):
        part = part.strip()
        if not part:
            continue
        todo = [part]
        while todo:
            cur = todo.pop(0)
            m = _RANGE.search(cur)
            if not m:
                out.append(cur)
                continue
            lo, hi, width = int(m.group(1)), int(m.group(2)), len(m.group(1))
            todo = [cur[: m.start()] + str(i).zfill(width) + cur[m.end():] for i in range(lo, hi + 1)] + todo
    return out


DEFAULT_TASK_SAMPLE_PROBS = {"captioning": 0.15, "reasoning": 0.55, "mir": 0.3}      # m2t/arguments.py:61-67


def shard_probs(urls: Sequence[str], task_sample_probs: Dict[str, float]) -> List[float]:
    """``repeat_shards`` (m2t/data_modules.py:441-457): a shard's weight is the probability of the FIRST task key contained in
    its name, normalised over the list; a shard matching no key is an error."""
    probs = []
    for shard in urls:
        for k, prob in task_sample_probs.items():
            if k in shard:
                probs.append(float(prob))
                break
        else:
            raise ValueError(f"probability for shard {shard} not defined in probs {task_sample_probs}")
    total = sum(probs)
    if total <= 0:
        raise ValueError(f"task probabilities {task_sample_probs} give the shard list zero total weight")
    return [p / total for p in probs]


def split_by_rank(urls: Sequence[str], rank: int, world: int) -> List[str]:
    """``wds.split_by_node``: rank r reads shards r, r + world, ...  (every rank needs at least one shard)."""
    mine = list(urls[rank::world])
    if not mine:
        raise ValueError(f"{len(urls)} shard(s) cannot be split over {world} ranks")
    return mine


def _decode_member(name: str, data: bytes, allow_pickle: bool):
    if name.endswith(".json"):
        return json.loads(data.decode("utf-8"))
    if name.endswith(".npy"):
        return np.load(io.BytesIO(data), allow_pickle=False)
    if name.endswith(".pyd"):
        if not allow_pickle:
            raise ValueError(f"{name}: pickled member; pass allow_pickle=True only for shards you trust (or store .npy)")
        obj = pickle.loads(data)
        return obj.numpy() if isinstance(obj, torch.Tensor) else np.asarray(obj)
    return data


def iter_tar_samples(shards: Iterable[str], allow_pickle: bool = False) -> Iterator[Dict[str, Any]]:
    """Yields ``{"__key__", "__url__", "json", "audio_encoding.<ext>", ...}`` per key, in tar order (members of one sample
    are adjacent, as webdataset requires)."""
    for url in shards:
        with tarfile.open(url, "r:*") as tf:
            cur: Dict[str, Any] = {}
            for member in tf:
                if not member.isfile():
                    continue
                base = member.name.rsplit("/", 1)[-1]
                key, _, ext = base.partition(".")
                if cur and cur["__key__"] != key:
                    yield cur
                    cur = {}
                if not cur:
                    cur = {"__key__": key, "__url__": url}
                cur[ext] = _decode_member(base, tf.extractfile(member).read(), allow_pickle)
            if cur:
                yield cur


def element_to_conversations(elem: Dict[str, Any], rng: random.Random) -> Iterator[Dict[str, Any]]:
    """m2t/data_modules.py:295-340: one training example per (question, answer) of a sample; malformed samples are skipped."""
    js = elem.get("json")
    if not isinstance(js, dict) or not isinstance(js.get("response"), list) or not js["response"]:
        return
    enc = elem.get("audio_encoding.pyd", elem.get("audio_encoding.npy"))
    if enc is None or not hasattr(enc, "shape"):
        return
    for resp in js["response"]:
        audio_first = rng.uniform(0.0, 1.0) > 0.5
        yield {"audio_encoding": enc, "audio_encoding_shape": list(enc.shape), "id": elem["__key__"],
               "conversations": [{"from": "human", "value": concat_audio_token_and_prompt(resp["question"], audio_first)},
                                 {"from": "gpt", "value": resp["answer"]}]}


SHUFFLE_BUFFER = 100          # m2t/data_modules.py: dataset.shuffle(100) after webdataset_element_to_conversation


def _shuffled(items: Iterator[Dict[str, Any]], rng: random.Random, size: int) -> Iterator[Dict[str, Any]]:
    """webdataset's bounded shuffle: keep ``size`` items, emit a random one as each new item arrives, drain at the end."""
    buf: List[Dict[str, Any]] = []
    for it in items:
        if len(buf) < size:
            buf.append(it)
            continue
        j = rng.randrange(size)
        buf[j], it = it, buf[j]
        yield it
    rng.shuffle(buf)
    yield from buf


def micro_batches(train_data_path: str, tokenizer, multimodal_cfg: Dict[str, Any], batch_size: int, model_max_length: int,
                  rank: int = 0, world: int = 1, seed: int = 0, epochs: Optional[int] = None, allow_pickle: bool = False,
                  shuffle_buffer: int = SHUFFLE_BUFFER, skip_micro_batches: int = 0,
                  task_sample_probs: Optional[Dict[str, float]] = None):
    """Collated micro-batches (``input_ids``, ``labels``, ``attention_mask``, ``audio_encodings``) of THIS rank, forever
    (``epochs=None``, like the reference's ``repeat()``) or for a number of passes over its shards.

    Order (m2t/data_modules.py:560-640): shards shuffled per epoch, then the (question, answer) examples go through a
    bounded shuffle buffer of ``shuffle_buffer`` conversations so that the pairs of one clip are not emitted back to back;
    both generators are seeded per rank AND per epoch.  ``skip_micro_batches`` fast-forwards the stream (resume: the
    trainer passes ``step * gradient_accumulation_steps``) so a resumed run continues where the interrupted one stopped
    instead of replaying its first samples.  ``task_sample_probs``: see :func:`shard_probs` -- an epoch then reads as many shards
    as the rank owns, drawn with replacement by task weight over the WHOLE shard list (one draw shared by all ranks, then split
    r::world; the reference draws 1024 x len(urls) up front, before split_by_node)."""
    all_shards = expand_urls(train_data_path)
    shards = split_by_rank(all_shards, rank, world)
    # task weights are normalised over the GLOBAL shard list and the weighted order is drawn over it with a RANK-INDEPENDENT seed, then
    # split by rank -- the reference's repeat_shards() runs before split_by_node (m2t/data_modules.py:441-462, 560-640), so every rank
    # sees the task mix of the whole list, also when its own r::world subset is skewed or lacks a task
    weights = shard_probs(all_shards, task_sample_probs) if task_sample_probs else None
    collate = DataCollatorForSupervisedDataset(tokenizer)
    epoch = 0
    to_skip = max(0, int(skip_micro_batches))                         # whole micro-batches still to fast-forward over
    while epochs is None or epoch < epochs:
        rng = random.Random((seed * 1000003 + rank) * 7919 + epoch)
        if weights is None:
            order = list(shards)
            rng.shuffle(order)                                        # shardshuffle
        else:
            grng = random.Random(seed * 1000003 * 7919 + epoch)          # the same draw on every rank
            order = grng.choices(all_shards, weights=weights, k=len(shards) * world)[rank::world]

        def conversations():
            for elem in iter_tar_samples(order, allow_pickle):
                yield from element_to_conversations(elem, rng)

        stream = _shuffled(conversations(), rng, shuffle_buffer) if shuffle_buffer and shuffle_buffer > 1 else conversations()
        pending: List[Dict[str, Any]] = []
        skip_pending = 0      # conversations of the micro-batch being skipped; like `pending`, an epoch's remainder is dropped
        for conv in stream:
            if to_skip > 0:                                           # fast-forward without tokenising
                skip_pending += 1
                if skip_pending == batch_size:
                    to_skip -= 1
                    skip_pending = 0
                continue
            ex = preprocess_for_lm_mappable(preprocess_multimodal_mappable(conv, multimodal_cfg), tokenizer=tokenizer)
            ex["input_ids"], ex["labels"] = ex["input_ids"][:model_max_length], ex["labels"][:model_max_length]
            pending.append(ex)
            if len(pending) == batch_size:
                yield collate(pending)
                pending = []
        epoch += 1


# ---- packed ragged step (``--pack_sequences``): a whole optimizer step as ONE row stream ------------------------------------------------
IGNORE_INDEX = -100
PACK_ALIGN = 8               # every sequence starts at a multiple of 8 rows (the attention forward reads V^T in chunks of 8 keys)


@dataclass
class PackedStep:
    """The micro-batches of one optimizer step as a single stream of ``s_total`` rows with no padded sequence: sequence b occupies rows
    ``off_b .. off_b + len_b - 1`` (``len_b`` = its token count rounded up to PACK_ALIGN with ``pad_id`` / label -100; the pad rows follow
    their own sequence's tokens in the causal order, get no loss and so contribute exactly zero to every gradient)."""
    ids: torch.Tensor                          # int64 [s_total]
    labels: torch.Tensor                       # int64 [s_total]: first row of every sequence and every pad row are -100 (no row predicts across a boundary)
    seqs: List[Tuple[int, int]]                # (off_b, len_b), off_b % 8 == 0, contiguous: no row of the stream lies outside a sequence
    groups: List[Tuple[int, int]]              # [r0, r1) of each micro-batch: the loss is the mean over the micro-batches of each one's token mean
    segments: list                             # (sequence index, position of <audio_start> inside the sequence, frames)
    positions: torch.Tensor                    # int64 [s_total]: RoPE position of a row = its index inside its sequence
    tokens: List[int]                          # unpadded length of every sequence

    @property
    def s_total(self) -> int:
        return int(self.ids.numel())

    @property
    def max_len(self) -> int:
        return max(n for _, n in self.seqs)


def pack_sequences(seqs: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], groups: Sequence[int], segments=(), pad_id: int = 0) -> PackedStep:
    """Pure host function.  ``seqs`` / ``labels``: 1-D id / label tensors of any (equal per pair) lengths; ``groups``: how many consecutive
    sequences form each micro-batch; ``segments``: (sequence index, start, frames) with ``start`` inside the sequence."""
    if len(seqs) != len(labels) or sum(int(g) for g in groups) != len(seqs) or any(int(g) < 1 for g in groups):
        raise ValueError(f"pack_sequences: {len(seqs)} sequences, {len(labels)} label rows, groups {list(groups)} do not match")
    ids_out, lab_out, pos_out, table, tokens = [], [], [], [], []
    off = 0
    for b, (s, l) in enumerate(zip(seqs, labels)):
        s, l = s.detach().cpu().reshape(-1).long(), l.detach().cpu().reshape(-1).long()
        n = int(s.numel())
        if n < 1 or int(l.numel()) != n:
            raise ValueError(f"pack_sequences: sequence {b} has {n} tokens and {int(l.numel())} labels")
        ln = -(-n // PACK_ALIGN) * PACK_ALIGN
        ids_b = torch.full((ln,), int(pad_id), dtype=torch.long)
        lab_b = torch.full((ln,), IGNORE_INDEX, dtype=torch.long)
        ids_b[:n] = s
        lab_b[1:n] = l[1:]                                   # a sequence's first label is never a target (the loss is shifted)
        ids_out.append(ids_b)
        lab_out.append(lab_b)
        pos_out.append(torch.arange(ln, dtype=torch.long))
        table.append((off, ln))
        tokens.append(n)
        off += ln
    ranges, b0 = [], 0
    for g in groups:
        b1 = b0 + int(g)
        ranges.append((table[b0][0], table[b1 - 1][0] + table[b1 - 1][1]))
        b0 = b1
    segs = []
    for (b, start, frames) in segments:
        b, start = int(b), int(start)
        if not (0 <= b < len(table)) or start < 0 or start + 1 + int(frames.shape[0]) > tokens[b]:
            raise ValueError(f"pack_sequences: audio segment (sequence {b}, start {start}, {int(frames.shape[0])} frames) lies outside its sequence")
        segs.append((b, start, frames))
    return PackedStep(torch.cat(ids_out), torch.cat(lab_out), table, ranges, segs, torch.cat(pos_out), tokens)


def plan_packed_step(micro_batches_: Sequence[Dict[str, Any]], audio_cfg, pad_id: int) -> PackedStep:
    """The collated micro-batches of one optimizer step (``input_ids``, ``labels``, optional ``attention_mask`` / ``audio_encodings``) ->
    one :class:`PackedStep`.  Right padding is stripped with ``attention_mask``; without one, a trailing run of positions whose label is
    -100 and whose id is ``pad_id`` counts as padding.  A micro-batch none of whose rows keeps a token is refused."""
    from .llamav2 import plan_audio_splice

    seqs, labels, groups, segments = [], [], [], []
    for k, mb in enumerate(micro_batches_):
        ids, lab = mb["input_ids"].detach().cpu(), mb["labels"].detach().cpu()
        mask = mb.get("attention_mask")
        if mask is not None:
            keep = mask.detach().cpu().bool()
        else:
            keep = ~((ids == pad_id) & (lab == IGNORE_INDEX))
        lengths = []
        for b in range(ids.shape[0]):
            nz = keep[b].nonzero().reshape(-1)
            lengths.append(int(nz[-1]) + 1 if nz.numel() else 0)
        if not any(lengths):
            raise ValueError(f"plan_packed_step: micro-batch {k} has no token left after its padding is stripped")
        feats = mb.get("audio_encodings")
        segs = plan_audio_splice(ids, feats, audio_cfg, False) if feats is not None else []
        index = {}
        for b, n in enumerate(lengths):
            if n == 0:                                        # an all-padding row of a micro-batch that has others: nothing to learn from
                continue
            index[b] = len(seqs)
            seqs.append(ids[b, :n])
            labels.append(lab[b, :n])
        groups.append(len(index))
        for (b, start, frames) in segs:
            if b not in index:
                raise ValueError(f"plan_packed_step: micro-batch {k}, row {b}: audio in a row that is all padding")
            segments.append((index[b], start, frames))
    return pack_sequences(seqs, labels, groups, segments, pad_id)
