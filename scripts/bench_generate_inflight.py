#!/usr/bin/env python3
"""Generation throughput on a ragged workload: per-example batch-1 generate vs the grouped generate_batch vs in-flight slot refill.

Llama-2-7B dimensions with random weights (no checkpoint offline), 64 synthetic examples: 240 audio frames (about 1 in 4 a shorter
clip of 121 frames), prompt texts of 8-80 tokens, seeded per-example answer budgets of 16-256 tokens (random weights never emit
"###", so the budget is what makes answer lengths vary; keyword and EOS stops are off).  Schedules:
  (a) batch1   -- model.generate per example;
  (b) grouped  -- generate_batch over groups of up to 8 examples sharing one prompt length (what the uniform engine allows), each
                  group decoding until its longest budget, rows cut at their own budget;
  (c) inflight -- generate_inflight with every slot count of --slots (default 8, 16, 32, 64; above 16 slots the decode step runs on
                  ops.gemm16_mid).
Also the decode-step time of the ragged step with every slot active (1, 8, 16, 32, 48, 64 slots) and, at 16 and 64 slots, the
per-kernel split of one step from ops kernel timing.  Prints ONE JSON line.

    python scripts/bench_generate_inflight.py [--slots 8,16,32,64] [--examples N] [--schedules batch1,grouped,inflight]
                                              [--precision split] [--seed 0]
--examples defaults to 256 when a slot count above 16 is asked for (64 slots stay full for most of the run), 64 otherwise.

    python scripts/bench_generate_inflight.py --slots 16,32,64 --questions-per-clip 1,4,8 --share-prefix
Shared prompt prefixes: consecutive examples are the questions of one clip (one encoding, audio block first, one prefix key); every
(slots, questions per clip) cell runs the inflight schedule with share_prefix off and on, alternating which goes first, and records
clips/s, the decode step with every slot active, the attention launches' device time per step (ops kernel tags) and the time per
example of filling the slots.  ONE JSON line on stdout (each cell also on stderr as it finishes).

    python scripts/bench_generate_inflight.py --sampling [--slots 16,64]
Greedy against sampled decode step, same run: every slot active, blocks of 16 steps alternate between the greedy step and the step
whose tokens come from the device sampler (temperature 0.7, top-k 200, top-p 0.95, repetition penalty 1.3; one more launch per step),
which kind goes first alternating too.  Per slot count: the median block of either kind, the spread of the blocks, and the sampled
step's excess as a fraction of the greedy step.  ONE JSON line.

    python scripts/bench_generate_inflight.py --logprobs [--slots 16,64] [--out profiles/bench_generate_inflight_logprobs.json]
Greedy against greedy + token log-probabilities, same run and same block scheme: the second kind's step picks its token with
ops.sample_rows(do_sample=False) and appends its log-probability to the slot's history (ops.token_logprob_rows), two more launches per
step, as EngineSlots(logprobs=True) does.  ONE JSON line, also written to --out.

    python scripts/bench_generate_inflight.py --constraints [--slots 16,64] [--out profiles/bench_generate_inflight_constraints.json]
Greedy against constrained greedy, same run and same block scheme: the second kind's step turns its logits into the processed rows
(ops.constrain_rows under no_repeat_ngram_size 3, two bad words and min_new_tokens; the histories live on the device) and picks its
token from them with ops.sample_rows(do_sample=False), two more launches per step, as EngineSlots(constraints=...) does.  ONE JSON line,
also written to --out.

    python scripts/bench_generate_inflight.py --guided [--slots 16,64] [--out profiles/bench_generate_inflight_guided.json]
Greedy against guided greedy, same run and same block scheme: the second kind's step sets -inf outside the slot's choice set
(ops.guide_rows; 24 sequences long enough that every slot stays inside the tree for the whole run, the nodes live on the device) and picks
its token with ops.sample_rows(do_sample=False), two more launches per step, as EngineSlots(choice_sets=...) does.  ONE JSON line, also
written to --out.
"""
import argparse
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from llark_amd.m2t import bench_support as BS  # noqa: E402
from llark_amd.m2t.engine import HipLlamaEngine, LlamaDims  # noqa: E402
from llark_amd.m2t.infer_driver import generate_batch, generate_inflight  # noqa: E402
from llark_amd.m2t.llamav2 import WrappedLlamav2ForCausalLM  # noqa: E402


class _NoText:
    """generate_batch builds a keyword criterion per row; with no keywords it only needs batch_decode."""

    def __call__(self, text, **kw):
        return types.SimpleNamespace(input_ids=[0, 0])

    def batch_decode(self, rows, skip_special_tokens=False):
        return [""] * len(rows)


class RandomLlama:
    """The generate surface of WrappedLlamav2ForCausalLM (its own generate code, padded batches included) over a HipLlamaEngine with random
    Llama-2-7B weights: building the HF module at 7B on the host would take minutes and ~27 GB for weights that are random anyway."""

    generate = WrappedLlamav2ForCausalLM.generate
    prepare_inputs_for_generation = WrappedLlamav2ForCausalLM.prepare_inputs_for_generation

    def __init__(self, precision: str, max_batch: int, max_seq: int):
        dims = LlamaDims(vocab_size=BS.VOCAB)
        eng = HipLlamaEngine(dims, "cuda", max_batch=max_batch, max_seq=max_seq, precision=precision)
        g = torch.Generator(device="cuda").manual_seed(0)
        H, I = dims.hidden_size, dims.intermediate_size

        def n(*shape):
            return (torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * 0.02).to(torch.bfloat16)

        ones = torch.ones(H, device="cuda")
        for i in range(dims.num_hidden_layers):
            eng.set_layer(i, n(H, H), n(H, H), n(H, H), n(H, H), n(I, H), n(I, H), n(H, I), ones, ones)
        eng.set_globals(n(BS.VOCAB, H), ones, n(BS.VOCAB, H), n(H, dims.mm_hidden_size), torch.zeros(H, device="cuda"))
        eng.prepare_prefill()
        self.engine = eng
        self.generation_config = types.SimpleNamespace(eos_token_id=None, pad_token_id=None)
        ac = types.SimpleNamespace(use_audio_start_end=True, audio_start_token=BS.START, audio_end_token=BS.END, audio_patch_token=BS.PATCH)
        self.model = types.SimpleNamespace(audio_encoder_config=ac)

    def get_model(self):
        return self.model


def make_examples(n: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        frames = 121 if int(torch.randint(0, 4, (1,), generator=g)) == 0 else 240
        text = int(torch.randint(8, 81, (1,), generator=g))
        budget = int(torch.randint(16, 257, (1,), generator=g))
        ids = torch.tensor([1, BS.START] + [BS.PATCH] * frames + [BS.END] + torch.randint(3, 32000, (text,), generator=g).tolist())
        enc = torch.randn(frames, 4800, generator=g)
        out.append((ids, enc, budget))
    return out


def run_batch1(model, examples, tok):
    outs = {}
    for i, (ids, enc, budget) in enumerate(examples):
        outs[i] = generate_batch(model, ids[None].cuda(), enc[None].cuda(), tok, budget, keywords=())[0]
    return outs


def run_grouped(model, examples, tok, batch=8):
    by_len = {}
    for i, (ids, _, _) in enumerate(examples):
        by_len.setdefault(ids.numel(), []).append(i)
    outs, groups = {}, 0
    for _, idx in sorted(by_len.items()):
        for k in range(0, len(idx), batch):
            grp = idx[k: k + batch]
            groups += 1
            ids = torch.stack([examples[i][0] for i in grp]).cuda()
            enc = torch.stack([examples[i][1] for i in grp]).cuda()
            rows = generate_batch(model, ids, enc, tok, max(examples[i][2] for i in grp), keywords=())
            for i, r in zip(grp, rows):
                outs[i] = r[: examples[i][0].numel() + examples[i][2]]
    return outs, groups


def run_inflight(model, examples, slots):
    trace = []
    outs = dict(generate_inflight(model, iter((ids, enc.cuda(), b) for ids, enc, b in examples), slots=slots, keywords=(), trace=trace))
    return outs, sum(1 for e in trace if e[0] == "prefill")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def decode_step_ms(model, examples, n_slots, steps=32):
    """Ragged decode step with every slot active (prompts of the workload prefilled), wall clock over `steps` steps."""
    eng = model.engine
    eng.init_slots(n_slots)
    rows = [examples[i % len(examples)] for i in range(n_slots)]
    segs = [(k, 1, r[1].cuda()) for k, r in enumerate(rows)]
    logits = eng.prefill_slots([r[0].cuda() for r in rows], segs, range(n_slots))
    ids = logits.argmax(-1)
    for _ in range(4):
        ids, _, _ = eng.decode_slots(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ids, _, _ = eng.decode_slots(ids)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    split = None
    if n_slots in (16, 64):                                   # where one step's time goes: device time per kernel tag, one step
        from llark_amd import ops
        ops.start_kernel_timing()
        ids, _, _ = eng.decode_slots(ids)
        split = {k: round(v[1], 3) for k, v in sorted(ops.stop_kernel_timing().items(), key=lambda kv: -kv[1][1])}
    return ms, split


def make_clip_examples(n: int, per_clip: int, seed: int):
    """make_examples with `per_clip` consecutive examples per clip: one encoding, the audio block first (the shared prefix), a key,
    and a question and budget of their own."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        if i % per_clip == 0:
            frames = 121 if int(torch.randint(0, 4, (1,), generator=g)) == 0 else 240
            enc = torch.randn(frames, 4800, generator=g)
            head = [1, BS.START] + [BS.PATCH] * frames + [BS.END]
        text = int(torch.randint(8, 81, (1,), generator=g))
        budget = int(torch.randint(16, 257, (1,), generator=g))
        out.append((torch.tensor(head + torch.randint(3, 32000, (text,), generator=g).tolist()), enc, budget, f"clip{i // per_clip}"))
    return out


def run_inflight_keys(model, examples, slots, share):
    trace = []
    it = iter((ids, enc.cuda(), b, key) for ids, enc, b, key in examples)
    outs = dict(generate_inflight(model, it, slots=slots, keywords=(), trace=trace, share_prefix=share))
    return outs, sum(1 for e in trace if e[0] == "fork")


def full_step(model, examples, n_slots, share, steps=32):
    """Every slot active on the first n_slots examples (siblings forked from their clip's first example when `share`): ms per example
    of filling the slots, wall-clock ms per decode step, device ms of the attention launches per step (ops kernel tags), groups."""
    from llark_amd import ops
    eng = model.engine
    eng.init_slots(n_slots, share_prefix=share)
    rows = examples[:n_slots]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids = torch.zeros(n_slots, dtype=torch.int64, device="cuda")
    lead = {}
    full = [k for k, r in enumerate(rows) if not share or lead.setdefault(r[3], k) == k]
    ids[full] = eng.prefill_slots([rows[k][0].cuda() for k in full], [(j, 1, rows[k][1].cuda()) for j, k in enumerate(full)], full).argmax(-1)
    rest = [k for k in range(n_slots) if k not in full]
    if rest:
        past = [rows[k][1].shape[0] + 3 for k in rest]                   # <s> <audio_start> frames <audio_end>
        for src in sorted(set(lead.values())):                            # one copy launch per clip: its siblings share one length
            dsts = [k for k in rest if lead[rows[k][3]] == src]
            if dsts:
                eng.fork_slots(src, dsts, rows[src][1].shape[0] + 3)
        ids[rest] = eng.prefill_slots([rows[k][0][p:].cuda() for k, p in zip(rest, past)], [], rest, past=past).argmax(-1)
    torch.cuda.synchronize()
    fill_ms = (time.perf_counter() - t0) / n_slots * 1e3
    for _ in range(4):
        ids, _, _ = eng.decode_slots(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ids, _, _ = eng.decode_slots(ids)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ops.start_kernel_timing()
    for _ in range(4):
        ids, _, _ = eng.decode_slots(ids)
    tags = ops.stop_kernel_timing()
    attn = sum(v[1] for k, v in tags.items() if k in ("attn_decode_rope_rows", "attn_decode_rope_shared")) / 4
    return {"prefill_ms_per_example": round(fill_ms, 3), "decode_step_ms": round(ms, 3), "attention_ms_per_step": round(attn, 3),
            "groups": len(eng.group_list), "attention_tag": sorted(k for k in tags if k.startswith("attn_decode"))}


def main_shared(args, slot_list):
    """--questions-per-clip: the inflight schedule on clips with several questions each; with --share-prefix every cell runs twice in
    this process, sharing off then on (the off run first in even cells, the on run first in odd ones)."""
    qs = [int(x) for x in args.questions_per_clip.split(",") if x]
    n_examples = args.examples if args.examples is not None else (256 if max(slot_list) > 16 else 64)
    sets = {q: make_clip_examples(n_examples, q, args.seed) for q in qs}
    max_seq = max(ids.numel() + b for ex in sets.values() for ids, _, b, _ in ex) + 8
    model = RandomLlama(args.precision, max(slot_list), max_seq)
    modes = [False, True] if args.share_prefix else [False]
    for slots in slot_list:                                   # warm-up: every launch sequence once
        for share in modes:
            run_inflight_keys(model, [(i, e, 4, k) for i, e, _, k in sets[qs[-1]][: max(16, slots)]], slots, share)
    res = {"bench": "generate_inflight_shared_prefix", "model": "llama2-7b dims, random weights", "precision": args.precision,
           "examples": n_examples, "min_shared": model.engine.MIN_SHARED, "cells": []}
    for c, (slots, q) in enumerate((s, q) for s in slot_list for q in qs):
        ex = sets[q]
        cell = {"slots": slots, "questions_per_clip": q, "generated_tokens": sum(e[2] for e in ex)}
        outs = {}
        for share in (modes if c % 2 == 0 else modes[::-1]):
            (o, forks), t = timed(lambda: run_inflight_keys(model, ex, slots, share))
            assert all(o[i].numel() == ex[i][0].numel() + ex[i][2] for i in range(len(ex)))
            outs[share] = o
            row = {"s": round(t, 3), "clips_per_s": round(len(ex) / t, 3), "forks": forks}
            row.update(full_step(model, ex, slots, share))
            cell["on" if share else "off"] = row
        if len(modes) == 2:
            cell["outputs_equal"] = sum(torch.equal(outs[True][i].cpu(), outs[False][i].cpu()) for i in range(len(ex)))
            cell["on_over_off"] = {k: round(cell["on"][k] / cell["off"][k], 4)
                                   for k in ("clips_per_s", "decode_step_ms", "attention_ms_per_step", "prefill_ms_per_example")}
        res["cells"].append(cell)
        print(json.dumps(cell), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)


def main_sampling(args, slot_list):
    import statistics

    from llark_amd.m2t.sampling import DeviceSampler, SamplingParams
    steps, blocks = 16, 8
    examples = make_examples(64, args.seed)
    max_seq = max(ids.numel() for ids, _, _ in examples) + 8 + steps * (2 * blocks + 2)
    model = RandomLlama(args.precision, max(slot_list), max_seq)
    eng = model.engine
    sp = SamplingParams(do_sample=True, temperature=0.7, top_k=200, top_p=0.95, repetition_penalty=1.3, seed=args.seed)
    res = {"bench": "generate_inflight_sampling", "model": "llama2-7b dims, random weights", "precision": args.precision,
           "sampling": dict(temperature=0.7, top_k=200, top_p=0.95, repetition_penalty=1.3), "steps_per_block": steps, "blocks": blocks, "slots": {}}
    for n in slot_list:
        eng.init_slots(n)
        rows = [examples[i % len(examples)] for i in range(n)]
        logits = eng.prefill_slots([r[0].cuda() for r in rows], [(k, 1, r[1].cuda()) for k, r in enumerate(rows)], range(n))
        sampler = DeviceSampler(sp, n, logits.shape[-1], eng.device)
        sampler.admit(range(n), [r[0] for r in rows], range(n))
        kinds = {"greedy": None, "sampled": lambda lg: sampler(lg, state=eng.slot_state)}
        ids = logits.argmax(-1)

        def block(kind):
            nonlocal ids
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ids, _, _ = eng.decode_slots(ids, sample=kinds[kind])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        block("greedy"), block("sampled")                        # warm
        ms = {"greedy": [], "sampled": []}
        for b in range(blocks):
            for kind in (("greedy", "sampled") if b % 2 == 0 else ("sampled", "greedy")):
                ms[kind].append(block(kind))
        med = {k: statistics.median(v) for k, v in ms.items()}
        cell = {"greedy_step_ms": round(med["greedy"], 4), "sampled_step_ms": round(med["sampled"], 4),
                "greedy_min_max_ms": [round(min(ms["greedy"]), 4), round(max(ms["greedy"]), 4)],
                "sampled_min_max_ms": [round(min(ms["sampled"]), 4), round(max(ms["sampled"]), 4)],
                "excess_fraction_of_step": round(med["sampled"] / med["greedy"] - 1.0, 4), "fallback_rows": sampler.fallback_count()}
        res["slots"][str(n)] = cell
        print(json.dumps({str(n): cell}), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)


def main_logprobs(args, slot_list):
    import statistics

    from llark_amd import ops
    from llark_amd.m2t.logprob import LogprobTracker
    steps, blocks = 16, 8
    examples = make_examples(64, args.seed)
    max_seq = max(ids.numel() for ids, _, _ in examples) + 8 + steps * (2 * blocks + 2)
    model = RandomLlama(args.precision, max(slot_list), max_seq)
    eng = model.engine
    res = {"bench": "generate_inflight_logprobs", "model": "llama2-7b dims, random weights", "precision": args.precision,
           "steps_per_block": steps, "blocks": blocks, "slots": {}}
    for n in slot_list:
        eng.init_slots(n)
        rows = [examples[i % len(examples)] for i in range(n)]
        logits = eng.prefill_slots([r[0].cuda() for r in rows], [(k, 1, r[1].cuda()) for k, r in enumerate(rows)], range(n))
        tracker = LogprobTracker(n, logits.shape[-1], eng.device, eng.smax)
        choice = torch.zeros((n,), dtype=torch.int64, device=eng.device)

        def with_logprobs(lg):
            toks = ops.sample_rows(lg, choice, state=eng.slot_state, do_sample=False, repetition_penalty=1.0)
            tracker(lg, toks, state=eng.slot_state)
            return toks

        kinds = {"greedy": None, "logprobs": with_logprobs}
        ids = logits.argmax(-1)

        def block(kind):
            nonlocal ids
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ids, _, _ = eng.decode_slots(ids, sample=kinds[kind])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        block("greedy"), block("logprobs")                       # warm
        ms = {"greedy": [], "logprobs": []}
        for b in range(blocks):
            for kind in (("greedy", "logprobs") if b % 2 == 0 else ("logprobs", "greedy")):
                ms[kind].append(block(kind))
        med = {k: statistics.median(v) for k, v in ms.items()}
        taken = tracker.take(range(n))
        assert all(h.numel() == steps * (blocks + 1) and bool(torch.isfinite(h).all()) for h in taken)
        cell = {"greedy_step_ms": round(med["greedy"], 4), "logprobs_step_ms": round(med["logprobs"], 4),
                "greedy_min_max_ms": [round(min(ms["greedy"]), 4), round(max(ms["greedy"]), 4)],
                "logprobs_min_max_ms": [round(min(ms["logprobs"]), 4), round(max(ms["logprobs"]), 4)],
                "excess_fraction_of_step": round(med["logprobs"] / med["greedy"] - 1.0, 4)}
        res["slots"][str(n)] = cell
        print(json.dumps({str(n): cell}), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res), flush=True)


def main_constraints(args, slot_list):
    import statistics

    from llark_amd.m2t.choice import TokenChooser
    from llark_amd.m2t.constraints import TokenConstraints
    steps, blocks = 16, 8
    examples = make_examples(64, args.seed)
    max_seq = max(ids.numel() for ids, _, _ in examples) + 8 + steps * (2 * blocks + 2)
    model = RandomLlama(args.precision, max(slot_list), max_seq)
    eng = model.engine
    tc = TokenConstraints(no_repeat_ngram_size=3, bad_words_ids=[[5], [6, 7]], min_new_tokens=8)
    res = {"bench": "generate_inflight_constraints", "model": "llama2-7b dims, random weights", "precision": args.precision,
           "constraints": dict(no_repeat_ngram_size=3, bad_words=2, min_new_tokens=8, eos=2), "steps_per_block": steps, "blocks": blocks, "slots": {}}
    for n in slot_list:
        eng.init_slots(n)
        rows = [examples[i % len(examples)] for i in range(n)]
        logits = eng.prefill_slots([r[0].cuda() for r in rows], [(k, 1, r[1].cuda()) for k, r in enumerate(rows)], range(n))
        chooser = TokenChooser(n, logits.shape[-1], eng.device, constraints=tc, history_len=eng.smax + 1, eos=2)
        chooser.admit(range(n), [r[0] for r in rows])            # greedy on the processed rows: one constrain_rows + one sample_rows launch
        cons = chooser.cons
        kinds = {"greedy": None, "constrained": lambda lg: chooser(lg, state=eng.slot_state)}
        ids = chooser(logits, state=eng.slot_state)

        def block(kind):                                         # a history holds the constrained blocks' tokens only: the timing is the point
            nonlocal ids
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ids, _, _ = eng.decode_slots(ids, sample=kinds[kind])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        block("greedy"), block("constrained")                    # warm
        ms = {"greedy": [], "constrained": []}
        for b in range(blocks):
            for kind in (("greedy", "constrained") if b % 2 == 0 else ("constrained", "greedy")):
                ms[kind].append(block(kind))
        med = {k: statistics.median(v) for k, v in ms.items()}
        assert not cons.full() and int(cons.hist_len.min()) >= steps * (blocks + 1)
        cell = {"greedy_step_ms": round(med["greedy"], 4), "constrained_step_ms": round(med["constrained"], 4),
                "greedy_min_max_ms": [round(min(ms["greedy"]), 4), round(max(ms["greedy"]), 4)],
                "constrained_min_max_ms": [round(min(ms["constrained"]), 4), round(max(ms["constrained"]), 4)],
                "excess_fraction_of_step": round(med["constrained"] / med["greedy"] - 1.0, 4)}
        res["slots"][str(n)] = cell
        print(json.dumps({str(n): cell}), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res), flush=True)


def main_guided(args, slot_list):
    import statistics

    from llark_amd.m2t.choice import TokenChooser
    from llark_amd.m2t.guide import ChoiceSets
    steps, blocks = 16, 8
    examples = make_examples(64, args.seed)
    max_seq = max(ids.numel() for ids, _, _ in examples) + 8 + steps * (2 * blocks + 2)
    model = RandomLlama(args.precision, max(slot_list), max_seq)
    eng = model.engine
    n_seq, length = 24, steps * (blocks + 1) + 8                 # longer than the guided steps of a run: no slot reaches a leaf
    g = torch.Generator().manual_seed(args.seed)
    res = {"bench": "generate_inflight_guided", "model": "llama2-7b dims, random weights", "precision": args.precision,
           "choice_set": dict(sequences=n_seq, length=length, eos=2), "steps_per_block": steps, "blocks": blocks, "slots": {}}
    for n in slot_list:
        eng.init_slots(n)
        rows = [examples[i % len(examples)] for i in range(n)]
        logits = eng.prefill_slots([r[0].cuda() for r in rows], [(k, 1, r[1].cuda()) for k, r in enumerate(rows)], range(n))
        vocab = logits.shape[-1]
        first = torch.randint(3, vocab, (6,), generator=g).tolist()          # six first tokens: the root and the next nodes fan out
        seqs = [[first[i % 6], 3 + i % 4] + torch.randint(3, vocab, (length - 2,), generator=g).tolist() for i in range(n_seq)]
        chooser = TokenChooser(n, vocab, eng.device, guide=ChoiceSets([seqs]), eos=2)
        chooser.admit(range(n), [r[0] for r in rows], choice=[0] * n)        # greedy on the guided rows: one guide_rows + one sample_rows launch
        kinds = {"greedy": None, "guided": lambda lg: chooser(lg, state=eng.slot_state)}
        ids = chooser(logits, state=eng.slot_state)

        def block(kind):                                         # a node follows the guided blocks' tokens only: the timing is the point
            nonlocal ids
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ids, _, _ = eng.decode_slots(ids, sample=kinds[kind])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        block("greedy"), block("guided")                         # warm
        ms = {"greedy": [], "guided": []}
        for b in range(blocks):
            for kind in (("greedy", "guided") if b % 2 == 0 else ("guided", "greedy")):
                ms[kind].append(block(kind))
        med = {k: statistics.median(v) for k, v in ms.items()}
        chooser.finish()
        assert int(chooser.guide.node.min()) >= 0, "a slot left the tree: the timing is not of guided steps"
        cell = {"greedy_step_ms": round(med["greedy"], 4), "guided_step_ms": round(med["guided"], 4),
                "greedy_min_max_ms": [round(min(ms["greedy"]), 4), round(max(ms["greedy"]), 4)],
                "guided_min_max_ms": [round(min(ms["guided"]), 4), round(max(ms["guided"]), 4)],
                "excess_fraction_of_step": round(med["guided"] / med["greedy"] - 1.0, 4)}
        res["slots"][str(n)] = cell
        print(json.dumps({str(n): cell}), file=sys.stderr, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--guided", action="store_true", help="same-run A/B of the decode step with every slot active: greedy against greedy "
                    "inside a choice set of 24 sequences (default slot counts 16,64)")
    ap.add_argument("--constraints", action="store_true", help="same-run A/B of the decode step with every slot active: greedy against greedy "
                    "under no_repeat_ngram_size 3, two bad words and min_new_tokens (default slot counts 16,64)")
    ap.add_argument("--sampling", action="store_true", help="same-run A/B of the decode step with every slot active: greedy against the "
                    "device sampler (default slot counts 16,64)")
    ap.add_argument("--logprobs", action="store_true", help="same-run A/B of the decode step with every slot active: greedy against greedy + "
                    "token log-probabilities (default slot counts 16,64)")
    ap.add_argument("--out", default=None, help="with --logprobs / --constraints / --guided: also write the JSON here (default "
                    "profiles/bench_generate_inflight_logprobs.json / ..._constraints.json / ..._guided.json)")
    ap.add_argument("--questions-per-clip", default=None, help="e.g. 1,4,8: consecutive examples share an encoding, an audio-first prefix "
                    "and a prefix key (inflight schedule only; one result cell per slot count and value)")
    ap.add_argument("--share-prefix", action="store_true", help="with --questions-per-clip: run every cell with share_prefix off and on")
    ap.add_argument("--slots", default="8,16,32,64", help="slot counts of the inflight schedule, 1 .. 64 each")
    ap.add_argument("--examples", type=int, default=None, help="default: 256 with a slot count above 16, else 64")
    ap.add_argument("--schedules", default="batch1,grouped,inflight", help="which schedules to time")
    ap.add_argument("--precision", default="split", choices=["split", "bf16"])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate_inflight needs the GPU")
    slot_list = [int(x) for x in args.slots.split(",") if x]
    if not slot_list or any(not 1 <= n <= 64 for n in slot_list):
        ap.error(f"--slots takes counts in 1 .. 64, got {args.slots!r}")
    if args.sampling:
        return main_sampling(args, [16, 64] if args.slots == ap.get_default("slots") else slot_list)
    if args.logprobs:
        if args.out is None:
            args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_generate_inflight_logprobs.json")
        return main_logprobs(args, [16, 64] if args.slots == ap.get_default("slots") else slot_list)
    if args.constraints:
        if args.out is None:
            args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_generate_inflight_constraints.json")
        return main_constraints(args, [16, 64] if args.slots == ap.get_default("slots") else slot_list)
    if args.guided:
        if args.out is None:
            args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bench_generate_inflight_guided.json")
        return main_guided(args, [16, 64] if args.slots == ap.get_default("slots") else slot_list)
    if args.questions_per_clip:
        return main_shared(args, slot_list)
    if args.share_prefix:
        ap.error("--share-prefix needs --questions-per-clip")
    schedules = set(args.schedules.split(","))
    n_examples = args.examples if args.examples is not None else (256 if max(slot_list) > 16 else 64)
    step_slots = [n for n in (1, 8, 16, 32, 48, 64) if n <= max(16, max(slot_list))]
    examples = make_examples(n_examples, args.seed)
    max_seq = max(ids.numel() + b for ids, _, b in examples) + 8
    model = RandomLlama(args.precision, max(step_slots), max_seq)
    tok = _NoText()
    gen_tokens = sum(b for _, _, b in examples)
    warm = [(ids, enc, 4) for ids, enc, _ in examples[:16]]
    run_batch1(model, warm[:2], tok)
    run_grouped(model, warm, tok)
    for slots in slot_list:
        run_inflight(model, (warm * 4)[: max(16, slots)], slots)
    res = {"bench": "generate_inflight", "model": "llama2-7b dims, random weights", "precision": args.precision,
           "examples": len(examples), "frames": {"240": sum(e[1].shape[0] == 240 for e in examples),
                                                  "121": sum(e[1].shape[0] == 121 for e in examples)},
           "prompt_tokens": [min(e[0].numel() for e in examples), max(e[0].numel() for e in examples)],
           "generated_tokens": gen_tokens, "schedules": {}}
    outs_a = None
    if "batch1" in schedules:
        outs_a, t = timed(lambda: run_batch1(model, examples, tok))
        res["schedules"]["batch1"] = {"s": round(t, 3), "clips_per_s": round(len(examples) / t, 3), "tokens_per_s": round(gen_tokens / t, 1)}
    if "grouped" in schedules:
        (outs_b, groups), t = timed(lambda: run_grouped(model, examples, tok))
        res["schedules"]["grouped_b8"] = {"s": round(t, 3), "clips_per_s": round(len(examples) / t, 3), "tokens_per_s": round(gen_tokens / t, 1),
                                          "generate_calls": groups, "mean_rows_per_call": round(len(examples) / groups, 2)}
    first = None                                              # without batch1: the first slot count's outputs are what the others are compared to
    for slots in slot_list if "inflight" in schedules else ():
        (outs_c, prefills), t = timed(lambda: run_inflight(model, examples, slots))
        assert all(outs_c[i].numel() == examples[i][0].numel() + examples[i][2] for i in range(len(examples)))
        row = {"s": round(t, 3), "clips_per_s": round(len(examples) / t, 3), "tokens_per_s": round(gen_tokens / t, 1), "prefill_calls": prefills}
        if outs_a is not None:
            row["outputs_equal_to_batch1"] = sum(torch.equal(outs_c[i].cpu(), outs_a[i].cpu()) for i in range(len(examples)))
        elif first is not None:
            row[f"outputs_equal_to_inflight_{slot_list[0]}"] = sum(torch.equal(outs_c[i].cpu(), first[i]) for i in range(len(examples)))
        else:
            first = {i: o.cpu() for i, o in outs_c.items()}
        res["schedules"][f"inflight_{slots}"] = row
    res["decode_step_ms"], res["decode_step_kernels_ms"] = {}, {}
    for n in step_slots:
        ms, split = decode_step_ms(model, examples, n)
        res["decode_step_ms"][str(n)] = round(ms, 3)
        res["decode_step_ms_per_slot"] = {k: round(v / int(k), 4) for k, v in res["decode_step_ms"].items()}
        if split is not None:
            res["decode_step_kernels_ms"][str(n)] = split
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
