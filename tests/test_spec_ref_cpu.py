"""The restatement of the speculative greedy step (tests/spec_ref.py) on the CPU: whatever the drafter proposes, the block loop emits
the plain greedy loop's tokens; and the header, the build list and the ops wrappers carry the new entry points."""
import os
import random
import re

import pytest

import spec_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy_model(seed, vocab, order):
    """a deterministic next-token function of the last ``order`` tokens and the length class: repeats itself often enough that
    the prompt lookup accepts some drafts and rejects others"""
    def f(seq):
        h = seed
        for t in seq[-order:]:
            h = (h * 1000003 + t + 1) % 2147483647
        return h % vocab
    return f


def _drafter(kind, rng, plain, prompt_len, vocab):
    if kind == "lookup":
        return lambda hist: None
    if kind == "random":
        return lambda hist: [rng.randrange(vocab) for _ in range(rng.randrange(0, 9))]
    if kind == "perfect":
        return lambda hist: plain[len(hist) - prompt_len:][:7]
    if kind == "wrong":
        return lambda hist: [(t + 1) % vocab for t in plain[len(hist) - prompt_len:][:7]]
    # scripted: the plain run's tokens, corrupted now and then
    return lambda hist: [t if rng.random() < 0.8 else (t + 1) % vocab for t in plain[len(hist) - prompt_len:][:7]]


KINDS = ["lookup", "random", "perfect", "wrong", "scripted"]


def test_block_loop_equals_plain_loop():
    """2 000 seeded cases over drafters, block sizes, eos, budget and smax cuts"""
    rng = random.Random(20240611)
    seen = {k: [0, 0] for k in KINDS}                       # steps saved / cases, per drafter
    cuts = {"eos": 0, "budget": 0, "smax": 0}
    for case in range(2000):
        vocab = rng.choice([3, 5, 17])
        model = _toy_model(rng.randrange(1 << 30), vocab, rng.choice([1, 2, 3]))
        prompt = [rng.randrange(vocab) for _ in range(rng.randrange(1, 12))]
        max_new = rng.randrange(1, 40)
        eos = rng.choice([-1, 0, 1])
        smax = rng.choice([len(prompt) + rng.randrange(0, 24), 4096])
        k_max = rng.randrange(1, 8)
        stride = rng.randrange(k_max + 1, 9)
        g_max = rng.randrange(1, 5)
        plain = S.plain_loop(model, prompt, max_new, eos, smax)
        kind = KINDS[case % len(KINDS)]
        got, steps = S.block_loop(model, prompt, max_new, eos, smax, stride, k_max, _drafter(kind, rng, plain, len(prompt), vocab), g_max=g_max)
        assert got == plain, (case, kind, prompt, max_new, eos, smax, stride, k_max, got, plain)
        assert steps <= len(plain) and (steps >= 1 or not plain)
        if kind == "perfect":
            assert steps == -(-len(plain) // (k_max + 1)), (case, steps, len(plain), k_max)
        if kind == "wrong" and vocab > 1:
            assert steps == len(plain)
        seen[kind][0] += len(plain) - steps
        seen[kind][1] += 1
        if plain and eos >= 0 and plain[-1] == eos:
            cuts["eos"] += 1
        elif len(plain) == max_new:
            cuts["budget"] += 1
        else:
            cuts["smax"] += 1
    assert all(v > 50 for v in cuts.values()), cuts         # every way a run ends was reached
    assert seen["lookup"][0] > 0 and seen["scripted"][0] > 0 and seen["wrong"][0] == 0, seen


def test_verify_rules():
    pad = 99
    # all accepted: g_0..g_3 emitted
    assert S.verify([5, 6, 7, 8], [1, 5, 6, 7], 4, S.ACTIVE, 10, 100, -1, pad)[:5] == ([5, 6, 7, 8] + [pad] * 4, 4, S.ACTIVE, 14, 96)
    # none accepted: the plain step
    assert S.verify([5, 6, 7, 8], [1, 4, 6, 7], 4, S.ACTIVE, 10, 100, -1, pad)[:2] == ([5] + [pad] * 7, 1)
    # partial; what follows a rejected draft does not count even when it matches
    assert S.verify([5, 6, 7, 8], [1, 5, 0, 7], 4, S.ACTIVE, 10, 100, -1, pad)[:2] == ([5, 6] + [pad] * 6, 2)
    # eos inside the accepted run ends it and finishes the slot
    assert S.verify([5, 6, 7, 8], [1, 5, 6, 7], 4, S.ACTIVE, 10, 100, 6, pad)[:5] == ([5, 6] + [pad] * 6, 2, S.FINISHED, 12, 98)
    # the budget cuts first; an eos behind the cut does not finish the slot
    assert S.verify([5, 6, 7, 8], [1, 5, 6, 7], 4, S.ACTIVE, 10, 2, 7, pad)[:5] == ([5, 6] + [pad] * 6, 2, S.ACTIVE, 12, 0)
    for st in (S.IDLE, S.FINISHED):
        assert S.verify([5, 6], [1, 5], 2, st, 10, 5, -1, pad) == ([pad] * 8, 0, st, 10, 5, None)
    assert S.verify([5, 6], [1, 5], 0, S.ACTIVE, 10, 5, -1, pad)[1] == 0
    hist = [1]
    S.verify([5, 6, 7], [1, 5, 6], 3, S.ACTIVE, 10, 100, -1, pad, hist, ld_hist=3)
    assert hist == [1, 5, 6]                                # the history is cut at ld_hist


def test_argmax_rules():
    nan = float("nan")
    assert S.argmax([1.0, 3.0, 3.0, 2.0]) == 1              # first maximal index
    assert S.argmax([1.0, nan, 5.0, nan]) == 1              # a NaN counts as the maximum, the first one wins
    assert S.argmax([float("-inf")] * 3) == 0
    assert S.argmax([-1.0, float("inf"), float("inf")]) == 1


def test_lookup_rules():
    assert S.lookup([1, 2, 3, 9, 1, 2, 3], 7, 3) == [9, 1, 2, 3]             # the longest suffix; the continuation runs into it
    assert S.lookup([1, 2, 3, 9, 1, 2, 3], 2, 3) == [9, 1]
    assert S.lookup([7, 3, 4, 8, 3, 5, 6, 3], 7, 2) == [5, 6, 3]             # g = 2 has no match, g = 1 takes the MOST RECENT earlier one
    assert S.lookup([1, 2, 3, 4], 7, 2) == []                               # no match
    assert S.lookup([5], 7, 2) == [] and S.lookup([], 7, 2) == []           # shorter than any suffix + 1
    assert S.lookup([5, 5], 7, 2) == [5]                                    # shorter than G + 1: falls to g = 1
    assert S.lookup([4, 4, 4, 4], 7, 2) == [4]                              # most recent earlier start: s = 1, one token follows


def test_draft_caps():
    pad = 0
    assert S.draft(9, S.ACTIVE, 10, 100, 8, 7, 64, pad, drafts=[1, 2, 3]) == ([9, 1, 2, 3, 0, 0, 0, 0], 4)
    assert S.draft(9, S.ACTIVE, 10, 100, 4, 3, 64, pad, drafts=[1, 2, 3, 4, 5]) == ([9, 1, 2, 3], 4)     # k_max
    assert S.draft(9, S.ACTIVE, 10, 2, 4, 3, 64, pad, drafts=[1, 2, 3]) == ([9, 1, 0, 0], 2)              # budget
    assert S.draft(9, S.ACTIVE, 62, 100, 4, 3, 64, pad, drafts=[1, 2, 3]) == ([9, 1, 0, 0], 2)            # pos + blk <= smax
    assert S.draft(9, S.ACTIVE, 64, 100, 4, 3, 64, pad, drafts=[1, 2, 3]) == ([0, 0, 0, 0], 0)
    assert S.draft(9, S.ACTIVE, 10, 0, 4, 3, 64, pad, drafts=[1]) == ([0, 0, 0, 0], 0)
    assert S.draft(9, S.FINISHED, 10, 5, 4, 3, 64, pad, drafts=[1]) == ([0, 0, 0, 0], 0)
    assert S.draft(3, S.ACTIVE, 10, 100, 4, 3, 64, pad, hist=[1, 2, 3, 9, 1, 2, 3]) == ([3, 9, 1, 2], 4)


def test_entry_points_are_declared_built_and_wrapped():
    from llark_amd import _lib, ops
    names = {"llark_attn_decode_rope_bf16_block", "llark_spec_verify_rows", "llark_spec_draft_rows"}
    assert names <= set(_lib.declared_symbols())
    with open(os.path.join(ROOT, "llark_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*=(.*)$", f.read(), re.M).group(1).split()
    assert {"attn_block.hip", "speculate.hip"} <= set(srcs)
    for fn in ("attn_decode_rope_block", "spec_verify_rows", "spec_draft_rows", "spec_step_buffer", "spec_step_views"):
        assert callable(getattr(ops, fn))


def test_speculation_params_validate_and_refuse():
    from llark_amd.m2t.speculate import PromptLookup, SpeculationParams
    assert SpeculationParams.from_generate(None) is None and SpeculationParams.from_generate(0) is None
    assert SpeculationParams.from_generate(None, do_sample=True) is None          # off: nothing else is looked at
    p = SpeculationParams.from_generate(3)
    assert (p.num_tokens, p.max_ngram, p.stride) == (3, 2, 4)
    assert SpeculationParams.from_generate(7, 5, do_sample=False, num_beams=False).max_ngram == 5
    for bad in (8, -1, 2.5, True, "3"):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            SpeculationParams.from_generate(bad)
    for bad in (0, 65, 1.5):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            SpeculationParams.from_generate(2, bad)
    for name in ("do_sample", "temperature", "top_k", "top_p", "seed", "repetition_penalty", "num_beams", "no_repeat_ngram_size", "bad_words_ids",
                 "suppress_tokens", "min_new_tokens", "min_length", "allowed_continuations", "return_logprobs", "share_prefix"):
        with pytest.raises(NotImplementedError, match=name):
            SpeculationParams.from_generate(2, **{name: True})
    p.check_batch(4)
    with pytest.raises(ValueError, match=r"B \* \(K \+ 1\)"):
        p.check_batch(5)
    rng = random.Random(3)
    for _ in range(500):                                                           # the host lookup is the restatement's
        hist = [rng.randrange(4) for _ in range(rng.randrange(0, 20))]
        k, g = rng.randrange(1, 8), rng.randrange(1, 5)
        assert PromptLookup(k, g)(hist) == S.lookup(hist, k, g)
