"""tests/constrain_ref.py against the installed transformers' logits processors (seeded cases), and against hand-written expected sets
from HF 4.29.2's rules where the installed release differs (a multi-token bad word longer than the history) or where the edge matters."""
import numpy as np
import pytest

import constrain_ref as CR


def test_ngram_edges():
    # L = n - 2: the rule does not apply (L + 1 < n); L = n - 1: it applies, the history holds no whole n-gram yet (i runs over
    # 0 .. L - n = -1); L = n: the first history that can ban, through its own first n-gram
    assert CR.banned_set([5], 8, n=3) == set()
    assert CR.banned_set([5, 5], 8, n=3) == set()
    assert CR.banned_set([5, 5, 5], 8, n=3) == {5}
    assert CR.banned_set([5, 5, 6], 8, n=3) == set()
    assert CR.banned_set([], 8, n=2) == set()
    assert CR.banned_set([5], 8, n=2) == set()
    assert CR.banned_set([5, 5], 8, n=2) == {5}
    assert CR.banned_set([1, 2, 1], 8, n=2) == {2}
    assert CR.banned_set([1, 2, 3, 1, 2], 8, n=3) == {3}
    assert CR.banned_set([1, 2, 3, 1, 2], 8, n=4) == set()
    assert CR.banned_set([], 8, n=1) == set()
    assert CR.banned_set([3, 1, 3, 7], 8, n=1) == {1, 3, 7}


def test_ngram_ids_outside_the_vocabulary_compare_but_never_ban():
    assert CR.banned_set([-1, 4, -1], 8, n=2) == {4}
    assert CR.banned_set([4, -1, 4], 8, n=2) == set()                  # the continuation is -1
    assert CR.banned_set([4, 9, 4], 8, n=2) == set()                   # 9 >= vocab


def test_bad_words_tokens_match_of_4_29_2():
    # _tokens_match: a one-token word always; k tokens need the last k - 1 of the history; k - 1 > L: no match
    assert CR.banned_set([], 8, words=[[3]]) == {3}
    assert CR.banned_set([2], 8, words=[[2, 2]]) == {2}
    assert CR.banned_set([2], 8, words=[[1, 2, 2]]) == set()           # longer than the history + 1
    assert CR.banned_set([1, 2], 8, words=[[1, 2, 2]]) == {2}
    assert CR.banned_set([0, 1], 8, words=[[1, 2, 2]]) == set()
    assert CR.banned_set([], 8, words=[[2, 2]]) == set()
    assert CR.banned_set([7, 1], 8, words=[[1, 5], [7, 1, 6], [4]]) == {4, 5, 6}


def test_eos_word_dropped_and_suppress_folded_in():
    assert CR.words_of([[2], [2, 3]], [5, 2], eos=2) == [[2, 3], [5]]
    assert CR.words_of([[2]], [2], eos=-1) == [[2], [2]]
    assert CR.words_of([[2]], (), eos=None) == [[2]]


def test_min_lengths():
    assert CR.banned_set([1, 1, 1], 8, eos=7, prompt_len=3, min_new=2) == {7}
    assert CR.banned_set([1, 1, 1, 4], 8, eos=7, prompt_len=3, min_new=2) == {7}
    assert CR.banned_set([1, 1, 1, 4, 4], 8, eos=7, prompt_len=3, min_new=2) == set()
    assert CR.banned_set([1, 1, 1], 8, eos=7, prompt_len=3, min_len=4) == {7}
    assert CR.banned_set([1, 1, 1, 1], 8, eos=7, prompt_len=3, min_len=4) == set()
    assert CR.banned_set([1], 8, eos=-1, prompt_len=1, min_new=5, min_len=9) == set()      # without an EOS both are no-ops
    assert CR.banned_set([1], 8, eos=None, prompt_len=1, min_new=5, min_len=9) == set()


def test_history_update_with_parents():
    h, full = CR.update_history([[1, 2], [3, 4], [5, 6]], parent=[0, 0, 1], last=[7, 8, 9])
    assert h == [[1, 2, 7], [1, 2, 8], [3, 4, 9]] and not full
    h, full = CR.update_history([[1, 2], [3, 4]], parent=[-1, 5], last=[7, 8], width=2)
    assert h == [[1, 2], [3, 4]] and full
    h, _ = CR.update_history([[1], [2]], last=[7, 8], active=[True, False])
    assert h == [[1, 7], [2]]


def test_processed_row_and_bitmap():
    row = np.array([0.5, -1.0, np.nan, 2.0], dtype=np.float32)
    out = CR.processed_row(row, {1, 3})
    assert out[1] == -np.inf and out[3] == -np.inf and out[0] == np.float32(0.5) and np.isnan(out[2])
    assert CR.bitmap({0, 31, 32, 69}, 70).view(np.uint32).tolist() == [0x80000001, 1, 1 << 5]


def test_against_the_installed_transformers():
    pytest.importorskip("transformers")
    import torch
    from transformers import (MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                              NoRepeatNGramLogitsProcessor)

    rng = np.random.default_rng(20240607)
    mismatches = 0
    for case in range(3000):
        vocab = int(rng.integers(3, 9))
        L = int(rng.integers(3, 31))
        hist = rng.integers(0, vocab, size=L).tolist()
        n = int(rng.integers(1, 5))
        eos = int(rng.integers(0, vocab))
        words = []
        for _ in range(int(rng.integers(1, 4))):
            w = rng.integers(0, vocab, size=int(rng.integers(1, 4))).tolist()
            if w not in words:
                words.append(w)
        prompt_len = int(rng.integers(0, L + 1))
        min_new, min_len = int(rng.integers(0, 8)), int(rng.integers(0, 34))
        ids = torch.tensor([hist], dtype=torch.long)
        scores = torch.zeros((1, vocab))
        hf_words = [w for w in words if w != [eos]]
        procs = [NoRepeatNGramLogitsProcessor(n)]
        if hf_words:
            procs.append(NoBadWordsLogitsProcessor(hf_words, eos_token_id=eos))
        if min_new > 0:
            procs.append(MinNewTokensLengthLogitsProcessor(prompt_len, min_new, eos))
        if min_len > 0:
            procs.append(MinLengthLogitsProcessor(min_len, eos))
        for p in procs:
            scores = p(ids, scores.clone())
        want = {int(t) for t in torch.nonzero(torch.isinf(scores[0]) & (scores[0] < 0)).reshape(-1)}
        got = CR.banned_set(hist, vocab, n=n, words=CR.words_of(words, (), eos), eos=eos, prompt_len=prompt_len, min_new=min_new, min_len=min_len)
        mismatches += got != want
    assert mismatches == 0
