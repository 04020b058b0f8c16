"""GPU: ``generate(prompt_lookup_num_tokens=K)`` on the tiny Llama of tests/test_constrain_generate_gpu.py gives the tokens of the plain
``generate()``, whatever is drafted: lookup drafts, scripted perfect drafts, always-wrong drafts and drafts corrupted at seeded places
(injected through the caller-tensor form of the draft kernel, ``model.speculation_drafter``), uniform and left-padded batches, an EOS
that ends one row early, a stopping criterion that fires inside an accepted run.  The first new token comes from the prefill, so N new
tokens take ceil((N - 1) / (K + 1)) block steps with a perfect drafter and N - 1 with one that is always wrong."""
import random

import pytest
import torch

import test_constrain_generate_gpu as CG
import test_ragged_generate_gpu as LG

pytestmark = pytest.mark.gpu

N = 14


def _inputs(mode):
    rows = [CG._words_prompt(2, 30), CG._words_prompt(4, 17)]
    if mode == "padded":
        ids, mask = LG._padded(rows, True)
        return dict(input_ids=ids.cuda(), attention_mask=mask.cuda()), [30, 17]
    if mode == "single":
        return dict(input_ids=rows[1][None].cuda()), [17]
    return dict(input_ids=torch.stack([rows[0], CG._words_prompt(14, 30)]).cuda()), [30, 30]


def _plain(mode, **kw):
    _, lm = CG._llama()
    inp, _ = _inputs(mode)
    return lm.generate(**inp, max_new_tokens=N, **{"eos_token_id": -1, **kw}).cpu()


def _spec(mode, K, drafter=None, **kw):
    _, lm = CG._llama()
    inp, lens = _inputs(mode)
    stats = {}
    lm.speculation_drafter, lm.speculation_stats = drafter, stats
    try:
        out = lm.generate(**inp, max_new_tokens=N, prompt_lookup_num_tokens=K, **{"eos_token_id": -1, **kw}).cpu()
    finally:
        del lm.speculation_drafter, lm.speculation_stats
    return out, stats, lens


@pytest.mark.parametrize("mode", ["single", "uniform", "padded"])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_lookup_equals_plain(mode, K):
    want = _plain(mode)
    got, stats, _ = _spec(mode, K)
    assert torch.equal(got, want), (got[:, -N:].tolist(), want[:, -N:].tolist())
    assert 1 <= stats["steps"] <= N - 1
    got_g, _, _ = _spec(mode, K, max_matching_ngram_size=4)
    assert torch.equal(got_g, want)


@pytest.mark.parametrize("mode", ["uniform", "padded"])
def test_eos_ends_one_row_early(mode):
    free = _plain(mode)
    S = free.shape[1] - N
    eos = int(free[0, S + 4])                                  # row 0 stops at its fifth token at the latest
    want = _plain(mode, eos_token_id=eos)
    for K in (3, 7):
        got, _, _ = _spec(mode, K, eos_token_id=eos)
        assert torch.equal(got, want), (K, got[:, S:].tolist(), want[:, S:].tolist())
        perfect = lambda b, new: want[b, S + len(new):].tolist()
        got, _, _ = _spec(mode, K, perfect, eos_token_id=eos)
        assert torch.equal(got, want), (K, got[:, S:].tolist(), want[:, S:].tolist())


class _StopAt:
    """fires once the rows hold `n` new tokens; records what it was shown"""

    def __init__(self, S, n):
        self.S, self.n, self.calls = S, n, []

    def __call__(self, ids, scores, **kw):
        self.calls.append((ids.shape[1] - self.S, ids.cpu().clone(), scores.float().cpu().clone()))
        return ids.shape[1] - self.S >= self.n


@pytest.mark.parametrize("mode", ["single", "padded"])
def test_stopping_criterion_inside_an_accepted_run(mode):
    """a perfect drafter with K = 7 accepts 8 tokens per step; the criterion fires at 5: the rest is dropped, the slots go back to the
    state the plain loop leaves (the last kept token is not fed yet: prompt + kept - 1 positions), and the criterion saw the tokens one
    step at a time, each with the logits row it is the argmax of"""
    _, lm = CG._llama()
    free = _plain(mode)
    S = free.shape[1] - N
    plain_stop = _StopAt(S, 5)
    want = _plain(mode, stopping_criteria=[plain_stop])
    stop = _StopAt(S, 5)
    perfect = lambda b, new: free[b, S + len(new):].tolist()
    got, stats, lens = _spec(mode, 7, perfect, stopping_criteria=[stop])
    assert torch.equal(got, want) and got.shape[1] == S + 5
    assert stats["steps"] == 1 and stats["accepted"] >= 4
    assert lm.engine.slot_len_host[: len(lens)] == [n + 5 - 1 for n in lens]
    assert lm.engine.slot_len.cpu().tolist()[: len(lens)] == [n + 5 - 1 for n in lens]
    assert [c[0] for c in stop.calls] == [1, 2, 3, 4, 5] == [c[0] for c in plain_stop.calls]
    for (n, ids, sc), (_, pids, _) in zip(stop.calls, plain_stop.calls):
        assert torch.equal(ids, pids)
        assert sc.argmax(-1).tolist() == ids[:, -1].tolist()


@pytest.mark.parametrize("mode", ["single", "padded"])
@pytest.mark.parametrize("K", [1, 3, 7])
def test_scripted_drafters(mode, K):
    want = _plain(mode)
    S, B = want.shape[1] - N, want.shape[0]
    perfect = lambda b, new: want[b, S + len(new):].tolist()
    got, stats, _ = _spec(mode, K, perfect)
    assert torch.equal(got, want) and stats["steps"] == -(-(N - 1) // (K + 1)), stats
    assert stats["accepted"] == stats["drafted"]
    V = 90
    wrong = lambda b, new: [(t + 1) % V for t in want[b, S + len(new):].tolist()]
    got, stats, _ = _spec(mode, K, wrong)
    assert torch.equal(got, want) and stats["steps"] == N - 1 and stats["accepted"] == 0, stats
    rng = random.Random(7)
    corrupt = lambda b, new: [t if rng.random() < 0.7 else (t + 1) % V for t in want[b, S + len(new):].tolist()]
    got, stats, _ = _spec(mode, K, corrupt)
    assert torch.equal(got, want)
    if K > 1:
        assert 0 < stats["accepted"] < stats["drafted"], stats


def test_off_is_the_plain_run():
    _, lm = CG._llama()
    inp, _ = _inputs("uniform")
    want = _plain("uniform")
    for off in (None, 0):
        assert torch.equal(lm.generate(**inp, max_new_tokens=N, eos_token_id=-1, prompt_lookup_num_tokens=off).cpu(), want)


REFUSED = [dict(do_sample=True), dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(seed=1), dict(repetition_penalty=1.3),
           dict(num_beams=2), dict(no_repeat_ngram_size=2), dict(bad_words_ids=[[5]]), dict(suppress_tokens=[5]), dict(min_new_tokens=2),
           dict(min_length=40), dict(allowed_continuations=[[5, 6]]), dict(return_logprobs=True), dict(share_prefix=True)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: next(iter(kw)))
def test_refused_by_name(kw):
    _, lm = CG._llama()
    inp, _ = _inputs("uniform")
    with pytest.raises(NotImplementedError, match=next(iter(kw))):
        lm.generate(**inp, max_new_tokens=4, eos_token_id=-1, prompt_lookup_num_tokens=3, **kw)


def test_refused_shapes_and_values():
    _, lm = CG._llama()
    inp, _ = _inputs("uniform")
    with pytest.raises(ValueError, match=r"B \* \(K \+ 1\)"):
        lm.generate(input_ids=inp["input_ids"].repeat(2, 1)[:3], max_new_tokens=4, prompt_lookup_num_tokens=7)
    for bad in (8, -1, 2.5, True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            lm.generate(**inp, max_new_tokens=4, prompt_lookup_num_tokens=bad)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        lm.generate(**inp, max_new_tokens=4, prompt_lookup_num_tokens=2, max_matching_ngram_size=0)


def test_refused_on_mpt():
    mm = CG._mpt()
    _, kw, _ = CG._cases()["mpt_uniform"]
    with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
        mm.generate(**kw, prompt_lookup_num_tokens=3)
