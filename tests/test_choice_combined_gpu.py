"""GPU: every stage of the token choice switched on at once -- constraints, the device sampler with a repetition penalty, and token
log-probabilities -- through both wrappers' ``generate`` (uniform and padded) and ``generate_inflight``, on the tiny models and the four
cases of tests/test_constrain_generate_gpu.py.

The replay states the order of the stages (llark_amd/m2t/choice.py): a stopping criterion that never stops taps every step's RAW logits;
tests/constrain_ref.py bans on them from each row's own history (its prompt without padding, then what it generated), a fresh
``DeviceSampler`` admitted with the same prompts and stream ids 0 .. B - 1 draws from those processed rows, and the log-probability is
``ops.token_logprob_rows`` of the raw row.  Tokens are compared exactly, log-probabilities bit for bit."""
import numpy as np
import pytest
import torch

import constrain_ref as CR
import test_constrain_generate_gpu as CG
from kernel_util import bits
from llark_amd import ops

pytestmark = pytest.mark.gpu

SAMPLING = dict(do_sample=True, top_k=8, top_p=0.9, repetition_penalty=1.2, seed=7)
ALL_ON = dict(SAMPLING, no_repeat_ngram_size=2, return_logprobs=True)


def _params():
    from llark_amd.m2t.sampling import SamplingParams
    return SamplingParams(temperature=1.0, **SAMPLING)


@pytest.mark.parametrize("name", CG.CASES)
def test_all_stages_at_once_equal_a_replay_on_the_raw_logits(name):
    from llark_amd.m2t.sampling import DeviceSampler
    m, kw, rows = CG._cases()[name]
    S, B = kw["input_ids"].shape[1], len(rows)
    tap = CG._Tap()
    ids, lps = m.generate(**kw, stopping_criteria=[tap], **ALL_ON)
    assert ids.shape == (B, S + CG.N) and lps.shape == (B, CG.N) and len(tap.steps) == CG.N
    vocab = tap.steps[0][1].shape[-1]
    sampler = DeviceSampler(_params(), B, vocab, "cuda")
    sampler.admit(range(B), rows, range(B))
    active = torch.full((B,), ops.ROW_ACTIVE, dtype=torch.int32, device="cuda")      # eos = -1: no row ever finishes
    host = ids.cpu()
    for t, (seen, scores) in enumerate(tap.steps):
        assert torch.equal(seen, host[:, : S + t + 1])
        processed = np.stack([CR.processed_row(scores[b].numpy(), CR.banned_set(rows[b].tolist() + host[b, S:S + t].tolist(), vocab, n=2))
                              for b in range(B)])
        want = sampler(torch.from_numpy(processed).cuda(), state=active)
        assert want.cpu().tolist() == host[:, S + t].tolist(), f"step {t}: generate chose {host[:, S + t].tolist()}, the replay {want.cpu().tolist()}"
        lp = ops.token_logprob_rows(scores.cuda().contiguous(), ids[:, S + t].contiguous(), torch.zeros((B,), dtype=torch.float32, device="cuda"))
        assert torch.equal(bits(lp), bits(lps[:, t].contiguous())), f"step {t}: not the log-softmax of the raw logits"
    for b in range(B):                                             # the ban did bite on these prompts of repeated words, or at least held
        whole = rows[b].tolist() + host[b, S:].tolist()
        bg = CG._bigrams(whole)[rows[b].numel() - 1:]
        assert not set(bg) & set(CG._bigrams(rows[b].tolist())) and len(set(bg)) == len(bg), f"row {b}: a bigram repeats in {whole}"


def _inflight_examples(kind):
    if kind == "mpt":
        m, _, ex = CG._inflight_examples("mpt")
        return m, ex[:3]                                            # budgets 10, 3, 7
    _, m = CG._llama()
    return m, [(CG._words_prompt(first, length), None, budget) for first, length, budget in ((2, 30, 9), (4, 17, 4), (14, 30, 7))]


@pytest.mark.parametrize("kind", ["llama", "mpt"])
def test_inflight_all_stages_equal_generate_on_the_example_alone(kind):
    """Three examples on two slots: the second one's slot is refilled with the third.  Example i against ``generate`` over i + 1 copies of
    it, left-padded by one column so that they run on the slot mode too: row i there has the stream id i that the example has in flight."""
    from llark_amd.m2t.constraints import TokenConstraints
    from llark_amd.m2t.infer_driver import generate_inflight
    m, ex = _inflight_examples(kind)
    trace = []
    got = {i: (ids, lp) for i, ids, lp in generate_inflight(m, iter(ex), slots=2, max_new_tokens=CG.N, keywords=(), sampling=_params(),
                                                           constraints=TokenConstraints(no_repeat_ngram_size=2), return_logprobs=True,
                                                           trace=trace)}
    assert sorted(got) == [0, 1, 2] and sum(1 for e in trace if e[0] == "prefill") == 2, "no refill happened"
    for i, (prompt, enc, budget) in enumerate(ex):
        n = i + 1
        batch = torch.cat((torch.zeros((n, 1), dtype=torch.int64), prompt[None].repeat(n, 1)), dim=1)
        mask = torch.cat((torch.zeros((n, 1), dtype=torch.int64), torch.ones((n, prompt.numel()), dtype=torch.int64)), dim=1)
        kw = dict(audio_encodings=[enc.cuda()] * n) if enc is not None else {}
        if kind == "llama":
            kw["eos_token_id"] = -1
        ids, lps = m.generate(input_ids=batch.cuda(), attention_mask=mask.cuda(), max_new_tokens=budget, **kw, **ALL_ON)
        fly_ids, fly_lp = got[i]
        k = fly_ids.numel() - prompt.numel()                        # in flight the model's own EOS may end an example before its budget
        assert 1 <= k <= budget and fly_lp.numel() == k
        assert fly_ids[prompt.numel():].tolist() == ids[i, 1 + prompt.numel(): 1 + prompt.numel() + k].cpu().tolist(), f"example {i}"
        assert torch.equal(fly_lp.view(torch.int32), lps[i, :k].cpu().contiguous().view(torch.int32)), f"example {i}: {fly_lp} vs {lps[i, :k]}"
